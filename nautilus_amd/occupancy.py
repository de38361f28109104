"""The occupancy grid on the GPU: every scan at its solved pose, free space ray-traced from the sensor to every return,
one observation per scan and cell, classified into ROS OccupancyGrid values (100 occupied, 0 free, -1 unknown).

The reference publishes the merged cloud and stops there; the raster is this build's (nhip_occupancy_dev, kernel unit K14).
The spec -- all integer after the cells, so a numpy restatement pins it bit for bit -- is DESIGN.md section 3, "Occupancy
grid".  Torch tensors are only the allocator, as in vectorize.py.
"""
import ctypes as C

import numpy as np

from . import _lib, hostside
from ._lib import NHIP_OCC_ACCUMULATE, OccupancySpec, check
from .vectorize import pose_affines

STATS_FIELDS = ("scans_traced", "scans_dropped", "beams_traced", "beams_long", "points_dropped", "cells_occupied", "cells_free",
                "cells_unknown")


def default_spec():
    """nhip_occupancy_spec_default (works without a device); the window is the caller's to set (window_spec)."""
    s = OccupancySpec()
    check(_lib.load().nhip_occupancy_spec_default(C.byref(s)))
    return s


def spec(**overrides):
    """The defaults with the named fields replaced."""
    s = default_spec()
    for k, v in overrides.items():
        if k not in dict(OccupancySpec._fields_):
            raise TypeError("occupancy.spec: no field %r" % k)
        setattr(s, k, v)
    return s


def window_spec(poses, range_m=30.0, **overrides):
    """spec(**overrides) with the smallest window that holds every pose +- range_m (hostside.map_window)."""
    s = spec(**overrides)
    s.cell_x0, s.cell_y0, s.width, s.height = hostside.map_window(poses, range_m, s.res)
    return s


def _run_dev(lib, torch, dev, d_xy, d_off, n_scans, poses, spec, planes):
    """nhip_occupancy_dev on device tensors; (grid, hits, misses, stats) as numpy arrays."""
    aff = pose_affines(poses)
    if len(aff) != n_scans:
        raise ValueError("occupancy_grid: %d poses for %d scans" % (len(aff), n_scans))
    shape = (spec.height, spec.width)
    accumulate = bool(spec.flags & NHIP_OCC_ACCUMULATE)
    if planes is None:
        if accumulate:
            raise ValueError("occupancy_grid: NHIP_OCC_ACCUMULATE needs planes=(hits, misses) to add onto")
        d_hits, d_misses = (torch.empty(shape, dtype=torch.int32, device=dev) for _ in range(2))
    else:
        d_hits, d_misses = planes
        for t in (d_hits, d_misses):
            if t.dtype != torch.int32 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
                raise ValueError("occupancy_grid: planes must be contiguous int32 %s tensors on %s" % (shape, dev))
    d_aff = torch.from_numpy(aff).to(dev) if n_scans else torch.zeros(4, dtype=torch.float32, device=dev)
    d_grid = torch.empty(shape, dtype=torch.int8, device=dev)
    d_stats = torch.empty(8, dtype=torch.int64, device=dev)
    sp = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    check(lib.nhip_occupancy_dev(d_xy.data_ptr(), d_off.data_ptr(), d_aff.data_ptr(), n_scans, C.byref(spec), d_hits.data_ptr(),
                                 d_misses.data_ptr(), d_grid.data_ptr(), d_stats.data_ptr(), sp))
    check(lib.nhip_dev_status(sp, None))
    return d_grid.cpu().numpy(), d_hits.cpu().numpy(), d_misses.cpu().numpy(), d_stats.cpu().numpy()


def occupancy_grid(xy, offsets, poses, spec, device="cuda:0", planes=None):
    """The grid of the packed scans (xy, offsets) at `poses` (n_scans, 3): (grid int8 (H, W), hits int32 (H, W), misses int32
    (H, W), stats int64 (8,): STATS_FIELDS).  planes=(hits, misses): device tensors (int32, (H, W)) the call works in -- with
    NHIP_OCC_ACCUMULATE in spec.flags it adds onto what they hold, so a map can be built from batches of scans; without the
    flag they are cleared first.  A scan whose offsets are not a scan raises NhipError (nhip_dev_status)."""
    import torch
    lib, dev = _lib.load(), torch.device(device)
    offsets = np.ascontiguousarray(offsets, dtype=np.int32)
    xy = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
    n_scans = len(offsets) - 1
    d_xy = torch.from_numpy(xy).to(dev) if len(xy) else torch.zeros(2, dtype=torch.float32, device=dev)
    d_off = torch.from_numpy(offsets).to(dev)
    return _run_dev(lib, torch, dev, d_xy, d_off, n_scans, poses, spec, planes)


def occupancy_grid_on_device(d_xy, d_off, n_scans, poses, spec, planes=None):
    """occupancy_grid() on scans that already live on the device (torch tensors: float32 xy, int32 offsets)."""
    import torch
    return _run_dev(_lib.load(), torch, d_xy.device, d_xy, d_off, n_scans, poses, spec, planes)


def occupancy_grid_on_handle(scans, poses, spec, planes=None):
    """The handle form (nhip_occupancy) on a csm.ScanTable: host poses, host outputs.  planes=(hits, misses): numpy int32
    (H, W) arrays that NHIP_OCC_ACCUMULATE adds onto (they are not modified; the sums are returned)."""
    P = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
    shape = (spec.height, spec.width)
    if planes is None:
        if spec.flags & NHIP_OCC_ACCUMULATE:
            raise ValueError("occupancy_grid_on_handle: NHIP_OCC_ACCUMULATE needs planes=(hits, misses) to add onto")
        hits, misses = np.zeros(shape, np.int32), np.zeros(shape, np.int32)
    else:
        hits, misses = (np.array(p, dtype=np.int32, order="C").reshape(shape) for p in planes)
    grid, stats = np.zeros(shape, np.int8), np.zeros(8, np.int64)
    check(_lib.load().nhip_occupancy(scans._h, _lib.ptr(P), C.byref(spec), _lib.ptr(hits), _lib.ptr(misses), _lib.ptr(grid),
                                     _lib.ptr(stats)))
    check(_lib.load().nhip_dev_status(None, None))
    return grid, hits, misses, stats
