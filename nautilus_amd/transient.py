"""Transient returns on the GPU: every return of every scan, at its solved pose, classified by the two planes of the
occupancy grid under it -- how many scans stopped around its cell, how many saw through it -- and the returns that are not
transient packed into clouds of the layout every other entry point takes.

The reference has no counterpart (a person walking past is cleaned up by a human with the HITL tool); the filter is this
build's (nhip_transient_filter_dev, kernel unit K19).  The spec -- all integer after the cells, so a numpy restatement pins
it bit for bit (hostside.transient_filter) -- is DESIGN.md section 3, "Transient returns".  Torch tensors are only the
allocator, as in occupancy.py.
"""
import ctypes as C
from collections import namedtuple

import numpy as np

from . import _lib
from ._lib import TransientSpec, check
from .vectorize import pose_affines

LABELS = ("static", "transient", "unobserved", "invalid")
STATS_FIELDS = ("points_static", "points_transient", "points_unobserved", "points_invalid", "scans_processed", "scans_bad_offsets",
                "scans_emptied", "zero")
# what a call returns: the kept points (float32 (kept, 2), bit copies), their offsets per scan (int32 (n_scans + 1,)), the
# index of each in the input cloud (int32 (kept,)), a label per input point (uint8 (n_points,): LABELS) and the stats (int64 (8,))
Filtered = namedtuple("Filtered", "xy offsets index labels stats")
# ... and static_scans(): the same, the occupancy trace's stats (occupancy.STATS_FIELDS) and the planes (int32 (H, W))
StaticScans = namedtuple("StaticScans", "xy offsets index labels stats occupancy_stats hits misses")


def default_spec():
    """nhip_transient_spec_default (works without a device); the window is the caller's to set (spec_from)."""
    s = TransientSpec()
    check(_lib.load().nhip_transient_spec_default(C.byref(s)))
    return s


def spec(**overrides):
    """The defaults with the named fields replaced."""
    s = default_spec()
    for k, v in overrides.items():
        if k not in dict(TransientSpec._fields_):
            raise TypeError("transient.spec: no field %r" % k)
        setattr(s, k, v)
    return s


def spec_from(occupancy_spec, **overrides):
    """spec(**overrides) with the window and the cell size of an occupancy spec: the planes that spec's trace wrote."""
    o = occupancy_spec
    return spec(**dict(dict(res=o.res, cell_x0=o.cell_x0, cell_y0=o.cell_y0, width=o.width, height=o.height), **overrides))


def _outputs(torch, dev, n_scans, n_points):
    cap = max(n_points, 1)
    return (torch.empty(cap, dtype=torch.uint8, device=dev), torch.empty((cap, 2), dtype=torch.float32, device=dev),
            torch.empty(n_scans + 1, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.int32, device=dev),
            torch.empty(8, dtype=torch.int64, device=dev))


def _enqueue(lib, d_xy, d_off, n_scans, n_points, d_aff, spec, d_hits, d_misses, out, sp):
    d_labels, d_out_xy, d_out_off, d_out_idx, d_stats = out
    check(lib.nhip_transient_filter_dev(d_xy.data_ptr(), d_off.data_ptr(), n_scans, n_points, d_aff.data_ptr(), C.byref(spec),
                                        d_hits.data_ptr(), d_misses.data_ptr(), d_labels.data_ptr(), d_out_xy.data_ptr(),
                                        d_out_off.data_ptr(), d_out_idx.data_ptr(), d_stats.data_ptr(), sp))


def _download(out, n_points):
    d_labels, d_out_xy, d_out_off, d_out_idx, d_stats = out
    offsets = d_out_off.cpu().numpy()
    kept = int(offsets[-1])
    return Filtered(d_out_xy[:kept].cpu().numpy(), offsets, d_out_idx[:kept].cpu().numpy(), d_labels[:n_points].cpu().numpy(),
                    d_stats.cpu().numpy())


def _affines(torch, dev, poses, n_scans, who):
    aff = pose_affines(poses)
    if len(aff) != n_scans:
        raise ValueError("%s: %d poses for %d scans" % (who, len(aff), n_scans))
    return torch.from_numpy(aff).to(dev) if n_scans else torch.zeros(4, dtype=torch.float32, device=dev)


def _planes(torch, dev, planes, spec, who):
    shape = (spec.height, spec.width)
    out = []
    for p in planes:
        t = p if isinstance(p, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(p, dtype=np.int32)).to(dev)
        if t.dtype != torch.int32 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
            raise ValueError("%s: planes must be contiguous int32 %s arrays, or tensors on %s" % (who, shape, dev))
        out.append(t)
    return out


def _run_dev(lib, torch, dev, d_xy, d_off, n_scans, n_points, poses, spec, planes):
    d_aff = _affines(torch, dev, poses, n_scans, "transient.filter")
    d_hits, d_misses = _planes(torch, dev, planes, spec, "transient.filter")
    out = _outputs(torch, dev, n_scans, n_points)
    sp = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _enqueue(lib, d_xy, d_off, n_scans, n_points, d_aff, spec, d_hits, d_misses, out, sp)
    check(lib.nhip_dev_status(sp, None))
    return _download(out, n_points)


def _upload(torch, dev, xy, offsets):
    offsets = np.ascontiguousarray(offsets, dtype=np.int32)
    xy = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
    d_xy = torch.from_numpy(xy).to(dev) if len(xy) else torch.zeros(2, dtype=torch.float32, device=dev)
    return d_xy, torch.from_numpy(offsets).to(dev), len(offsets) - 1, len(xy)


def filter(xy, offsets, poses, spec, planes, device="cuda:0"):
    """The packed scans (xy, offsets) at `poses` (n_scans, 3) against planes=(hits, misses) -- host arrays or device tensors,
    int32 (H, W), what occupancy.occupancy_grid returned or worked in; they are read, never written: Filtered.  A scan whose
    offsets are not a scan raises NhipError (nhip_dev_status)."""
    import torch
    dev = torch.device(device)
    d_xy, d_off, n_scans, n_points = _upload(torch, dev, xy, offsets)
    return _run_dev(_lib.load(), torch, dev, d_xy, d_off, n_scans, n_points, poses, spec, planes)


def filter_on_device(d_xy, d_off, n_scans, poses, spec, planes):
    """filter() on scans that already live on the device (torch tensors: float32 xy (n_points, 2), int32 offsets)."""
    import torch
    return _run_dev(_lib.load(), torch, d_xy.device, d_xy, d_off, n_scans, int(d_xy.numel()) // 2, poses, spec, planes)


def filter_on_handle(scans, poses, spec, planes):
    """The handle form (nhip_transient_filter) on a csm.ScanTable: host poses, host planes (numpy int32 (H, W)), host outputs."""
    P = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
    hits, misses = (np.ascontiguousarray(p, dtype=np.int32).reshape(spec.height, spec.width) for p in planes)
    n, cap = scans.n_scans, max(len(scans.xy), 1)
    labels, out_xy = np.zeros(cap, np.uint8), np.zeros((cap, 2), np.float32)
    out_off, out_idx, stats = np.zeros(n + 1, np.int32), np.zeros(cap, np.int32), np.zeros(8, np.int64)
    lib = _lib.load()
    check(lib.nhip_transient_filter(scans._h, _lib.ptr(P), C.byref(spec), _lib.ptr(hits), _lib.ptr(misses), _lib.ptr(labels),
                                    _lib.ptr(out_xy), _lib.ptr(out_off), _lib.ptr(out_idx), _lib.ptr(stats)))
    check(lib.nhip_dev_status(None, None))
    kept = int(out_off[-1])
    return Filtered(out_xy[:kept].copy(), out_off, out_idx[:kept].copy(), labels[:len(scans.xy)].copy(), stats)


def _static_dev(lib, torch, dev, d_xy, d_off, n_scans, n_points, poses, occ_spec, overrides):
    from ._lib import NHIP_OCC_ACCUMULATE
    if occ_spec.flags & NHIP_OCC_ACCUMULATE:
        raise ValueError("transient.static_scans: the trace is this call's own: NHIP_OCC_ACCUMULATE is not taken")
    tspec = spec_from(occ_spec, **overrides)
    d_aff = _affines(torch, dev, poses, n_scans, "transient.static_scans")
    shape = (occ_spec.height, occ_spec.width)
    d_hits, d_misses = (torch.empty(shape, dtype=torch.int32, device=dev) for _ in range(2))
    d_grid = torch.empty(shape, dtype=torch.int8, device=dev)
    d_occ_stats = torch.empty(8, dtype=torch.int64, device=dev)
    out = _outputs(torch, dev, n_scans, n_points)
    sp = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    # trace, then filter, on one stream: the second call reads the planes the first wrote, nothing waits in between
    check(lib.nhip_occupancy_dev(d_xy.data_ptr(), d_off.data_ptr(), d_aff.data_ptr(), n_scans, C.byref(occ_spec), d_hits.data_ptr(),
                                 d_misses.data_ptr(), d_grid.data_ptr(), d_occ_stats.data_ptr(), sp))
    _enqueue(lib, d_xy, d_off, n_scans, n_points, d_aff, tspec, d_hits, d_misses, out, sp)
    check(lib.nhip_dev_status(sp, None))
    f = _download(out, n_points)
    return StaticScans(f.xy, f.offsets, f.index, f.labels, f.stats, d_occ_stats.cpu().numpy(), d_hits.cpu().numpy(),
                       d_misses.cpu().numpy())


def static_scans(xy, offsets, poses, occ_spec, device="cuda:0", **overrides):
    """One occupancy trace of the packed scans at `poses` (occ_spec: an occupancy spec with its window), then the filter on
    the planes it wrote -- spec_from(occ_spec, **overrides) -- in-stream, the planes never leaving the device in between:
    StaticScans, whose (xy, offsets) any entry point takes in place of the input's and whose index gathers normals alongside."""
    import torch
    dev = torch.device(device)
    d_xy, d_off, n_scans, n_points = _upload(torch, dev, xy, offsets)
    return _static_dev(_lib.load(), torch, dev, d_xy, d_off, n_scans, n_points, poses, occ_spec, overrides)


def static_scans_on_device(d_xy, d_off, n_scans, poses, occ_spec, **overrides):
    """static_scans() on scans that already live on the device."""
    import torch
    return _static_dev(_lib.load(), torch, d_xy.device, d_xy, d_off, n_scans, int(d_xy.numel()) // 2, poses, occ_spec, overrides)
