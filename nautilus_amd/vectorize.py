"""The vector map on the GPU: every scan at its solved pose, merged, reduced to wall segments.

  Solver::Vectorize                       src/optimization/solver.cc:581-624 (VectorMaps::ExtractLines: third_party/vector_maps,
    -> nhip_vectorize_dev                 an empty directory in the reference tree)
The spec -- an exhaustive, deterministic Hough transform over the occupied cells of a world raster with greedy peak
extraction, all integer after the point transform -- is DESIGN.md section 3, "Map vectorisation".  Torch tensors are only
the allocator, as in normals.py.
"""
import ctypes as C

import numpy as np

from . import _lib, hostside
from ._lib import VectorizeLayout, VectorizeSpec, check

RECORD_FIELDS = ("t", "b", "a_lo", "a_hi", "n", "sum_x", "sum_y", "sum_xx", "sum_xy", "sum_yy")
STATS_FIELDS = ("cells", "segments", "rounds", "flag", "emitted", "retired", "n_rho", "zero")
MAX_ROUNDS = 2 ** 31 - 1  # (every round kills a cell: a call ends after at most M of them)


def default_spec():
    """nhip_vectorize_spec_default (works without a device); the window is the caller's to set (window_spec)."""
    s = VectorizeSpec()
    check(_lib.load().nhip_vectorize_spec_default(C.byref(s)))
    return s


def spec(**overrides):
    """The defaults with the named fields replaced."""
    s = default_spec()
    for k, v in overrides.items():
        if k not in dict(VectorizeSpec._fields_):
            raise TypeError("vectorize.spec: no field %r" % k)
        setattr(s, k, v)
    return s


def window_spec(poses, range_m=30.0, **overrides):
    """spec(**overrides) with the smallest window that holds every pose +- range_m (hostside.map_window)."""
    s = spec(**overrides)
    s.cell_x0, s.cell_y0, s.width, s.height = hostside.map_window(poses, range_m, s.res)
    return s


def tables(spec):
    """(C, S): int32 (n_theta,) each (nhip_vectorize_tables; pure host)."""
    c, s = np.zeros(spec.n_theta, np.int32), np.zeros(spec.n_theta, np.int32)
    check(_lib.load().nhip_vectorize_tables(C.byref(spec), _lib.ptr(c), _lib.ptr(s)))
    return c, s


def pose_affines(poses):
    """float32 (n, 4): (cos, sin, x, y) of every pose, rounded from double (nhip_map_pose_affines; pure host)."""
    P = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
    out = np.zeros((len(P), 4), np.float32)
    check(_lib.load().nhip_map_pose_affines(_lib.ptr(P), len(P), _lib.ptr(out)))
    return out


def workspace_layout(spec, max_cells):
    L = VectorizeLayout()
    check(_lib.load().nhip_vectorize_workspace_layout(C.byref(spec), int(max_cells), C.byref(L)))
    return L


def endpoints(spec, records):
    """float32 (n, 4) lines x1 y1 x2 y2 in metres from the records (nhip_vectorize_endpoints; pure host)."""
    rec = np.ascontiguousarray(records, dtype=np.int64).reshape(-1, 10)
    lines = np.zeros((len(rec), 4), np.float32)
    check(_lib.load().nhip_vectorize_endpoints(C.byref(spec), _lib.ptr(rec), len(rec), _lib.ptr(lines)))
    return lines


def _run_dev(lib, torch, dev, d_xy, d_off, n_scans, poses, spec, max_cells, max_rounds, check_every, planes):
    """nhip_vectorize_dev on device tensors; (lines, records, stats[, planes])."""
    if max_cells is None:
        max_cells = min(spec.width * spec.height, 1 << 26)
    L = workspace_layout(spec, max_cells)
    aff = pose_affines(poses)
    if len(aff) != n_scans:
        raise ValueError("vectorize: %d poses for %d scans" % (len(aff), n_scans))
    d_aff = torch.from_numpy(aff).to(dev) if n_scans else torch.zeros(4, dtype=torch.float32, device=dev)
    d_ws = torch.empty(L.bytes + 256, dtype=torch.uint8, device=dev)
    ws = d_ws[(-d_ws.data_ptr()) % 256:][:L.bytes]
    d_rec = torch.zeros(10 * max(spec.max_segments, 1), dtype=torch.int64, device=dev)
    d_stats = torch.zeros(8, dtype=torch.int32, device=dev)
    sp = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    check(lib.nhip_vectorize_dev(d_xy.data_ptr(), d_off.data_ptr(), d_aff.data_ptr(), n_scans, C.byref(spec), int(max_cells),
                                 int(max_rounds), int(check_every), d_rec.data_ptr(), d_stats.data_ptr(), ws.data_ptr(),
                                 L.bytes, sp))
    check(lib.nhip_dev_status(sp, None))
    stats = d_stats.cpu().numpy().copy()
    rec = d_rec[:10 * int(stats[1])].cpu().numpy().reshape(-1, 10).copy()
    out = (endpoints(spec, rec), rec, stats)
    if planes:
        M = min(int(stats[0]), int(max_cells)) if stats[3] != 3 else 0
        view = lambda off, n, dt: ws[off:off + n * np.dtype(dt).itemsize].cpu().numpy().view(dt).copy()
        out += ({"counts": view(L.counts_offset, spec.width * spec.height, np.int32).reshape(spec.height, spec.width),
                 "cells": view(L.cells_offset, 2 * M, np.int32).reshape(M, 2),
                 "votes": view(L.votes_offset, spec.n_theta * L.n_rho, np.int32).reshape(spec.n_theta, L.n_rho),
                 "live": view(L.live_offset, M, np.uint8)},)
    return out


def vectorize(xy, offsets, poses, spec, device="cuda:0", planes=False, max_cells=None, max_rounds=MAX_ROUNDS, check_every=8):
    """The segments of the packed scans (xy, offsets) at `poses` (n_scans, 3): (lines float32 (n, 4), records int64 (n, 10),
    stats int32 (8,)); with planes=True also the dict of the workspace's planes after the call -- counts, cells, votes (of
    the cells still live), live.  max_rounds=0 with planes=True shows the initial votes.  stats[3] is the flag: 0 ended below
    min_votes, 1 max_rounds, 2 max_segments (the stopping round committed nothing), 3 more than max_cells cells (stats[0]: the
    count needed).  A scan whose offsets are not a scan raises NhipError (nhip_dev_status)."""
    import torch
    lib, dev = _lib.load(), torch.device(device)
    offsets = np.ascontiguousarray(offsets, dtype=np.int32)
    xy = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
    n_scans = len(offsets) - 1
    d_xy = torch.from_numpy(xy).to(dev) if len(xy) else torch.zeros(2, dtype=torch.float32, device=dev)
    d_off = torch.from_numpy(offsets).to(dev)
    return _run_dev(lib, torch, dev, d_xy, d_off, n_scans, poses, spec, max_cells, max_rounds, check_every, planes)


def vectorize_on_device(d_xy, d_off, n_scans, poses, spec, max_cells=None, max_rounds=MAX_ROUNDS, check_every=8):
    """vectorize() on scans that already live on the device (torch tensors: float32 xy, int32 offsets)."""
    import torch
    return _run_dev(_lib.load(), torch, d_xy.device, d_xy, d_off, n_scans, poses, spec, max_cells, max_rounds, check_every, False)


def vectorize_on_handle(scans, poses, spec, max_cells=None, max_rounds=MAX_ROUNDS, check_every=8):
    """The handle form (nhip_vectorize) on a csm.ScanTable: (lines, records, stats)."""
    if max_cells is None:
        max_cells = min(spec.width * spec.height, 1 << 26)
    P = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
    rec = np.zeros((max(spec.max_segments, 1), 10), np.int64)
    stats = np.zeros(8, np.int32)
    check(_lib.load().nhip_vectorize(scans._h, _lib.ptr(P), C.byref(spec), int(max_cells), int(max_rounds), int(check_every),
                                     _lib.ptr(rec), _lib.ptr(stats)))
    rec = rec[:int(stats[1])].copy()
    return endpoints(spec, rec), rec, stats
