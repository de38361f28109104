"""Scans localised in a finished occupancy grid: "here is a scan and a rough pose, where in this map am I?"

The map is what HipBackend.occupancy_grid built and hostside.write_occupancy_map saved; the matcher is the correlative one
every loop closure goes through.  This module joins them: the occupied cells of the grid around each prior pose become a
target cloud on the device (nhip_mapwin_cells_dev, nhip_mapwin_gather_dev: kernel unit K20), nhip_grid_build_dev builds the
tables on those clouds, nhip_csm_match_dev matches every scan against its own, and the records are composed into world poses
on the host.  The reference has no such step; the spec is DESIGN.md section 3, "Map windows", and hostside.map_cells /
map_windows / localize restate it in numpy for any backend.  Torch tensors are only the allocator, as in occupancy.py.
"""
import ctypes as C
import math

import numpy as np

from . import _lib, csm, hostside
from ._lib import MapwinSpec, check

STATS_FIELDS = ("cells_occupied", "queries", "points_stored", "windows_empty", "largest_window", "cells_overflow", "points_overflow",
                "zero")
KIND_CELLS, KIND_POINTS = 524288, 1048576  # nhip_dev_status: the cell list / the windows did not fit


def default_spec():
    """nhip_mapwin_spec_default (works without a device); the map's window and the side are the caller's to set (spec)."""
    s = MapwinSpec()
    check(_lib.load().nhip_mapwin_spec_default(C.byref(s)))
    return s


def spec(occ_spec, grid_spec, occ_min=100):
    """The window spec of a map (occ_spec: an occupancy spec, or anything with res and the window) for tables of grid_spec:
    side = grid_layout(grid_spec).side.  ValueError if the two cell sizes differ: a window is a crop, nothing is resampled."""
    if float(grid_spec.res) != float(occ_spec.res):
        raise ValueError("localize.spec: the tables' res %r is not the map's %r" % (float(grid_spec.res), float(occ_spec.res)))
    s = default_spec()
    s.res, s.cell_x0, s.cell_y0, s.width, s.height = float(occ_spec.res), occ_spec.cell_x0, occ_spec.cell_y0, occ_spec.width, occ_spec.height
    s.side, s.occ_min = csm.grid_layout(grid_spec).side, int(occ_min)
    return s


def origins(priors, res):
    """nhip_mapwin_origins (pure host): (origins int32 (n, 2), theta0 float64 (n,)) of priors (n, 3)."""
    P = np.ascontiguousarray(priors, dtype=np.float64).reshape(-1, 3)
    org, th = np.zeros((len(P), 2), np.int32), np.zeros(len(P), np.float64)
    check(_lib.load().nhip_mapwin_origins(_lib.ptr(P), len(P), float(res), _lib.ptr(org), _lib.ptr(th)))
    return org, th


def compose(records, origins, theta0, grid_spec, search):
    """World poses (n, 3) float64 from the records of matches against map windows; NaN for a rejected record
    (hostside.localize_compose: the one statement of item 6 of the spec)."""
    return hostside.localize_compose(records, origins, theta0, grid_spec, search)


def _stream(torch, dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _grid_tensor(torch, dev, grid, mw):
    if isinstance(grid, torch.Tensor):
        if grid.dtype != torch.int8 or tuple(grid.shape) != (mw.height, mw.width) or not grid.is_contiguous() or grid.device != dev:
            raise ValueError("localize: the grid must be a contiguous int8 (%d, %d) tensor on %s" % (mw.height, mw.width, dev))
        return grid
    g = np.ascontiguousarray(grid, dtype=np.int8)
    if g.shape != (mw.height, mw.width):
        raise ValueError("localize: grid of shape %s for a window of %d x %d" % (g.shape, mw.height, mw.width))
    return torch.from_numpy(g).to(dev)


def map_cells_on_device(d_grid, mw, max_cells=None, d_stats=None):
    """nhip_mapwin_cells_dev on a device grid (int8 (H, W) tensor), enqueued on torch's current stream: (d_row_ptr int32
    (H + 1,), d_cols int32 (max_cells,), d_stats int64 (8,)).  max_cells=None: counted from the grid (one reduction on the
    device, which waits for it)."""
    import torch
    dev = d_grid.device
    if max_cells is None:
        max_cells = int((d_grid >= int(mw.occ_min)).sum().item())
    d_row_ptr = torch.empty(mw.height + 1, dtype=torch.int32, device=dev)
    d_cols = torch.empty(max(int(max_cells), 1), dtype=torch.int32, device=dev)
    d_stats = torch.empty(8, dtype=torch.int64, device=dev) if d_stats is None else d_stats
    check(_lib.load().nhip_mapwin_cells_dev(d_grid.data_ptr(), C.byref(mw), int(max_cells), d_row_ptr.data_ptr(), d_cols.data_ptr(),
                                            d_stats.data_ptr(), _stream(torch, dev)))
    return d_row_ptr, d_cols, d_stats


def map_cells(grid, mw, device="cuda:0", max_cells=None):
    """The occupied cells of a grid (host array or device tensor), row by row, made on the GPU: (row_ptr int32 (H + 1,), cols
    int32 (n_occ,), stats int64 (8,)).  More cells than max_cells raises NhipError (kind 524288)."""
    import torch
    dev = torch.device(device)
    d_row_ptr, d_cols, d_stats = map_cells_on_device(_grid_tensor(torch, dev, grid, mw), mw, max_cells)
    check(_lib.load().nhip_dev_status(_stream(torch, dev), None))
    row_ptr = d_row_ptr.cpu().numpy()
    return row_ptr, d_cols[:int(row_ptr[-1])].cpu().numpy(), d_stats.cpu().numpy()


def windows_on_device(d_row_ptr, d_cols, mw, d_origins, n_queries, capacity, d_stats=None):
    """nhip_mapwin_gather_dev on device buffers (d_origins: int32 (n_queries, 2)), enqueued on torch's current stream: (d_xy
    float32 (max(capacity, 1), 2), d_offsets int32 (n_queries + 1,), d_stats int64 (8,)).  Nothing waits; the caller asks
    nhip_dev_status where it synchronises anyway."""
    import torch
    dev, lib = d_row_ptr.device, _lib.load()
    d_xy = torch.empty((max(int(capacity), 1), 2), dtype=torch.float32, device=dev)
    d_off = torch.empty(n_queries + 1, dtype=torch.int32, device=dev)
    d_stats = torch.empty(8, dtype=torch.int64, device=dev) if d_stats is None else d_stats
    ws = lib.nhip_mapwin_workspace_bytes(n_queries)
    d_ws = torch.empty(ws, dtype=torch.uint8, device=dev)
    check(lib.nhip_mapwin_gather_dev(d_row_ptr.data_ptr(), d_cols.data_ptr(), C.byref(mw), d_origins.data_ptr() if n_queries else None,
                                     n_queries, d_xy.data_ptr(), int(capacity), d_off.data_ptr(), d_stats.data_ptr(), d_ws.data_ptr(), ws,
                                     _stream(torch, dev)))
    return d_xy, d_off, d_stats


def _origin_tensor(torch, dev, org):
    org = np.ascontiguousarray(org, dtype=np.int32).reshape(-1, 2)
    return (torch.from_numpy(org).to(dev) if len(org) else torch.zeros((1, 2), dtype=torch.int32, device=dev)), len(org)


def windows(grid, mw, origins, device="cuda:0", capacity=None):
    """The windows of a grid (host array or device tensor) around origins (n, 2), gathered on the GPU: (xy float32 (n_points,
    2), offsets int32 (n + 1,), stats int64 (8,): STATS_FIELDS) -- hostside.map_windows' three arrays bit for bit.
    capacity=None: n x min(occupied cells, side^2) points, which always fits; a smaller one that does not raises NhipError
    (kind 1048576), as a cell list that does not fit does."""
    import torch
    dev = torch.device(device)
    d_row_ptr, d_cols, d_stats = map_cells_on_device(_grid_tensor(torch, dev, grid, mw), mw)
    d_org, n = _origin_tensor(torch, dev, origins)
    if capacity is None:
        capacity = n * min(int(d_cols.numel()), mw.side * mw.side)
    d_xy, d_off, d_stats = windows_on_device(d_row_ptr, d_cols, mw, d_org, n, capacity, d_stats)
    check(_lib.load().nhip_dev_status(_stream(torch, dev), None))
    off = d_off.cpu().numpy()
    return d_xy[:int(off[-1])].cpu().numpy(), off, d_stats.cpu().numpy()


def windows_host_form(grid, mw, origins, capacity):
    """The host form (nhip_map_windows): host grid, host origins, host outputs; (xy, offsets, stats)."""
    g = np.ascontiguousarray(grid, dtype=np.int8).reshape(mw.height, mw.width)
    org = np.ascontiguousarray(origins, dtype=np.int32).reshape(-1, 2)
    xy, off, stats = np.zeros((max(int(capacity), 1), 2), np.float32), np.zeros(len(org) + 1, np.int32), np.zeros(8, np.int64)
    check(_lib.load().nhip_map_windows(_lib.ptr(g), C.byref(mw), _lib.ptr(org) if len(org) else None, len(org), _lib.ptr(xy),
                                       int(capacity), _lib.ptr(off), _lib.ptr(stats)))
    return xy[:int(off[-1])].copy(), off, stats


def localize(xy, offsets, priors, grid, occ_spec, grid_spec=None, search=None, min_score=None, cell_bits=16, occ_min=100,
             device="cuda:0", max_slots=128, timings=None):
    """Scan q of the packed scans (xy, offsets) localised in `grid` (int8 (H, W): what occupancy_grid returned or
    read_occupancy_map read; occ_spec: its window and res -- an occupancy spec, or a window spec made by spec()) from priors[q]
    (x, y, heading).  The device path is the submap branch of HipBackend.match with the window gather in the place of the
    submap gather: the scans go up as the sources, the windows of the distinct origins are gathered into buffers of their
    own (queries whose priors share a world cell share one window and one table), nhip_grid_build_dev builds tables on those,
    nhip_csm_match_dev (min_score given: nhip_csm_match_gated_dev) matches with theta0 = the priors' headings.  Tables of
    max_slots origins are on the device at a time (a table of config #2 is 12 MB).
    grid_spec, search: BASELINE config #2's table and lattice (30 m / 0.05 m, 61 x 81 x 81) unless given.  ValueError for a
    grid_spec whose res is not the map's, or a window spec whose side is not the layout's.
    Returns {"poses": (Q, 3) float64 world poses, NaN where rejected; "records": MATCH_DTYPE (Q,); "origins": int32 (Q, 2);
    "rejected": bool (Q,); "points_per_window": int32 (Q,)}.  timings: a dict that receives the seconds of cells, gather,
    build and match, each behind a wait (measurements only; None: nothing waits between the steps)."""
    import torch
    lib, dev = _lib.load(), torch.device(device)
    gs = csm.grid_spec(30.0, 0.05, 2.0, 1e-10, 40, cell_bits) if grid_spec is None else grid_spec
    srch = csm.search_spec(61, 81, 81, math.radians(1.0)) if search is None else \
        _lib.Search(search.n_theta, search.nx, search.ny, search.flags, search.theta_step)
    side, slot_bytes = csm.grid_layout(gs).side, csm.grid_layout(gs).slot_bytes
    if hasattr(occ_spec, "side"):
        if occ_spec.side != side:
            raise ValueError("localize: the window spec's side %d is not the tables' %d" % (occ_spec.side, side))
        if float(occ_spec.res) != float(gs.res):
            raise ValueError("localize: the tables' res %r is not the map's %r" % (float(gs.res), float(occ_spec.res)))
        mw = occ_spec
    else:
        mw = spec(occ_spec, gs, occ_min)
    off = np.ascontiguousarray(offsets, dtype=np.int32)
    Q = len(off) - 1
    P = np.ascontiguousarray(priors, dtype=np.float64).reshape(-1, 3)
    if len(P) != Q:
        raise ValueError("localize: %d priors for %d scans" % (len(P), Q))
    org, theta0 = origins(P, mw.res)
    rec = np.zeros(Q, dtype=csm.MATCH_DTYPE)
    ppw = np.zeros(Q, np.int32)
    if Q == 0:
        return {"poses": np.zeros((0, 3)), "records": rec, "origins": org, "rejected": np.zeros(0, bool), "points_per_window": ppw}
    uniq, slot = np.unique(org, axis=0, return_inverse=True)
    slot = np.asarray(slot).reshape(-1)
    xy = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
    if int(np.diff(off).max()) <= _lib.NHIP_SHORT_SCAN_POINTS:
        srch.flags |= _lib.NHIP_SEARCH_SHORT_SCANS
    clock = _Clock(torch, dev, timings)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_sxy = t(xy) if len(xy) else torch.zeros((1, 2), dtype=torch.float32, device=dev)
    d_soff, d_delta = t(off), t(csm.delta_table(srch))
    rot0 = np.empty((Q, 2))
    check(lib.nhip_csm_rot0(_lib.ptr(theta0), None, Q, _lib.ptr(rot0)))
    sp = _stream(torch, dev)
    d_grid = _grid_tensor(torch, dev, grid, mw)
    clock.start()
    d_row_ptr, d_cols, d_stats = map_cells_on_device(d_grid, mw)
    clock.stop("cells")
    n_occ = int(d_cols.numel())
    order = np.argsort(slot, kind="stable")  # the queries by slot: a batch is a run of them
    max_slots = max(int(max_slots), 1)
    n_batch = min(max_slots, len(uniq))
    d_tables = torch.empty(lib.nhip_grids_bytes(C.byref(gs), n_batch), dtype=torch.uint8, device=dev)
    ws_g = lib.nhip_grid_workspace_bytes(C.byref(gs), n_batch)
    d_ws_g = torch.empty(ws_g, dtype=torch.uint8, device=dev)
    d_gids = torch.arange(n_batch, dtype=torch.int32, device=dev)
    for s0 in range(0, len(uniq), max_slots):
        s1 = min(s0 + max_slots, len(uniq))
        ns = s1 - s0
        q = order[np.searchsorted(slot[order], s0, "left"):np.searchsorted(slot[order], s1, "left")]
        n = len(q)
        d_org, _ = _origin_tensor(torch, dev, uniq[s0:s1])
        clock.start()
        d_wxy, d_woff, _ = windows_on_device(d_row_ptr, d_cols, mw, d_org, ns, ns * min(n_occ, side * side), d_stats)
        clock.stop("gather")
        # (nhip_grid_build_dev zero-fills the slots itself; only the 256 bytes of read slack behind them are this caller's)
        d_tables[ns * slot_bytes:ns * slot_bytes + 256].zero_()
        clock.start()
        check(lib.nhip_grid_build_dev(d_wxy.data_ptr(), d_woff.data_ptr(), ns, d_gids.data_ptr(), ns, C.byref(gs), d_tables.data_ptr(),
                                      d_ws_g.data_ptr(), ws_g, sp))
        clock.stop("build")
        d_src, d_slot, d_rot0 = t(q.astype(np.int32)), t((slot[q] - s0).astype(np.int32)), t(rot0[q])
        ws_m = lib.nhip_csm_workspace_bytes(n)
        d_ws_m = torch.empty(ws_m, dtype=torch.uint8, device=dev)
        d_keys = torch.empty(n, dtype=torch.int64, device=dev)
        d_out = torch.empty((n, 4), dtype=torch.int32, device=dev)
        args = (d_sxy.data_ptr(), d_soff.data_ptr(), Q, d_tables.data_ptr(), ns, C.byref(gs), d_src.data_ptr(), d_slot.data_ptr(),
                d_rot0.data_ptr(), d_delta.data_ptr(), None, n, C.byref(srch), d_keys.data_ptr(), d_out.data_ptr(), None,
                d_ws_m.data_ptr(), ws_m, sp)
        clock.start()
        if min_score is None:
            check(lib.nhip_csm_match_dev(*args))
        else:
            check(lib.nhip_csm_match_gated_dev(*args, float(min_score)))
        clock.stop("match")
        rec[q] = d_out.cpu().numpy().view(csm.MATCH_DTYPE).reshape(-1)
        ppw[q] = np.diff(d_woff.cpu().numpy())[slot[q] - s0]
    check(lib.nhip_dev_status(sp, None))
    return {"poses": compose(rec, org, theta0, gs, srch), "records": rec, "origins": org, "rejected": csm.rejected(rec),
            "points_per_window": ppw}


class _Clock:
    """Seconds per step into a dict, each step between two waits for the device; without a dict nothing waits."""

    def __init__(self, torch, dev, out):
        self.torch, self.dev, self.out, self.t0 = torch, dev, out, 0.0

    def start(self):
        if self.out is not None:
            import time
            self.torch.cuda.synchronize(self.dev)
            self.t0 = time.perf_counter()

    def stop(self, key):
        if self.out is not None:
            import time
            self.torch.cuda.synchronize(self.dev)
            self.out[key] = self.out.get(key, 0.0) + time.perf_counter() - self.t0
