"""Global localisation by range signatures: "here is a scan and NO pose, where in this map am I?"

Every free lattice cell of a finished occupancy grid (an anchor) gets 64 bytes -- the quantised distance to the nearest wall in
each of 64 sectors, ray-cast in the grid -- and every scan the same 64 bytes from its own returns.  A scan is placed at an
anchor under the best of the 64 rotations by the sum of absolute differences of the bytes over the sectors the scan has a
return in; the K best anchors per scan, neighbours suppressed, are the priors localize.localize then refines (relocalize.py).

Build-defined (nhip_rangesig_*, kernel unit K21); the reference has no counterpart.  The spec -- integer after the float
comparisons of a scan's points, so that a per-ray restatement pins it bit for bit -- is DESIGN.md section 3, "Range
signatures"; hostside.range_signatures / scan_signatures / signature_candidates restate it in numpy for any backend.  Torch
tensors are only the allocator, as in localize.py.
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import NHIP_RANGESIG_UNKNOWN_STOPS, RangesigSpec, check, ptr

SECTORS = 64
RECORD_FIELDS = ("anchor", "shift", "cost", "valid")
STATS_FIELDS = ("lattice_nodes", "anchors", "anchors_left_out", "rays_wall", "rays_unknown", "rays_outside", "queries_without_record",
                "records")
KIND_ANCHORS = 2097152  # nhip_dev_status: the anchors did not fit / an entry of the ray table is not a ray
MAX_ANCHORS = 1 << 20


def default_spec():
    """nhip_rangesig_spec_default (works without a device); the map's window is the caller's to set (spec)."""
    s = RangesigSpec()
    check(_lib.load().nhip_rangesig_spec_default(C.byref(s)))
    return s


def spec(occ_spec=None, **overrides):
    """The defaults on the window and res of occ_spec (an occupancy spec, or anything with res and the window), with the named
    fields replaced."""
    s = default_spec()
    if occ_spec is not None:
        s.res, s.cell_x0, s.cell_y0, s.width, s.height = float(occ_spec.res), occ_spec.cell_x0, occ_spec.cell_y0, occ_spec.width, occ_spec.height
    for k, v in overrides.items():
        if k not in dict(RangesigSpec._fields_):
            raise TypeError("rangesig.spec: no field %r" % k)
        setattr(s, k, v)
    return s


def tables(spec):
    """nhip_rangesig_tables (works without a device): (rays int32 (64 m, 4) = {dx, dy, n, scale}, edge2 float32 (255,))."""
    m = int(spec.rays_per_sector)
    rays, edge2 = np.zeros((SECTORS * (m if m in (1, 2, 4, 8) else 1), 4), np.int32), np.zeros(255, np.float32)
    check(_lib.load().nhip_rangesig_tables(C.byref(spec), ptr(rays), ptr(edge2)))
    return rays, edge2


def workspace_bytes(spec, n_anchors, n_queries):
    """nhip_rangesig_workspace_bytes (works without a device)."""
    n = _lib.load().nhip_rangesig_workspace_bytes(C.byref(spec), int(n_anchors), int(n_queries))
    if n < 0:
        check(_lib.NHIP_ERR_ARG)
    return n


def _stream(torch, dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _grid_tensor(torch, dev, grid, spec):
    if isinstance(grid, torch.Tensor):
        if grid.dtype != torch.int8 or tuple(grid.shape) != (spec.height, spec.width) or not grid.is_contiguous() or grid.device != dev:
            raise ValueError("rangesig: the grid must be a contiguous int8 (%d, %d) tensor on %s" % (spec.height, spec.width, dev))
        return grid
    g = np.ascontiguousarray(grid, dtype=np.int8)
    if g.shape != (spec.height, spec.width):
        raise ValueError("rangesig: grid of shape %s for a window of %d x %d" % (g.shape, spec.height, spec.width))
    return torch.from_numpy(g).to(dev)


def anchors_on_device(d_grid, spec, max_anchors=None, d_stats=None):
    """nhip_rangesig_anchors_dev on a device grid (int8 (H, W) tensor), enqueued on torch's current stream: (d_anchors int32
    (max(max_anchors, 1), 4), d_stats int64 (8,), max_anchors).  Entries behind the anchors found are four -1.
    max_anchors=None: counted from the grid (one reduction on the device, which waits for it), at most 2^20."""
    import torch
    dev, lib = d_grid.device, _lib.load()
    if max_anchors is None:
        h, st = int(spec.stride) // 2, max(int(spec.stride), 1)
        nodes = d_grid[h::st, h::st]
        max_anchors = min(int(((nodes >= 0) & (nodes <= int(spec.free_max))).sum().item()), MAX_ANCHORS)
    d_anchors = torch.empty((max(int(max_anchors), 1), 4), dtype=torch.int32, device=dev)
    d_stats = torch.empty(8, dtype=torch.int64, device=dev) if d_stats is None else d_stats
    ws = workspace_bytes(spec, 0, 0)
    d_ws = torch.empty(ws, dtype=torch.uint8, device=dev)
    check(lib.nhip_rangesig_anchors_dev(d_grid.data_ptr(), C.byref(spec), int(max_anchors), d_anchors.data_ptr(), d_stats.data_ptr(),
                                        d_ws.data_ptr(), ws, _stream(torch, dev)))
    return d_anchors, d_stats, int(max_anchors)


def map_signatures_on_device(d_grid, spec, d_anchors, n_anchors, d_stats, d_rays=None):
    """nhip_rangesig_map_dev on device tensors, on torch's current stream: d_sig uint8 (max(n_anchors, 1), 64).  d_rays: the ray
    table on the device, int32 (64 m, 4) (None: tables(spec), uploaded)."""
    import torch
    dev = d_grid.device
    if d_rays is None:
        d_rays = torch.from_numpy(tables(spec)[0]).to(dev)
    d_sig = torch.empty((max(int(n_anchors), 1), SECTORS), dtype=torch.uint8, device=dev)
    check(_lib.load().nhip_rangesig_map_dev(d_grid.data_ptr(), C.byref(spec), d_rays.data_ptr(), d_anchors.data_ptr(), int(n_anchors),
                                            d_sig.data_ptr(), d_stats.data_ptr(), _stream(torch, dev)))
    return d_sig


def scan_signatures_on_device(d_xy, d_off, n_scans, spec):
    """nhip_rangesig_scans_dev on device tensors (float32 xy, int32 offsets), on torch's current stream: d_sig uint8
    (max(n_scans, 1), 64)."""
    import torch
    dev = d_off.device
    d_sig = torch.empty((max(int(n_scans), 1), SECTORS), dtype=torch.uint8, device=dev)
    check(_lib.load().nhip_rangesig_scans_dev(d_xy.data_ptr(), d_off.data_ptr(), int(n_scans), C.byref(spec), d_sig.data_ptr(),
                                              _stream(torch, dev)))
    return d_sig


def match_on_device(d_query_sig, n_queries, d_map_sig, d_anchors, n_anchors, spec, d_stats=None, workspace=None):
    """nhip_rangesig_match_dev on device tensors (two arrays of signature bytes, the anchor list), on torch's current stream:
    (d_records int32 (n_queries, K, 4), d_stats int64 (8,)).  workspace: bytes of the key workspace (None:
    nhip_rangesig_workspace_bytes; smaller: more chunks of query rows, the same records).  nhip_dev_status is the caller's to
    check."""
    import torch
    dev, lib = d_map_sig.device, _lib.load()
    n_queries, n_anchors = int(n_queries), int(n_anchors)
    ws = workspace_bytes(spec, n_anchors, n_queries) if workspace is None else int(workspace)
    d_ws = torch.empty(max(ws, 4) // 4, dtype=torch.int32, device=dev)
    d_rec = torch.empty((max(n_queries, 1), int(spec.top_k), 4), dtype=torch.int32, device=dev)
    d_stats = torch.zeros(8, dtype=torch.int64, device=dev) if d_stats is None else d_stats
    check(lib.nhip_rangesig_match_dev(d_query_sig.data_ptr(), n_queries, d_map_sig.data_ptr(), d_anchors.data_ptr(), n_anchors,
                                      C.byref(spec), d_rec.data_ptr(), d_stats.data_ptr(), d_ws.data_ptr(), ws, _stream(torch, dev)))
    return d_rec[:n_queries], d_stats


def candidates_on_device(d_grid, spec, d_xy, d_off, n_scans, max_anchors=None):
    """The four calls in turn on device tensors: a dict of the device tensors anchors (A, 4), map_sig (A, 64), scan_sig (n, 64),
    records (n, K, 4), stats (8,) and the int n_anchors.  The only wait is the count behind max_anchors=None."""
    d_anchors, d_stats, n = anchors_on_device(d_grid, spec, max_anchors)
    d_map = map_signatures_on_device(d_grid, spec, d_anchors, n, d_stats)
    d_scan = scan_signatures_on_device(d_xy, d_off, n_scans, spec)
    d_rec, d_stats = match_on_device(d_scan, n_scans, d_map, d_anchors, n, spec, d_stats)
    return {"anchors": d_anchors[:n], "map_sig": d_map[:n], "scan_sig": d_scan[:int(n_scans)], "records": d_rec, "stats": d_stats,
            "n_anchors": n}


def candidates(grid, occ_spec, xy, offsets, device="cuda:0", max_anchors=None):
    """Proposals for the packed scans (xy, offsets) in `grid` (host array or device tensor; occ_spec: a RangesigSpec, or an
    occupancy spec whose window and res the defaults are put on), made on the GPU: a dict of the host arrays records int32 (n, K,
    4): RECORD_FIELDS, four -1 where unfilled; anchors int32 (A, 4) = {cx, cy, i, j}; map_sig uint8 (A, 64); scan_sig uint8
    (n, 64); stats int64 (8,): STATS_FIELDS -- hostside.range_signatures / scan_signatures / signature_candidates bit for bit.
    More anchors than max_anchors (None: all, at most 2^20) raises NhipError (kind 2097152)."""
    import torch
    dev = torch.device(device)
    s = occ_spec if isinstance(occ_spec, RangesigSpec) else spec(occ_spec)
    off = np.ascontiguousarray(offsets, dtype=np.int32)
    n = len(off) - 1
    p = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
    d_xy = torch.from_numpy(p).to(dev) if len(p) else torch.zeros((1, 2), dtype=torch.float32, device=dev)
    out = candidates_on_device(_grid_tensor(torch, dev, grid, s), s, d_xy, torch.from_numpy(off).to(dev), n, max_anchors)
    check(_lib.load().nhip_dev_status(_stream(torch, dev), None))
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in out.items()}


def candidates_host_form(grid, spec, xy, offsets, max_anchors):
    """The host form (nhip_rangesig_candidates): host grid, host scans, host outputs; the dict of candidates()."""
    g = np.ascontiguousarray(grid, dtype=np.int8).reshape(spec.height, spec.width)
    p = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
    off = np.ascontiguousarray(offsets, dtype=np.int32)
    n, cap = len(off) - 1, max(int(max_anchors), 0)
    rec = np.full((n, max(int(spec.top_k), 0), 4), -1, np.int32)
    anchors, n_anchors, stats = np.full((max(cap, 1), 4), -1, np.int32), np.zeros(1, np.int32), np.zeros(8, np.int64)
    map_sig, scan_sig = np.zeros((max(cap, 1), SECTORS), np.uint8), np.zeros((max(n, 1), SECTORS), np.uint8)
    check(_lib.load().nhip_rangesig_candidates(ptr(g), C.byref(spec), ptr(p) if len(p) else None, ptr(off), n, cap, ptr(rec), ptr(anchors),
                                               ptr(n_anchors), ptr(stats), ptr(map_sig), ptr(scan_sig)))
    a = int(n_anchors[0])
    return {"records": rec, "anchors": anchors[:a].copy(), "map_sig": map_sig[:a].copy(), "scan_sig": scan_sig[:n].copy(), "stats": stats,
            "n_anchors": a}


def priors(records, anchors, spec):
    """The poses the records propose (item 7 of the spec; host, double): float64, the records' shape with (x, y, heading) in the
    place of the four fields; x = (cell_x0 + cx + 0.5) res, y likewise, heading = angle_mod(shift 2 pi / 64) -- shift w for
    shift <= 32, else (shift - 64) w; NaN for an unfilled record."""
    rec = np.asarray(records, dtype=np.int64)
    an = np.asarray(anchors, dtype=np.int64).reshape(-1, 4)
    filled = rec[..., 0] >= 0
    a = np.where(filled, rec[..., 0], 0)
    shift = rec[..., 1]
    w, res = 2.0 * math.pi / SECTORS, float(spec.res)
    out = np.full(rec.shape[:-1] + (3,), np.nan)
    if len(an):
        out[..., 0] = (int(spec.cell_x0) + an[a, 0] + 0.5) * res
        out[..., 1] = (int(spec.cell_y0) + an[a, 1] + 0.5) * res
        out[..., 2] = np.where(shift <= 32, shift * w, (shift - SECTORS) * w)
    out[~filled] = np.nan
    return out
