"""The free-space check of match records on the GPU: where a source scan's returns land under a matched pose -- near a hit
of the target, in space the target's beams crossed, or where the target saw nothing -- and how many of the source's own
beams run through a target hit.  A score cannot tell a contradiction from a partial overlap; these counts can.

Build-defined (nhip_freespace_trace_dev / nhip_freespace_check_dev / nhip_csm_freespace, kernel unit K15).  The spec -- the
occupancy grid's ray on the matcher's cells, all integer after the cells, so a numpy restatement pins it bit for bit -- is
DESIGN.md section 3, "Free-space check".  Torch tensors are only the allocator, as in occupancy.py.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import FreespaceSpec, check, ptr

COUNT_FIELDS = ("n_points", "dropped", "outside", "hit", "free", "unknown", "through", "reserved")
# The gate's default: a pair is kept iff free + through <= 200 permille of hit + free + unknown.  Measured on SynthBag(320)
# ("Free-space check", item 6): the largest share at a right pose is 0.084, the smallest at a wrong one
# 0.448; matches within 0.05 m of the truth reach 0.116, wrong interior optima start at 0.181.
DEFAULT_MAX_PERMILLE = 200


def default_spec():
    """nhip_freespace_spec_default (works without a device)."""
    s = FreespaceSpec()
    check(_lib.load().nhip_freespace_spec_default(C.byref(s)))
    return s


def spec(**overrides):
    """The defaults with the named fields replaced."""
    s = default_spec()
    for k, v in overrides.items():
        if k not in dict(FreespaceSpec._fields_):
            raise TypeError("freespace.spec: no field %r" % k)
        setattr(s, k, v)
    return s


def planes_bytes(grid_spec, n_slots):
    """nhip_freespace_planes_bytes: bytes of the free planes of n_slots slots (works without a device)."""
    n = _lib.load().nhip_freespace_planes_bytes(C.byref(grid_spec), int(n_slots))
    if n < 0:
        check(_lib.NHIP_ERR_ARG)
    return n


def keep(counts, max_permille=DEFAULT_MAX_PERMILLE):
    """The gate, host-side and in integers: pair i is kept iff 1000 (free + through) <= max_permille (hit + free + unknown).
    The record of a rejected match (eight -1) is not kept; a pair without a point inside the grid is (nothing contradicts it)."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1, 8)
    max_permille = int(max_permille)
    if not 0 <= max_permille <= 1000:
        raise ValueError("freespace.keep: max_permille %d outside 0..1000" % max_permille)
    return (c[:, 0] >= 0) & (1000 * (c[:, 4] + c[:, 6]) <= max_permille * (c[:, 3] + c[:, 4] + c[:, 5]))


def violation_share(counts):
    """(free + through) / (hit + free + unknown) per pair as float64; 0 where the denominator is 0, nan for a rejected record."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1, 8)
    den = c[:, 3] + c[:, 4] + c[:, 5]
    out = np.where(den > 0, (c[:, 4] + c[:, 6]) / np.maximum(den, 1), 0.0)
    return np.where(c[:, 0] < 0, np.nan, out)


def trace_on_device(d_xy, d_off, n_scans, d_target_ids, n_targets, grid_spec, d_grids):
    """nhip_freespace_trace_dev on device tensors (float32 xy, int32 offsets and target ids, the uint8 slots
    nhip_grid_build_dev filled): the free planes as a uint8 tensor of n_targets x hits_bytes, on torch's current stream."""
    import torch
    lib, dev = _lib.load(), d_grids.device
    d_free = torch.empty(max(planes_bytes(grid_spec, n_targets), 16), dtype=torch.uint8, device=dev)
    sp = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    check(lib.nhip_freespace_trace_dev(d_xy.data_ptr(), d_off.data_ptr(), int(n_scans), d_target_ids.data_ptr(), int(n_targets),
                                       C.byref(grid_spec), d_grids.data_ptr(), d_free.data_ptr(), sp))
    return d_free


def check_on_device(d_xy, d_off, n_scans, d_grids, n_grids, grid_spec, d_src, d_slot, d_rot0, d_delta, d_origin, n_pairs, search,
                    d_free, d_matches, fs_spec=None):
    """nhip_freespace_check_dev on device tensors, the matcher's own (d_origin may be None; d_matches: the records as the
    matcher left them): the counts as an int32 tensor (n_pairs, 8), on torch's current stream.  nhip_dev_status is the
    caller's to check."""
    import torch
    lib, dev = _lib.load(), d_grids.device
    fs_spec = default_spec() if fs_spec is None else fs_spec
    d_counts = torch.empty((max(int(n_pairs), 1), 8), dtype=torch.int32, device=dev)
    sp = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    check(lib.nhip_freespace_check_dev(d_xy.data_ptr(), d_off.data_ptr(), int(n_scans), d_grids.data_ptr(), int(n_grids),
                                       C.byref(grid_spec), d_src.data_ptr(), d_slot.data_ptr(), d_rot0.data_ptr(), d_delta.data_ptr(),
                                       None if d_origin is None else d_origin.data_ptr(), int(n_pairs), C.byref(search),
                                       d_free.data_ptr(), d_matches.data_ptr(), C.byref(fs_spec), d_counts.data_ptr(), sp))
    return d_counts[:int(n_pairs)]


def plane_cells(raw, layout):
    """One slot's free plane (hits_bytes uint8, as trace_on_device lays it out) as (side, side) uint8 of 0 / 1."""
    L = layout
    rows = np.asarray(raw, dtype=np.uint8)[:L.hits_pitch * (L.side + 64)].reshape(L.side + 64, L.hits_pitch)
    return np.unpackbits(rows, axis=1, bitorder="little")[32:32 + L.side, 32:32 + L.side]


def check_pairs(scans, grids, pair_src, pair_slot, theta0, search, matches, pair_origin=None, fs_spec=None):
    """The handle form (nhip_csm_freespace) on a csm.ScanTable and the csm.LikelihoodGrids built from it: the arguments of
    csm.match_pairs plus the records it returned; counts int32 (n, 8): COUNT_FIELDS.  The first call on `grids` traces its
    free planes, which stay with the handle.  Grids from LikelihoodGrids.from_submaps are refused (NhipError, NHIP_ERR_STATE)."""
    from .csm import MATCH_DTYPE
    pair_src = np.ascontiguousarray(pair_src, dtype=np.int32)
    pair_slot = np.ascontiguousarray(pair_slot, dtype=np.int32)
    theta0 = np.ascontiguousarray(theta0, dtype=np.float64)
    m = np.ascontiguousarray(matches, dtype=MATCH_DTYPE)
    n = pair_src.size
    if pair_slot.size != n or theta0.size != n or m.size != n:
        raise ValueError("pair arrays differ in length")
    org = None if pair_origin is None else np.ascontiguousarray(pair_origin, dtype=np.int32).reshape(n, 2)
    fs_spec = default_spec() if fs_spec is None else fs_spec
    counts = np.zeros((n, 8), dtype=np.int32)
    check(_lib.load().nhip_csm_freespace(scans._h, grids._h, ptr(pair_src), ptr(pair_slot), ptr(theta0), ptr(org), n,
                                         C.byref(search), ptr(m), C.byref(fs_spec), ptr(counts)))
    return counts
