"""Loop-closure candidates by appearance on the GPU: every scan as a ring descriptor -- R rings x 64 sectors of the scan
frame, one bit per bin that holds a return -- and the K nearest scans of each query of a list under the best of the 64
rotations, by Hamming distance.  No pose enters: this is what proposes pairs when drift has left the geometric gate's 3.5 m
and the matcher's window, and the rotation that aligns two descriptors is the matcher's theta0.

Build-defined (nhip_place_describe_dev / nhip_place_match_dev / nhip_place_candidates, kernel unit K16), in the place of the
reference's learned embedding behind a service (lc_match_threshold, solver.cc:58-60).  The spec -- two float comparisons per
point, integers after them, so a numpy restatement pins it bit for bit -- is DESIGN.md section 3, "Place descriptors".  Torch
tensors are only the allocator, as in freespace.py.

Place sequences (nhip_place_seq_*, kernel unit K16b; DESIGN.md section 3, "Place sequences") take the same distances over a
window of 2W + 1 frames around both scans of a pair, in both directions of travel: what averages out the disturbance of a
single scan.  The reference's window of five frames (lc_match_window_size, default_config.lua:138-139) is W = 2.
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import NHIP_PLACE_PAST_ONLY, PlaceSeqSpec, PlaceSpec, check, ptr

SECTORS = 64
RECORD_FIELDS = ("j", "shift", "dist", "bits_j")
SEQ_RECORD_FIELDS = RECORD_FIELDS + ("seq", "sum", "frames", "direction")
SEQ_STATS_FIELDS = ("n_ids", "admissible", "gated", "records", "queries_without_record", "scans_without_bits", "reverse", "short")
STATS_FIELDS = ("n_ids", "admissible", "gated", "records", "queries_without_record", "scans_without_bits", "reserved0", "reserved1")


def default_spec():
    """nhip_place_spec_default (works without a device)."""
    s = PlaceSpec()
    check(_lib.load().nhip_place_spec_default(C.byref(s)))
    return s


def spec(**overrides):
    """The defaults with the named fields replaced."""
    s = default_spec()
    for k, v in overrides.items():
        if k not in dict(PlaceSpec._fields_):
            raise TypeError("place.spec: no field %r" % k)
        setattr(s, k, v)
    return s


def tables(spec=None):
    """nhip_place_tables (works without a device): (edge2 float32 (R + 1,), dir float32 (32, 2))."""
    spec = default_spec() if spec is None else spec
    edge2, dirs = np.zeros(max(int(spec.n_rings), 0) + 1, np.float32), np.zeros((32, 2), np.float32)
    check(_lib.load().nhip_place_tables(C.byref(spec), ptr(edge2), ptr(dirs)))
    return edge2, dirs


def workspace_bytes(spec, n_ids):
    """nhip_place_workspace_bytes (works without a device)."""
    n = _lib.load().nhip_place_workspace_bytes(C.byref(spec), int(n_ids))
    if n < 0:
        check(_lib.NHIP_ERR_ARG)
    return n


def describe_on_device(d_xy, d_off, n_scans, spec=None):
    """nhip_place_describe_dev on device tensors (float32 xy, int32 offsets): (descriptors int64 (n_scans, R) -- the uint64
    words, bit for bit -- and bits int32 (n_scans,)), on torch's current stream."""
    import torch
    lib, dev = _lib.load(), d_xy.device
    spec = default_spec() if spec is None else spec
    d_desc = torch.empty((max(int(n_scans), 1), max(int(spec.n_rings), 1)), dtype=torch.int64, device=dev)
    d_bits = torch.empty(max(int(n_scans), 1), dtype=torch.int32, device=dev)
    sp = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    check(lib.nhip_place_describe_dev(d_xy.data_ptr(), d_off.data_ptr(), int(n_scans), C.byref(spec), d_desc.data_ptr(),
                                      d_bits.data_ptr(), sp))
    return d_desc[:int(n_scans)], d_bits[:int(n_scans)]


def match_on_device(d_desc, d_bits, n_scans, d_ids, n_ids, spec=None, workspace=None):
    """nhip_place_match_dev on device tensors (the descriptors of describe_on_device, int32 ids, ascending): (records int32
    (n_ids, K, 4), stats int64 (8,)), on torch's current stream.  workspace: bytes of the key workspace (None:
    nhip_place_workspace_bytes; smaller: more chunks of query rows, the same records).  nhip_dev_status is the caller's to
    check."""
    import torch
    lib, dev = _lib.load(), d_desc.device
    spec = default_spec() if spec is None else spec
    n_ids = int(n_ids)
    ws = workspace_bytes(spec, n_ids) if workspace is None else int(workspace)
    d_ws = torch.empty(max(ws, 2) // 2, dtype=torch.int16, device=dev)
    d_rec = torch.empty((max(n_ids, 1), int(spec.top_k), 4), dtype=torch.int32, device=dev)
    d_stats = torch.empty(8, dtype=torch.int64, device=dev)
    sp = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    check(lib.nhip_place_match_dev(d_desc.data_ptr(), d_bits.data_ptr(), int(n_scans), d_ids.data_ptr(), n_ids, C.byref(spec),
                                   d_rec.data_ptr(), d_stats.data_ptr(), d_ws.data_ptr(), ws, sp))
    return d_rec[:n_ids], d_stats


def candidates(scans, ids, spec=None, descriptors=False):
    """The handle form (nhip_place_candidates) on a csm.ScanTable: ids, strictly ascending scan ids (anything else raises
    NhipError before a launch); (records int32 (n_ids, K, 4): RECORD_FIELDS, four -1 where unfilled; stats int64 (8,):
    STATS_FIELDS), with descriptors=True also (descriptors uint64 (n_scans, R), bits int32 (n_scans,))."""
    spec = default_spec() if spec is None else spec
    ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
    rec = np.full((len(ids), max(int(spec.top_k), 0), 4), -1, dtype=np.int32)
    stats = np.zeros(8, dtype=np.int64)
    desc = np.zeros((scans.n_scans, max(int(spec.n_rings), 0)), dtype=np.uint64) if descriptors else None
    bits = np.zeros(scans.n_scans, dtype=np.int32) if descriptors else None
    check(_lib.load().nhip_place_candidates(scans._h, ptr(ids), len(ids), C.byref(spec), ptr(rec), ptr(stats), ptr(desc), ptr(bits)))
    return (rec, stats, desc, bits) if descriptors else (rec, stats)


def default_seq_spec():
    """nhip_place_seq_spec_default (works without a device)."""
    s = PlaceSeqSpec()
    check(_lib.load().nhip_place_seq_spec_default(C.byref(s)))
    return s


def seq_spec(**overrides):
    """The sequence defaults with the named fields replaced."""
    s = default_seq_spec()
    for k, v in overrides.items():
        if k not in dict(PlaceSeqSpec._fields_):
            raise TypeError("place.seq_spec: no field %r" % k)
        setattr(s, k, v)
    return s


def seq_workspace_bytes(spec, seq, n_scans, n_ids):
    """nhip_place_seq_workspace_bytes (works without a device)."""
    n = _lib.load().nhip_place_seq_workspace_bytes(C.byref(spec), C.byref(seq), int(n_scans), int(n_ids))
    if n < 0:
        check(_lib.NHIP_ERR_ARG)
    return n


def sequence_match_on_device(d_desc, d_bits, n_scans, d_ids, n_ids, spec, seq=None, workspace=None):
    """nhip_place_seq_match_dev on device tensors (the descriptors of ALL n_scans scans, int32 ids, ascending): (records int32
    (n_ids, K, 8), stats int64 (8,)), on torch's current stream.  workspace: bytes of the workspace (None:
    nhip_place_seq_workspace_bytes; smaller: more chunks of query scans, the same records).  nhip_dev_status is the caller's to
    check."""
    import torch
    lib, dev = _lib.load(), d_desc.device
    seq = default_seq_spec() if seq is None else seq
    n_ids = int(n_ids)
    ws = seq_workspace_bytes(spec, seq, n_scans, n_ids) if workspace is None else int(workspace)
    d_ws = torch.empty(max(ws, 2) // 2, dtype=torch.int16, device=dev)
    d_rec = torch.empty((max(n_ids, 1), int(spec.top_k), 8), dtype=torch.int32, device=dev)
    d_stats = torch.empty(8, dtype=torch.int64, device=dev)
    sp = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    check(lib.nhip_place_seq_match_dev(d_desc.data_ptr(), d_bits.data_ptr(), int(n_scans), d_ids.data_ptr(), n_ids, C.byref(spec),
                                       C.byref(seq), d_rec.data_ptr(), d_stats.data_ptr(), d_ws.data_ptr(), ws, sp))
    return d_rec[:n_ids], d_stats


def sequence_candidates(scans, ids, spec, seq=None):
    """The handle form (nhip_place_seq_candidates) on a csm.ScanTable that holds every scan a window reaches: ids, strictly
    ascending scan ids (anything else raises NhipError before a launch); (records int32 (n_ids, K, 8): SEQ_RECORD_FIELDS, eight
    -1 where unfilled; stats int64 (8,): SEQ_STATS_FIELDS)."""
    seq = default_seq_spec() if seq is None else seq
    ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
    rec = np.full((len(ids), max(int(spec.top_k), 0), 8), -1, dtype=np.int32)
    stats = np.zeros(8, dtype=np.int64)
    check(_lib.load().nhip_place_seq_candidates(scans._h, ptr(ids), len(ids), C.byref(spec), C.byref(seq), ptr(rec), ptr(stats)))
    return rec, stats


def theta0(records):
    """The heading of each record's query relative to its candidate, AngleMod(-shift 2 pi / 64): the matcher's theta0 for the
    pair (src = query, tgt = j).  float64, the records' shape without the last axis; nan for an unfilled record."""
    shift = np.asarray(records, dtype=np.int64)[..., 1]
    w = 2.0 * math.pi / SECTORS
    return np.where(shift < 0, np.nan, np.where(shift <= 32, -shift * w, (SECTORS - shift) * w))


def pairs(ids, records):
    """(pair_src int32, pair_tgt int32, theta0 float64) of all filled records, query by query in the records' order.  Records
    of four fields (candidates) or eight (sequence_candidates): fields 0 and 1 are read."""
    rec = np.asarray(records, dtype=np.int32)
    ids = np.asarray(ids, dtype=np.int32).reshape(-1)
    if rec.ndim != 3 or rec.shape[0] != len(ids) or rec.shape[2] not in (4, 8):
        raise ValueError("place.pairs: records of shape %s for %d ids" % (rec.shape, len(ids)))
    filled = rec[:, :, 0] >= 0
    src = np.broadcast_to(ids[:, None], filled.shape)[filled]
    return src.astype(np.int32), rec[:, :, 0][filled].astype(np.int32), theta0(rec)[filled]
