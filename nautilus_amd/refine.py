"""Match refinement on the GPU: every match record taken from its pose of the search lattice (one cell, one rotation step) to
the sub-cell pose at which the source scan's points lie on the target scan's lines -- a few Gauss-Newton updates on
point-to-line residuals, one workgroup per pair, one launch for the list.

Build-defined (nhip_refine_start_poses / nhip_refine_icp_dev / nhip_refine_icp, kernel unit K22).  The rule -- every operation
and the order of every sum, so that a numpy restatement pins the device bit for bit -- is DESIGN.md section 3, "Match
refinement"; hostside.refine_icp is the same rule in vectorised numpy.  Torch tensors are only the allocator, as in freespace.py.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import RefineSpec, check, ptr
from .hostside import REFINED_DTYPE, refine_thresholds

SKIPPED, TARGET_TOO_LONG, FEW, SINGULAR, RUNAWAY, NOT_CONVERGED = 1, 2, 4, 8, 16, 32
KIND_SCAN_ID = 4194304  # nhip_dev_status: a pair's source or target scan id was out of range
TRACE_SHAPE = (_lib.NHIP_REFINE_THRESHOLDS, 4)


def default_spec():
    """nhip_refine_spec_default (works without a device)."""
    s = RefineSpec()
    check(_lib.load().nhip_refine_spec_default(C.byref(s)))
    return s


def spec(**overrides):
    """The defaults with the named fields replaced; the threshold table is filled again from thr0, shrink and thr_min unless
    `thr` (16 values) is given itself."""
    s = default_spec()
    for k, v in overrides.items():
        if k not in dict(RefineSpec._fields_):
            raise TypeError("refine.spec: no field %r" % k)
        if k != "thr":
            setattr(s, k, v)
    thr = overrides["thr"] if "thr" in overrides else refine_thresholds(s.thr0, s.shrink, s.thr_min)
    if len(thr) != _lib.NHIP_REFINE_THRESHOLDS:
        raise ValueError("refine.spec: thr takes %d values" % _lib.NHIP_REFINE_THRESHOLDS)
    for k in range(_lib.NHIP_REFINE_THRESHOLDS):
        s.thr[k] = float(thr[k])
    return s


def start_poses(records, theta0, grid_spec, search, pair_origin=None):
    """nhip_refine_start_poses (works without a device): (n, 4) float64 (cos, sin, tx, ty) of the records' lattice poses; four
    NaNs for a rejected record."""
    from .csm import MATCH_DTYPE
    m = np.ascontiguousarray(records, dtype=MATCH_DTYPE)
    n = m.size
    theta0 = np.ascontiguousarray(theta0, dtype=np.float64)
    if theta0.size != n:
        raise ValueError("start_poses: one theta0 per record")
    org = None if pair_origin is None else np.ascontiguousarray(pair_origin, dtype=np.int32).reshape(n, 2)
    out = np.zeros((n, 4), dtype=np.float64)
    check(_lib.load().nhip_refine_start_poses(ptr(m), ptr(theta0), ptr(org), n, C.byref(grid_spec), C.byref(search), ptr(out)))
    return out


def icp(xy, normals, offsets, pair_src, pair_tgt, pose0, spec=None, trace=False):
    """The host form (nhip_refine_icp) on packed scans (xy and normals float32 (n, 2), offsets), scan ids per pair and start
    poses (n, 4): the refined records (REFINED_DTYPE), and with trace=True also the poses after every update, float64
    (n, 16, 4), zeros behind the last one."""
    xy = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
    normals = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 2)
    off = np.ascontiguousarray(offsets, dtype=np.int32)
    pair_src = np.ascontiguousarray(pair_src, dtype=np.int32).reshape(-1)
    pair_tgt = np.ascontiguousarray(pair_tgt, dtype=np.int32).reshape(-1)
    n = pair_src.size
    pose0 = np.ascontiguousarray(pose0, dtype=np.float64).reshape(n, 4)
    if pair_tgt.size != n or len(normals) != len(xy):
        raise ValueError("refine.icp: array lengths differ")
    spec = default_spec() if spec is None else spec
    out = np.zeros(n, dtype=REFINED_DTYPE)
    tr = np.zeros((n,) + TRACE_SHAPE, dtype=np.float64) if trace else None
    check(_lib.load().nhip_refine_icp(ptr(xy), ptr(normals), ptr(off), len(off) - 1, ptr(pair_src), ptr(pair_tgt), ptr(pose0), n,
                                      C.byref(spec), ptr(out), ptr(tr)))
    return (out, tr) if trace else out


def icp_on_device(d_xy, d_normals, d_off, n_scans, d_src, d_tgt, d_pose0, n_pairs, spec=None, trace=False):
    """nhip_refine_icp_dev on device tensors (float32 xy and normals, int32 offsets and scan ids, float64 start poses): the
    records as a uint8 tensor (n_pairs, 104) -- records_from() turns its host copy into REFINED_DTYPE -- and with trace=True
    the float64 tensor (n_pairs, 16, 4), on torch's current stream.  nhip_dev_status is the caller's to check."""
    import torch
    lib, dev = _lib.load(), d_xy.device
    spec = default_spec() if spec is None else spec
    n = int(n_pairs)
    d_out = torch.empty((max(n, 1), REFINED_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    d_trace = torch.empty((max(n, 1),) + TRACE_SHAPE, dtype=torch.float64, device=dev) if trace else None
    sp = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    check(lib.nhip_refine_icp_dev(d_xy.data_ptr(), d_normals.data_ptr(), d_off.data_ptr(), int(n_scans), d_src.data_ptr(),
                                  d_tgt.data_ptr(), d_pose0.data_ptr(), n, C.byref(spec), d_out.data_ptr(),
                                  None if d_trace is None else d_trace.data_ptr(), sp))
    return (d_out[:n], d_trace[:n]) if trace else d_out[:n]


def records_from(d_out):
    """The host copy of icp_on_device's uint8 tensor as REFINED_DTYPE records."""
    return np.ascontiguousarray(d_out.cpu().numpy()).view(REFINED_DTYPE).reshape(-1)


def to_transform(refined):
    """nhip_refined_to_transform per record (works without a device): (n, 3) float64 (tx, ty, theta = atan2(s, c))."""
    r = np.ascontiguousarray(refined, dtype=REFINED_DTYPE).reshape(-1)
    lib, out = _lib.load(), np.zeros((r.size, 3))
    tx, ty, th = C.c_double(), C.c_double(), C.c_double()
    for i in range(r.size):
        check(lib.nhip_refined_to_transform(C.cast(r[i:i + 1].ctypes.data, C.POINTER(_lib.Refined)), C.byref(tx), C.byref(ty), C.byref(th)))
        out[i] = (tx.value, ty.value, th.value)
    return out
