"""Planar and edge scan features on the GPU: what Solver::SolveSLAM's FEATURE mode builds its blocks from.

  FeatureExtractor(pointcloud, 0.008, 2.0, 10, 10, 20, 10)   src/util/slam_types.h:66-69, src/input/feature_extracter.cc
    -> nhip_features_extract_dev   (scores + the two greedy selections of every scan, one launch)
    -> nhip_features_pack_dev      (the selected points and their own normals as packed clouds: what IcpBatch takes)
The spec is DESIGN.md section 3, "Scan features".  Torch tensors are only the allocator, as in correspondence.py.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import FeatureSpec, check


def default_spec():
    """The reference's constants (nhip_feature_spec_default; works without a device)."""
    s = FeatureSpec()
    check(_lib.load().nhip_feature_spec_default(C.byref(s)))
    return s


def feature_spec(**kw):
    """The defaults with the named fields replaced."""
    s = default_spec()
    for k, v in kw.items():
        if k not in dict(FeatureSpec._fields_):
            raise TypeError("feature_spec: no field %r" % k)
        setattr(s, k, v)
    return s


class Features:
    """Host copies of one extraction: planar_idx (n_scans, max_planar) and edge_idx (n_scans, max_edge), scan-local indices
    in acceptance order, -1 padded; planar_count, edge_count (n_scans,); scores (n_points,) float64 with NaN = no score, or
    None.  The device copies stay alive for clouds()."""

    def __init__(self, spec, device, d_pidx, d_pcnt, d_eidx, d_ecnt, d_scores, n_scans):
        self.spec, self.device, self.n_scans = spec, device, n_scans
        self._d = (d_pidx, d_pcnt, d_eidx, d_ecnt)
        self.planar_idx = d_pidx.cpu().numpy().reshape(n_scans, spec.max_planar)
        self.planar_count = d_pcnt.cpu().numpy()[:n_scans]
        self.edge_idx = d_eidx.cpu().numpy().reshape(n_scans, spec.max_edge)
        self.edge_count = d_ecnt.cpu().numpy()[:n_scans]
        self.scores = None if d_scores is None else d_scores.cpu().numpy()

    def clouds(self, xy, normals, offsets):
        """((xy_p, nrm_p, off_p), (xy_e, nrm_e, off_e)): the planar and the edge points of every scan with their own normals,
        packed (nhip_features_pack_dev).  normals None: nrm_* are None."""
        import torch
        dev = torch.device(self.device)
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
        f = lambda a: t(np.reshape(a, (-1, 2)), np.float32) if np.size(a) else torch.zeros(2, dtype=torch.float32, device=dev)
        d_xy, d_off = f(xy), t(offsets, np.int32)  # (no points at all: still an address, the entry point refuses NULL)
        d_nrm = None if normals is None else f(normals)
        d_pidx, d_pcnt, d_eidx, d_ecnt = self._d
        return (pack(d_xy, d_nrm, d_off, self.n_scans, d_pidx, d_pcnt, self.spec.max_planar),
                pack(d_xy, d_nrm, d_off, self.n_scans, d_eidx, d_ecnt, self.spec.max_edge))


def pack(d_xy, d_normals, d_offsets, n_scans, d_idx, d_count, cap):
    """nhip_features_pack_dev on device tensors; returns host arrays (xy (m, 2), normals (m, 2) or None, offsets (n_scans + 1)).
    An index or count that does not fit its scan raises NhipError (nhip_dev_status); the offender is left out."""
    import torch
    lib, dev = _lib.load(), d_xy.device
    e = lambda n, dt: torch.empty(max(int(n), 1), dtype=dt, device=dev)
    d_xo, d_oo = e(2 * n_scans * cap, torch.float32), e(n_scans + 1, torch.int32)
    d_no = None if d_normals is None else e(2 * n_scans * cap, torch.float32)
    sp = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    check(lib.nhip_features_pack_dev(d_xy.data_ptr(), None if d_normals is None else d_normals.data_ptr(), d_offsets.data_ptr(),
                                     n_scans, d_idx.data_ptr(), d_count.data_ptr(), cap, d_xo.data_ptr(),
                                     None if d_no is None else d_no.data_ptr(), d_oo.data_ptr(), sp))
    check(lib.nhip_dev_status(sp, None))
    off = d_oo.cpu().numpy()[:n_scans + 1].copy()
    m = int(off[-1])
    xy = d_xo[:2 * m].cpu().numpy().reshape(m, 2).copy()
    nrm = None if d_no is None else d_no[:2 * m].cpu().numpy().reshape(m, 2).copy()
    return xy, nrm, off


def extract(xy, offsets, spec=None, device="cuda:0", want_scores=False):
    """The features of every scan of (xy, offsets) -> Features."""
    import torch
    spec = default_spec() if spec is None else spec
    lib, dev = _lib.load(), torch.device(device)
    offsets = np.ascontiguousarray(offsets, dtype=np.int32)
    xy = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
    n = len(offsets) - 1
    if len(xy) != int(offsets[-1]):
        raise ValueError("features.extract: offsets[-1] = %d, but %d points" % (int(offsets[-1]), len(xy)))
    t = lambda a: torch.from_numpy(a).to(dev)
    e = lambda k, dt: torch.empty(max(int(k), 1), dtype=dt, device=dev)
    d_xy, d_off = (t(xy) if len(xy) else e(2, torch.float32)), t(offsets)
    d_pidx, d_pcnt = e(n * spec.max_planar, torch.int32), e(n, torch.int32)
    d_eidx, d_ecnt = e(n * spec.max_edge, torch.int32), e(n, torch.int32)
    d_sc = torch.empty(len(xy), dtype=torch.float64, device=dev) if want_scores else None
    sp = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    check(lib.nhip_features_extract_dev(d_xy.data_ptr(), d_off.data_ptr(), n, C.byref(spec), d_pidx.data_ptr(), d_pcnt.data_ptr(),
                                        d_eidx.data_ptr(), d_ecnt.data_ptr(), None if d_sc is None else d_sc.data_ptr(), sp))
    return Features(spec, str(dev), d_pidx[:n * spec.max_planar], d_pcnt, d_eidx[:n * spec.max_edge], d_ecnt, d_sc, n)


def extract_on_handle(scans, spec=None, want_scores=False):
    """The handle form (nhip_features_extract) on a csm.ScanTable: (planar_idx, planar_count, edge_idx, edge_count, scores)."""
    spec = default_spec() if spec is None else spec
    n = scans.n_scans
    pidx, pcnt = np.empty((n, spec.max_planar), np.int32), np.empty(n, np.int32)
    eidx, ecnt = np.empty((n, spec.max_edge), np.int32), np.empty(n, np.int32)
    sc = np.empty(len(scans.xy)) if want_scores else None
    check(_lib.load().nhip_features_extract(scans._h, C.byref(spec), _lib.ptr(pidx), _lib.ptr(pcnt), _lib.ptr(eidx), _lib.ptr(ecnt),
                                            _lib.ptr(sc)))
    return pidx, pcnt, eidx, ecnt, sc
