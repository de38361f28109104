"""Scan normals on the GPU: the one input of the correspondence search, the normal residual and the feature clouds that a
real bag does not bring.

  NormalComputation::GetNormals(points)   src/input/normal_computation.{h,cc}, called from KDTree::EigenToKD (kdtree.cc:152-163)
    -> nhip_normals_estimate_dev          (the normals of every point of every scan, one call)
The spec -- the reference's randomised Hough estimate with a counter-based generator, and where it leaves the reference on
purpose -- is DESIGN.md section 3, "Scan normals".  Torch tensors are only the allocator, as in features.py.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import NormalsSpec, check


def default_spec():
    """config/default_config.lua's nc_* values (nhip_normals_spec_default; works without a device)."""
    s = NormalsSpec()
    check(_lib.load().nhip_normals_spec_default(C.byref(s)))
    return s


def spec(**overrides):
    """The defaults with the named fields replaced."""
    s = default_spec()
    for k, v in overrides.items():
        if k not in dict(NormalsSpec._fields_):
            raise TypeError("normals.spec: no field %r" % k)
        setattr(s, k, v)
    return s


def estimate(xy, offsets, spec=None, device="cuda:0", info=False):
    """The normals of every point of the packed scans (xy, offsets): float32 (n, 2); with info=True also the int32 (n, 4)
    record of every point {neighbour count, growth steps, winning bin or -1, votes in it | samples << 16}.  A scan whose
    offsets are not a scan raises NhipError (nhip_dev_status)."""
    import torch
    spec = default_spec() if spec is None else spec
    lib, dev = _lib.load(), torch.device(device)
    offsets = np.ascontiguousarray(offsets, dtype=np.int32)
    xy = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
    n_scans, n = len(offsets) - 1, len(xy)
    if n != int(offsets[-1]):
        raise ValueError("normals.estimate: offsets[-1] = %d, but %d points" % (int(offsets[-1]), n))
    z = lambda k, dt: torch.zeros(max(int(k), 1), dtype=dt, device=dev)
    d_xy = torch.from_numpy(xy).to(dev) if n else z(2, torch.float32)
    d_off = torch.from_numpy(offsets).to(dev)
    d_nrm = z(2 * n, torch.float32)  # (zeros: a scan the kernels refuse stays at (0, 0))
    d_info = z(4 * n, torch.int32) if info else None
    sp = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    check(lib.nhip_normals_estimate_dev(d_xy.data_ptr(), d_off.data_ptr(), n_scans, C.byref(spec), d_nrm.data_ptr(),
                                        None if d_info is None else d_info.data_ptr(), sp))
    check(lib.nhip_dev_status(sp, None))
    nrm = d_nrm[:2 * n].cpu().numpy().reshape(n, 2).copy()
    return (nrm, d_info[:4 * n].cpu().numpy().reshape(n, 4).copy()) if info else nrm


def estimate_on_handle(scans, spec=None, info=False):
    """The handle form (nhip_normals_estimate) on a csm.ScanTable."""
    spec = default_spec() if spec is None else spec
    n = len(scans.xy)
    nrm = np.zeros((n, 2), np.float32)
    inf = np.zeros((n, 4), np.int32) if info else None
    check(_lib.load().nhip_normals_estimate(scans._h, C.byref(spec), _lib.ptr(nrm), _lib.ptr(inf)))
    return (nrm, inf) if info else nrm
