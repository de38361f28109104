"""nhip_normals_estimate_dev called directly on device buffers: the one way in that tests/test_normals_gpu.py and
tests/test_normals_edges_gpu.py share."""
import ctypes as C

import numpy as np

from nautilus_amd import _lib

PAD = 8         # entries of filler kept behind the last point of both outputs
INFO_FILL = -7


def estimate_dev(xy, off, spec, want_info=True, fill=0.0):
    """-> (normals (n, 2), info (n, 4) or None, rc and info of nhip_dev_status).  Both outputs are allocated PAD entries longer
    than the points and filled (normals: `fill`, info: INFO_FILL) before the call; what lies behind the last point must come
    back as it was."""
    import torch
    lib, dev = _lib.load(), torch.device("cuda:0")
    xy, off = np.array(xy, np.float32).reshape(-1, 2), np.array(off, np.int32)  # (copies: the shared inputs are read-only)
    n = len(xy)
    d_xy = torch.from_numpy(xy).to(dev) if n else torch.zeros(2, dtype=torch.float32, device=dev)
    d_off = torch.from_numpy(off).to(dev)
    d_nrm = torch.full((n + PAD, 2), fill, dtype=torch.float32, device=dev)
    d_info = torch.full((n + PAD, 4), INFO_FILL, dtype=torch.int32, device=dev) if want_info else None
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.nhip_normals_estimate_dev(d_xy.data_ptr(), d_off.data_ptr(), len(off) - 1, C.byref(spec), d_nrm.data_ptr(),
                                             None if d_info is None else d_info.data_ptr(), sp))
    st = (C.c_int32 * 4)()
    rc = lib.nhip_dev_status(sp, st)
    nrm, info = d_nrm.cpu().numpy(), None if d_info is None else d_info.cpu().numpy()
    assert np.array_equal(nrm[n:].view(np.uint32), np.full((PAD, 2), fill, np.float32).view(np.uint32)), "normals written past the last point"
    assert info is None or np.all(info[n:] == INFO_FILL), "info written past the last point"
    return nrm[:n], None if info is None else info[:n], (rc, list(st))
