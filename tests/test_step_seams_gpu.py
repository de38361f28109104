"""The two other copies of the 1024-per-step exclusive scan across their step seams (inputs and what each crosses:
tests/step_seams.py; their preconditions: tests/test_step_seams_cpu.py).

hitl_offsets_kernel (nhip_hitl.hip) through hitl.select and through nhip_hitl_select_dev / nhip_hitl_pack_dev on
sentinel-filled buffers, against hostside.hitl_relevant_poses with the reference's double width comparison: totals,
scan_block, scan_offset, block_pose, block_offsets and the packed points as bytes.

feat_offsets_kernel and feat_pack_kernel (nhip_feat.hip) through nhip_features_pack_dev on synthesised idx / count tables,
with and without normals, against feature_reference.clouds: offsets and packed xy / normals as bytes.

Nothing may be written behind any output.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from nautilus_amd import _lib, hitl, posegraph
from tests import step_seams as S

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.25)
PAD = 64


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).to("cuda:0")  # (a copy: the builders' arrays are read-only)


def _full(n, dtype, value):
    import torch
    return torch.full((n + PAD,), value, dtype=dtype, device="cuda:0")


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _status():
    info = (C.c_int32 * 4)()
    return _lib.load().nhip_dev_status(_stream(), info), list(info)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _untouched(a, n):
    """Everything behind the first n entries still holds its sentinel."""
    tail = a[n:]
    return len(tail) >= PAD and bool(np.all(tail == (SENTINEL if a.dtype == np.float32 else (77 if a.dtype == np.uint8 else -99))))


# ------------------------------------------------------------------------------------------------------------------- HITL
@pytest.fixture(scope="module")
def backend(gpu):
    return posegraph.HipBackend()


@pytest.mark.parametrize("name", list(S.HITL_LISTS))
def test_hitl_selection_across_the_step_seams(backend, name):
    """hitl_offsets_kernel, `for base = 0; base < n_scans; base += 1024` with `carry[0 .. 3]`, and the second pass
    `scan_block[s] = n_a + (-2 - blk); scan_offset[s] += pts_a`: a ragged step, one full step (`sc[t][1023]` is the total), a
    second step of one lane, a third step; runs of non-members across every seam; no a-node at all; no b-node; the first
    a-node behind the first seam."""
    import torch
    s, e = S.hitl_list(name), S.hitl_expected(name)
    n, n_pts = len(s.scans), int(s.offsets[-1])
    nb, npts = e.n_a + e.n_b, len(e.points)
    # the adapter
    con = hitl.select(backend, np.array(s.xy), np.array(s.offsets), s.poses, S.LINE_A, S.LINE_B, S.WIDTH, S.THRESHOLD)
    assert (con.n_a, con.n_b, con.n_points) == (e.n_a, e.n_b, npts)
    assert np.array_equal(con.block_pose, e.block_pose) and np.array_equal(con.block_offsets, e.block_offsets)
    assert np.array_equal(_bits(con.d_points.cpu().numpy().reshape(-1, 2)), _bits(e.points))
    # the two entry points on sentinel-filled buffers
    lib = _lib.load()
    d_xy, d_off, d_aff = _dev(s.xy), _dev(s.offsets), _dev(hitl.pose_floats(s.poses))
    d_cls, d_cnt = _full(n_pts, torch.uint8, 77), _full(2 * n, torch.int32, -99)
    d_blk, d_so, d_tot = _full(n, torch.int32, -99), _full(n, torch.int32, -99), _full(3, torch.int32, -99)
    spec = hitl.hitl_spec(S.LINE_A, S.LINE_B, S.WIDTH, S.THRESHOLD)
    _lib.check(lib.nhip_hitl_select_dev(d_xy.data_ptr(), d_off.data_ptr(), n, d_aff.data_ptr(), C.byref(spec), d_cls.data_ptr(),
                                        d_cnt.data_ptr(), d_blk.data_ptr(), d_so.data_ptr(), d_tot.data_ptr(), _stream()))
    d_pts, d_bo, d_bp = _full(2 * npts, torch.float32, float(SENTINEL)), _full(nb + 1, torch.int32, -99), _full(nb, torch.int32, -99)
    _lib.check(lib.nhip_hitl_pack_dev(d_xy.data_ptr(), d_off.data_ptr(), n, d_cls.data_ptr(), d_cnt.data_ptr(), d_blk.data_ptr(),
                                      d_so.data_ptr(), d_tot.data_ptr(), nb, npts, d_pts.data_ptr(), d_bo.data_ptr(), d_bp.data_ptr(), _stream()))
    torch.cuda.synchronize()
    cls, cnt, blk, so, tot, pts, bo, bp = (t.cpu().numpy() for t in (d_cls, d_cnt, d_blk, d_so, d_tot, d_pts, d_bo, d_bp))
    assert tot[:3].tolist() == [e.n_a, e.n_b, npts]
    assert np.array_equal(blk[:n], e.scan_block), "scan_block differs first at scan %d" % np.nonzero(blk[:n] != e.scan_block)[0][0]
    assert np.array_equal(so[:n], e.scan_offset), "scan_offset differs first at scan %d" % np.nonzero(so[:n] != e.scan_offset)[0][0]
    assert np.array_equal(bp[:nb], e.block_pose) and np.array_equal(bo[:nb + 1], e.block_offsets)
    assert np.array_equal(_bits(pts[:2 * npts].reshape(-1, 2)), _bits(e.points))
    assert np.array_equal(cnt[:2 * n].reshape(n, 2)[e.block_pose, (np.arange(nb) >= e.n_a).astype(int)], np.diff(e.block_offsets))
    for a, k in ((cls, n_pts), (cnt, 2 * n), (blk, n), (so, n), (tot, 3), (pts, 2 * npts), (bo, nb + 1), (bp, nb)):
        assert _untouched(a, k)
    assert _status() == (_lib.NHIP_OK, [0, 0, 0, 0])
    print("HITL %s: %d scans, %d a-nodes, %d b-nodes, %d points equal" % (name, n, e.n_a, e.n_b, npts))


# ------------------------------------------------------------------------------------------------------------ features pack
@pytest.fixture(scope="module")
def feature_cloud(gpu):
    xy, normals, offsets = S.features_cloud()
    return _dev(xy), _dev(normals), _dev(offsets)


@pytest.mark.parametrize("with_normals", [True, False], ids=["normals", "no normals"])
@pytest.mark.parametrize("cap", S.FEATURE_CAPS)
@pytest.mark.parametrize("n", S.FEATURE_SCANS)
def test_features_pack_across_the_step_seams(feature_cloud, n, cap, with_normals):
    """feat_offsets_kernel, `for base = 0; base < n_scans; base += 1024` with `carry`: a ragged step, a second step of one
    lane, a third step of 1, 2 and 3 lanes, runs of scans without features across the seams.  feat_pack_kernel, `s =
    blockIdx.x * (FT / 64) + (threadIdx.x >> 6); if (s >= n_scans) return`: a last workgroup of 1, 2 and 3 scans; `lane < c`
    with caps 1, 20 and 64 (lane 63 live, `(1ull << lane) - 1ull` at 63)."""
    import torch
    d_xy, d_nrm, d_off = feature_cloud
    c = S.features_case(n, cap)
    want = c.expect[with_normals]
    want_xy, want_off = want[0], want[-1]
    m = int(want_off[-1])
    d_idx, d_cnt = _dev(c.idx.reshape(-1)), _dev(c.count)
    d_xo, d_oo = _full(2 * n * cap, torch.float32, float(SENTINEL)), _full(n + 1, torch.int32, -99)
    d_no = _full(2 * n * cap, torch.float32, float(SENTINEL)) if with_normals else None
    _lib.check(_lib.load().nhip_features_pack_dev(d_xy.data_ptr(), d_nrm.data_ptr() if with_normals else None, d_off.data_ptr(), n,
                                                  d_idx.data_ptr(), d_cnt.data_ptr(), cap, d_xo.data_ptr(),
                                                  d_no.data_ptr() if with_normals else None, d_oo.data_ptr(), _stream()))
    torch.cuda.synchronize()
    xo, oo = d_xo.cpu().numpy(), d_oo.cpu().numpy()
    assert np.array_equal(oo[:n + 1], want_off), "offsets differ first at scan %d" % np.nonzero(oo[:n + 1] != want_off)[0][0]
    assert np.array_equal(_bits(xo[:2 * m].reshape(-1, 2)), _bits(want_xy))
    assert _untouched(oo, n + 1) and _untouched(xo, 2 * m)
    if with_normals:
        no = d_no.cpu().numpy()
        assert np.array_equal(_bits(no[:2 * m].reshape(-1, 2)), _bits(want[1])) and _untouched(no, 2 * m)
    assert _status() == (_lib.NHIP_OK, [0, 0, 0, 0])
