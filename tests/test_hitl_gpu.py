"""The HITL path on the GPU (nhip_hitl.hip, resid_p2l_normal_eq_kernel, nautilus_amd/hitl.py, PoseGraph): the selection bit
for bit against hostside.hitl_relevant_poses under the reference's width comparison, the per-block normal equations within
(K + n) 2**-53 (sum of magnitudes) of the longdouble definition and of the per-point kernel's own rows, and a PoseGraph that
assembles and solves the same system from a device constraint as from a host one.  Inputs, expectations and K:
tests/hitl_reference.py; the CPU half: tests/test_hitl_cpu.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from nautilus_amd import _lib, hitl, hostside, posegraph
from tests import hitl_reference as HR, resid_reference as RR

pytestmark = pytest.mark.gpu

LD = RR.LD
SENTINEL = -7.25
PAD = 512       # doubles of sentinel behind the 28 per block


@pytest.fixture(scope="module")
def backend(gpu):
    return posegraph.HipBackend()


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).to("cuda:0")          # (a copy: the builders' arrays are read-only)


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _status():
    info = (C.c_int32 * 4)()
    return _lib.load().nhip_dev_status(_stream(), info), list(info)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------ selection
@pytest.mark.parametrize("name", list(HR.CONFIGS))
def test_selection_is_bit_exact(backend, name):
    s, e = HR.scans(), HR.expected(name)
    la, lb, w, thr = HR.CONFIGS[name]
    con = hitl.select(backend, s.xy, s.offsets, s.poses, la, lb, w, thr)
    print("SELECT %s: n_a %d n_b %d points %d (host %d %d %d)" % (name, con.n_a, con.n_b, con.n_points, e.n_a, e.n_b, len(e.points)))
    assert (con.n_a, con.n_b, con.n_points) == (e.n_a, e.n_b, len(e.points))
    assert con.block_pose.dtype == np.int32 and np.array_equal(con.block_pose, e.block_pose)
    assert np.array_equal(con.block_offsets, e.block_offsets)
    pts = con.d_points.cpu().numpy().reshape(-1, 2)
    assert np.array_equal(_bits(pts), _bits(e.points))
    assert np.array_equal(con.d_block_pose.cpu().numpy(), e.block_pose) and np.array_equal(con.d_block_offsets.cpu().numpy(), e.block_offsets)
    a, b = con.to_host()
    assert [i for i, _ in a] == [i for i, _ in e.a_poses] and [i for i, _ in b] == [i for i, _ in e.b_poses]
    for (_, g), (_, h) in zip(a + b, list(e.a_poses) + list(e.b_poses)):
        assert g.dtype == np.float32 and np.array_equal(_bits(g), _bits(h))
    assert not con.chosen_line_pose.any() and _status()[0] == _lib.NHIP_OK


def _select_raw(name, n_scans=None, pad=64, table=None):
    """nhip_hitl_select_dev on the scans: host copies of (class bytes, counts, scan_block, scan_offset, totals), each with
    `pad` sentinel entries behind it, and the device tensors.  table: a scan table other than hitl_reference's (xy, offsets,
    poses, scans), with name = its (line a, line b, width, threshold)."""
    import torch
    s = HR.scans() if table is None else table
    la, lb, w, thr = HR.CONFIGS[name] if table is None else name
    n = len(s.scans) if n_scans is None else n_scans
    n_pts = int(s.offsets[n])
    d_xy, d_off, d_aff = _dev(s.xy), _dev(s.offsets), _dev(hitl.pose_floats(s.poses))
    full = lambda k, dt, v: torch.full((k + pad,), v, dtype=dt, device="cuda:0")
    d = [full(n_pts, torch.uint8, 77), full(2 * n, torch.int32, -99), full(n, torch.int32, -99), full(n, torch.int32, -99), full(3, torch.int32, -99)]
    spec = hitl.hitl_spec(la, lb, w, thr)
    _lib.check(_lib.load().nhip_hitl_select_dev(d_xy.data_ptr(), d_off.data_ptr(), n, d_aff.data_ptr(), C.byref(spec), d[0].data_ptr(),
                                                d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), _stream()))
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in d], d, (d_xy, d_off), n, n_pts


def test_classes_counts_and_block_ids_of_every_scan(gpu):
    """What nhip_hitl_select_dev leaves behind, scan by scan: class bytes and counts as hostside classifies, block ids in the
    order all a-nodes, then all b-nodes, nothing written behind any output."""
    name = "oblique w0.05 t10"
    s, e = HR.scans(), HR.expected(name)
    (cls, cnt, blk, so, tot), _, _, n, n_pts = _select_raw(name)
    assert np.all(cls[n_pts:] == 77) and np.all(cnt[2 * n:] == -99) and np.all(blk[n:] == -99) and np.all(so[n:] == -99) and np.all(tot[3:] == -99)
    for k in range(n):
        on_a, on_b = HR.classes(name, k)
        want = on_a.astype(np.uint8) + 2 * on_b.astype(np.uint8)
        assert np.array_equal(cls[s.offsets[k]:s.offsets[k + 1]], want), k
        assert cnt[2 * k:2 * k + 2].tolist() == [int(on_a.sum()), int(on_b.sum())], k
    assert tot[:3].tolist() == [e.n_a, e.n_b, len(e.points)]
    want_blk = -np.ones(n, np.int32)
    want_blk[e.block_pose] = np.arange(len(e.block_pose))
    assert np.array_equal(blk[:n], want_blk) and np.array_equal(so[:n][e.block_pose], e.block_offsets[:-1])


def test_no_scans_and_sizes_that_are_not_the_totals(gpu):
    import torch
    lib = _lib.load()
    name = "oblique w0.05 t10"
    (_, _, _, _, tot), _, _, _, _ = _select_raw(name, n_scans=0)
    assert tot[:3].tolist() == [0, 0, 0]
    # all-NULL inputs with n_scans == 0 are fine too
    d_tot = torch.full((3,), -99, dtype=torch.int32, device="cuda:0")
    spec = hitl.default_spec()
    assert lib.nhip_hitl_select_dev(None, None, 0, None, C.byref(spec), None, None, None, None, d_tot.data_ptr(), _stream()) == _lib.NHIP_OK
    assert d_tot.cpu().numpy().tolist() == [0, 0, 0]
    # pack into buffers of other sizes than the totals: nothing is written, the status says so (kind 8)
    e = HR.expected(name)
    _, d, (d_xy, d_off), n, _ = _select_raw(name)
    nb, npts = e.n_a + e.n_b, len(e.points)
    for sizes in ((nb - 1, npts), (nb, npts - 1), (nb + 1, npts + 5)):
        d_pts = torch.full((2 * (npts + 8),), SENTINEL, dtype=torch.float32, device="cuda:0")
        d_bo, d_bp = torch.full((nb + 8,), -99, dtype=torch.int32, device="cuda:0"), torch.full((nb + 8,), -99, dtype=torch.int32, device="cuda:0")
        _lib.check(lib.nhip_hitl_pack_dev(d_xy.data_ptr(), d_off.data_ptr(), n, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                          d[4].data_ptr(), sizes[0], sizes[1], d_pts.data_ptr(), d_bo.data_ptr(), d_bp.data_ptr(), _stream()))
        rc, info = _status()
        assert rc == _lib.NHIP_ERR_ARG and info[1] == 8, (sizes, rc, info)
        assert np.all(d_pts.cpu().numpy() == np.float32(SENTINEL)) and np.all(d_bo.cpu().numpy() == -99) and np.all(d_bp.cpu().numpy() == -99)
    # ... and with the totals: the packed arrays, nothing behind them
    d_pts = torch.full((2 * (npts + 8),), SENTINEL, dtype=torch.float32, device="cuda:0")
    d_bo, d_bp = torch.full((nb + 9,), -99, dtype=torch.int32, device="cuda:0"), torch.full((nb + 8,), -99, dtype=torch.int32, device="cuda:0")
    _lib.check(lib.nhip_hitl_pack_dev(d_xy.data_ptr(), d_off.data_ptr(), n, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                      d[4].data_ptr(), nb, npts, d_pts.data_ptr(), d_bo.data_ptr(), d_bp.data_ptr(), _stream()))
    assert _status()[0] == _lib.NHIP_OK
    pts, bo, bp = d_pts.cpu().numpy(), d_bo.cpu().numpy(), d_bp.cpu().numpy()
    assert np.array_equal(_bits(pts[:2 * npts].reshape(-1, 2)), _bits(e.points)) and np.all(pts[2 * npts:] == np.float32(SENTINEL))
    assert np.array_equal(bo[:nb + 1], e.block_offsets) and np.all(bo[nb + 1:] == -99)
    assert np.array_equal(bp[:nb], e.block_pose) and np.all(bp[nb:] == -99)


# ------------------------------------------------------------------------------------------------ normal equations
def _normal_eq(b, bpose=None):
    """nhip_resid_point_to_line_normal_eq_dev on ne_blocks(): ((n_blocks, 28), the PAD doubles behind them)."""
    import torch
    nb = len(b.sizes)
    out = torch.full((28 * nb + PAD,), SENTINEL, dtype=torch.float64, device="cuda:0")
    a = [_dev(b.segs), _dev(b.pts), _dev(b.offsets), _dev(b.bpose if bpose is None else bpose), _dev(b.bline), _dev(b.poses), _dev(b.lines)]
    _lib.check(_lib.load().nhip_resid_point_to_line_normal_eq_dev(a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), a[3].data_ptr(), a[4].data_ptr(),
                                                                  nb, a[5].data_ptr(), len(b.poses), a[6].data_ptr(), len(b.lines), out.data_ptr(),
                                                                  _stream()))
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    return h[:28 * nb].reshape(nb, 28), h[28 * nb:]


def _rows(b):
    """The per-point kernel's rows of the same blocks (nhip_resid_point_to_line_dev): res (m,), jp, jl (m, 3)."""
    import torch
    m, nb = len(b.pts), len(b.sizes)
    pblock = np.repeat(np.arange(nb, dtype=np.int32), b.sizes)
    d = [_dev(b.segs), _dev(b.pts), _dev(pblock), _dev(b.bpose), _dev(b.bline), _dev(b.poses), _dev(b.lines)]
    o = [torch.full((k * m,), SENTINEL, dtype=torch.float64, device="cuda:0") for k in (1, 3, 3)]
    _lib.check(_lib.load().nhip_resid_point_to_line_dev(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), m, d[3].data_ptr(), d[4].data_ptr(), nb,
                                                        d[5].data_ptr(), nb, d[6].data_ptr(), nb, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(),
                                                        _stream()))
    torch.cuda.synchronize()
    return o[0].cpu().numpy(), o[1].cpu().numpy().reshape(m, 3), o[2].cpu().numpy().reshape(m, 3)


def test_normal_equations_at_every_block_size_and_branch(gpu):
    """Every branch of the functor (the blocks of RR.segments()), then blocks of 0 points, less than a wave, one wave, one
    workgroup, one trip of the row loop (1024 points), one more, two trips: all 28 numbers against the longdouble definition
    and against the host reduction of the per-point kernel's rows; NaN exactly where those rows have NaN; the same bits twice;
    nothing written behind the output."""
    b = HR.ne_blocks()
    got, tail = _normal_eq(b)
    assert _status()[0] == _lib.NHIP_OK
    assert np.array_equal(tail.view(np.int64), np.full(PAD, SENTINEL).view(np.int64)), "written past the end"
    again, _ = _normal_eq(b)
    assert np.array_equal(got.view(np.int64), again.view(np.int64)), "two runs differ"
    res, jp, jl = _rows(b)
    assert _status()[0] == _lib.NHIP_OK
    K, worst = HR.K_P2L_NE, 0.0
    for k, n in enumerate(b.sizes):
        n, o = int(n), int(b.offsets[k])
        if n == 0:
            assert np.array_equal(got[k].view(np.int64), np.zeros(28).view(np.int64)), "an empty block's normal equations are 28 zeros"
            continue
        host = HR.ne_of_rows(res[o:o + n], jp[o:o + n], jl[o:o + n])
        assert np.array_equal(np.isnan(got[k]), np.isnan(host.astype(np.float64))), (k, n)
        assert not np.isnan(host[~np.isnan(b.ne[k])]).any(), (k, n)
        q = [RR.ratio(got[k], b.ne[k], b.m_ne[k]), RR.ratio(host, b.ne[k], b.m_ne[k]), RR.ratio(got[k], host, b.m_ne[k])]
        print("RATIO p2l normal_eq block %d n %d: definition %.4g  rows %.4g  against rows %.4g (bound %d)" % (k, n, q[0], q[1], q[2], K + n))
        worst = max(worst, max(q) / (K + n))
        assert max(q) <= K + n, (k, n, q)
    assert np.isnan(got).any(), "the zero-length segment under a point gives NaN sums"
    print("RATIO p2l normal_eq(ratio/(K+n)) %.4g (bound 1)" % worst)


def test_normal_equations_with_a_pose_index_out_of_range(gpu):
    b = HR.ne_blocks()
    good, _ = _normal_eq(b)
    assert _status()[0] == _lib.NHIP_OK
    k = b.n_cases + HR.NE_SIZES.index(257)
    for value in (len(b.poses) + 3, -1):
        bpose = b.bpose.copy()
        bpose[k] = value
        got, tail = _normal_eq(b, bpose)
        rc, info = _status()
        assert rc == _lib.NHIP_ERR_ARG and info[1:] == [16, value, k], (rc, info)
        others = np.arange(len(b.sizes)) != k
        assert np.array_equal(got[others].view(np.int64), good[others].view(np.int64))
        assert np.array_equal(got[k].view(np.int64), np.zeros(28).view(np.int64))
        assert np.array_equal(tail.view(np.int64), np.full(PAD, SENTINEL).view(np.int64))
    assert _status()[0] == _lib.NHIP_OK


# ------------------------------------------------------------------------------------------------ PoseGraph
def test_posegraph_assembles_and_solves_the_same_system_from_either_constraint(backend, small_bag):
    """A two-segment message on the small bag, as examples/slam_loop.py draws it.  The device constraint and the host
    constraint hold the same points; H, g and the cost differ by the two ways the point-to-line terms are summed.
    Bound, entry by entry, (K + n + 16) 2**-53 M: n the point-to-line terms that meet in the entry, 16 for the handful of ICP
    and odometry terms summed beside them, M the sum of the terms' magnitudes -- the point-to-line ones from the host path's
    per-point rows, the others bounded by Cauchy-Schwarz from the diagonal of the system without the constraint (a sum of
    products J_i J_j is at most sqrt(sum J_i^2 sum J_j^2) in absolute terms)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import slam_loop
    from nautilus_amd import csm
    bag = small_bag
    xy, off = csm.pack_scans(bag.scans)
    nrm = np.concatenate(bag.normals).astype(np.float32)
    start = np.array(bag.odom, dtype=np.float64)
    lines = hostside.hitl_segments(slam_loop.synthetic_hitl_message(bag, start, 2, 45))
    a_poses, b_poses = hostside.hitl_relevant_poses(start, bag.scans, lines[0], lines[1], line_width=np.float64(0.05))
    host = posegraph.HitlConstraint(lines[0], lines[1], a_poses, b_poses)
    pg = posegraph.PoseGraph(xy, nrm, off, bag.odom, window=2, kind=_lib.NHIP_LIDAR_NORMAL, backend=backend)
    dev = backend.hitl_select(xy, off, start, lines[0], lines[1])
    n_points = int(sum(len(p) for _, p in host.blocks))
    assert (dev.n_a, dev.n_b, dev.n_points) == (host.n_a, host.n_b, n_points) and n_points >= 100 and host.n_a + host.n_b >= 4
    N = pg.n
    line0 = np.array([[0.02, -0.01, 0.003]])                      # a line pose off zero: every column of the Jacobian is live
    H0, g0, cost0 = pg._assemble(start, np.zeros((0, 3)), research=True)
    pg.add_hitl(host)
    Hh, gh, ch = pg._assemble(start, line0, research=False)
    pg.hitl = []
    pg.add_hitl(dev)
    Hd, gd, cd = pg._assemble(start, line0, research=False)
    Hh, Hd, NU = Hh.toarray(), Hd.toarray(), 3 * N + 3
    # magnitudes and term counts of the point-to-line part, from the host path's rows
    seg, pts, pb, bp, bl = host.arrays(0)
    r, j0, j1 = backend.point_to_line(seg, pts, pb, bp, bl, start, line0)
    J = np.abs(np.concatenate([j0, j1], axis=1))
    ids = np.concatenate([3 * bp[pb][:, None] + np.arange(3), np.full((len(pts), 1), 3 * N) + np.arange(3)], axis=1)
    M, CNT, Mg, CNTg = np.zeros((NU, NU)), np.zeros((NU, NU)), np.zeros(NU), np.zeros(NU)
    np.add.at(M, (np.repeat(ids, 6, axis=1).ravel(), np.tile(ids, (1, 6)).ravel()), np.einsum("ni,nj->nij", J, J).ravel())
    np.add.at(CNT, (np.repeat(ids, 6, axis=1).ravel(), np.tile(ids, (1, 6)).ravel()), 1.0)
    np.add.at(Mg, ids.ravel(), (J * np.abs(r)[:, None]).ravel())
    np.add.at(CNTg, ids.ravel(), 1.0)
    d0 = np.zeros(NU)
    d0[:3 * N] = H0.diagonal()
    U, K = RR.U, HR.K_P2L_NE
    tol_H = (K + CNT + 16) * U * (M + np.sqrt(np.outer(d0, d0)))
    tol_g = (K + CNTg + 16) * U * (Mg + np.sqrt(d0 * 2.0 * cost0))
    err_H, err_g = np.abs(Hd - Hh), np.abs(gd - gh)
    print("ASSEMBLY worst |dH| / tol %.4g, |dg| / tol %.4g, |dcost| / tol %.4g" % (
        (err_H / np.where(tol_H > 0, tol_H, 1))[tol_H > 0].max(), (err_g / np.where(tol_g > 0, tol_g, 1))[tol_g > 0].max(),
        abs(cd - ch) / ((K + n_points + 16) * U * ch)))
    assert np.all(err_H <= tol_H) and np.all(err_g <= tol_g) and abs(cd - ch) <= (K + n_points + 16) * U * ch
    assert np.abs(Hh[3 * N:, :]).max() > 0 and np.abs(Hh - np.pad(H0.toarray(), ((0, 3), (0, 3)))).max() > 0, "the constraint adds nothing"
    # the solves from the same start
    errs, lines_out = [], []
    for con in (host, dev):
        con.chosen_line_pose = np.zeros(3)
        pg.hitl = []
        pg.add_hitl(con)
        pg.poses = start.copy()
        poses, _ = pg.solve(iterations=4)
        errs.append(posegraph.trajectory_error(poses, bag.truth))
        lines_out.append(con.chosen_line_pose.copy())
    print("SOLVE trajectory errors %r, line poses %r" % (errs, lines_out))
    assert abs(errs[0] - errs[1]) < 1e-6 and any(abs(v) > 1e-8 for v in lines_out[1])


def test_a_backend_without_the_device_form_refuses_a_device_constraint(backend, small_bag):
    from nautilus_amd import csm
    xy, off = csm.pack_scans(small_bag.scans)
    dev = backend.hitl_select(xy, off, small_bag.odom, HR.FAR_A, HR.FAR_B)
    assert dev.n_a == dev.n_b == dev.n_points == 0 and dev.to_host() == ([], [])

    class Plain:
        name = "plain"
    pg = posegraph.PoseGraph.__new__(posegraph.PoseGraph)
    pg.backend, pg.hitl = Plain(), []
    with pytest.raises(TypeError):
        pg.add_hitl(dev)
    pg.add_hitl(posegraph.HitlConstraint(HR.FAR_A, HR.FAR_B, [], []))
    assert len(pg.hitl) == 1
