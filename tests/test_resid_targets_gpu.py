"""The residual kernels (nhip_resid.hip, and their host forms in nhip_host_solver.hip) against the high-precision definitions
of tests/resid_reference.py, at the sizes, branches and poses where they can go wrong: every loop shape of the per-block
normal equations, the tail tile of the per-row kernel, single blocks through the handle, far and rotated poses, every
branch of the point-to-line distance, the odometry wrap.  Every value is held to K * 2**-53 * magnitude (sums of n rows to
(K + n) * 2**-53 * sum of magnitudes), K per family as measured on the CPU (tests/test_resid_targets_cpu.py).  Each test
prints the worst ratio it saw before it asserts ("RATIO <family> <what> <figure>")."""
import ctypes as C

import numpy as np
import pytest

from nautilus_amd import _lib, residuals as R
from oracle import oracle as O
from tests import resid_reference as RR

pytestmark = pytest.mark.gpu

LD = RR.LD
KINDS = [_lib.NHIP_LIDAR_NORMAL, _lib.NHIP_LIDAR_POINT]
SENTINEL = -7.25
PAD = 2048      # doubles of sentinel behind every output: 16 KiB, more than one whole tile of Jacobian stores (3 * 256 * 16 B)


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).to("cuda:0")          # (a copy: the builders' arrays are read-only)


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _status():
    info = (C.c_int32 * 4)()
    return _lib.load().nhip_dev_status(_stream(), info), list(info)


def _hold(family, what, got, ref, mag, K, n=0):
    q = RR.ratio(got, ref, mag)
    print("RATIO %s %s %.4g (bound %d)" % (family, what, q, K + n))
    assert q <= K + n, (family, what, q)
    return q


def _lidar_dev(kind, c, want_src=True, want_tgt=True, pad=0):
    """nhip_resid_lidar_dev on a builder's batch: (res (2n,), js, jt ((2n, 3) or None), tails) -- tails: what stands in the
    `pad` doubles behind each output afterwards."""
    import torch
    n, nb = len(c.corr), len(c.src)
    full = lambda k: torch.full((k * n + pad,), SENTINEL, dtype=torch.float64, device="cuda:0")
    d_res, d_js, d_jt = full(2), full(6) if want_src else None, full(6) if want_tgt else None
    consts = torch.empty(8 * nb, dtype=torch.float64, device="cuda:0")
    a = [_dev(c.corr), _dev(c.corr_block), _dev(c.src), _dev(c.tgt), _dev(c.poses)]
    _lib.check(_lib.load().nhip_resid_lidar_dev(kind, a[0].data_ptr(), a[1].data_ptr(), n, a[2].data_ptr(), a[3].data_ptr(), nb,
                                                a[4].data_ptr(), len(c.poses), consts.data_ptr(), d_res.data_ptr(),
                                                d_js.data_ptr() if want_src else None, d_jt.data_ptr() if want_tgt else None, _stream()))
    torch.cuda.synchronize()
    host = [None if t is None else t.cpu().numpy() for t in (d_res, d_js, d_jt)]
    outs = [None if h is None else h[:len(h) - pad] for h in host]
    tails = [None if h is None else h[len(h) - pad:] for h in host]
    return outs[0], None if outs[1] is None else outs[1].reshape(-1, 3), None if outs[2] is None else outs[2].reshape(-1, 3), tails


def _hold_rows(what, ref, res, js, jt, rows=slice(None)):
    _hold("lidar", what + " res", res, ref.res[rows], ref.m_res[rows], RR.K_LIDAR)
    if js is not None:
        _hold("lidar", what + " jac_src", js, ref.js[rows], ref.m_js[rows], RR.K_LIDAR)
    if jt is not None:
        _hold("lidar", what + " jac_tgt", jt, ref.jt[rows], ref.m_jt[rows], RR.K_LIDAR)


def _normal_eq(kind, b, src=None):
    import torch
    nb = len(b.src)
    out = torch.full((28 * nb,), SENTINEL, dtype=torch.float64, device="cuda:0")
    consts = torch.empty(8 * nb, dtype=torch.float64, device="cuda:0")
    a = [_dev(b.corr), _dev(b.offsets), _dev(b.src if src is None else src), _dev(b.tgt), _dev(b.poses)]
    _lib.check(_lib.load().nhip_resid_lidar_normal_eq_dev(kind, a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), a[3].data_ptr(), nb,
                                                          a[4].data_ptr(), len(b.poses), consts.data_ptr(), out.data_ptr(), _stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(nb, 28)


# ------------------------------------------------------------------------------------------------ normal equations
@pytest.mark.parametrize("shift", range(4))
@pytest.mark.parametrize("kind", KINDS)
def test_normal_equations_at_every_block_size(gpu, kind, shift):
    """Blocks of 0 rows, less than a wave, one wave, one trip of the row loop (1280 rows), one row more, two trips, more:
    all 28 numbers of every block, on every pose pair over the four shifts."""
    b, ref = RR.blocks_by_size(kind, shift), RR.blocks_reference(kind, shift)
    got = _normal_eq(kind, b)
    assert _status()[0] == _lib.NHIP_OK
    res, js, jt, _ = _lidar_dev(kind, b)
    J = np.concatenate([js.reshape(-1, 2, 3), jt.reshape(-1, 2, 3)], axis=2).astype(LD)
    r = res.reshape(-1, 2).astype(LD)
    worst = 0.0
    for k, n in enumerate(b.sizes):
        n, o = int(n), int(b.offsets[k])
        if n == 0:
            assert np.array_equal(got[k], np.zeros(28)), "an empty block's normal equations are 28 zeros"
            continue
        q = RR.ratio(got[k], ref.ne[k], ref.m_ne[k])
        worst = max(worst, q / (RR.K_LIDAR + n))
        assert q <= RR.K_LIDAR + n, (n, q)
        # the same numbers formed on the host from the per-row kernel's own rows
        host = RR.normal_equations(r[o:o + n], J[o:o + n])
        assert RR.ratio(host, ref.ne[k], ref.m_ne[k]) <= RR.K_LIDAR + n, n
        assert RR.ratio(got[k], host, ref.m_ne[k]) <= RR.K_LIDAR + n, n
    print("RATIO lidar normal_eq(ratio/(K+n)) %.4g (bound 1)" % worst)


@pytest.mark.parametrize("kind", KINDS)
def test_normal_equations_with_a_pose_index_out_of_range(gpu, kind):
    b = RR.blocks_by_size(kind, 0)
    good = _normal_eq(kind, b)
    assert _status()[0] == _lib.NHIP_OK
    k = int(np.flatnonzero(b.sizes == 257)[0])
    src = b.src.copy()
    src[k] = len(b.poses) + 3
    got = _normal_eq(kind, b, src)
    rc, info = _status()
    assert rc == _lib.NHIP_ERR_ARG and info[1:] == [16, len(b.poses) + 3, k]
    others = np.arange(len(b.src)) != k
    assert np.array_equal(got[others].view(np.int64), good[others].view(np.int64)) and np.isfinite(got[k]).all()
    assert _status()[0] == _lib.NHIP_OK


# ------------------------------------------------------------------------------------------------ per-row kernel
@pytest.mark.parametrize("kind", KINDS)
def test_per_row_kernel_at_tile_edges_writes_nothing_past_the_end(gpu, kind):
    tail = np.full(PAD, SENTINEL).view(np.int64)
    for i, c in enumerate(RR.tile_edges()):
        ref = RR.tile_reference(kind, i)
        first = None
        for want_src, want_tgt in ((False, False), (True, False), (False, True), (True, True)):
            res, js, jt, tails = _lidar_dev(kind, c, want_src, want_tgt, pad=PAD)
            for t in tails:
                assert t is None or np.array_equal(t.view(np.int64), tail), "n_corr %d: written past the end" % c.n
            _hold_rows("tile n=%d" % c.n, ref, res, js, jt)
            first = res if first is None else first
            assert np.array_equal(res, first)
        assert _status()[0] == _lib.NHIP_OK


@pytest.mark.parametrize("kind", KINDS)
def test_handle_forms_at_tile_edges(gpu, kind):
    """nhip_resid_batch_eval, _eval_compact and _eval_q + nhip_resid_jacobians_from_q on the same batches (the handle takes
    no empty block: the single row is a batch of one block)."""
    lib = _lib.load()
    for i, c in enumerate(RR.tile_edges()):
        ref, n = RR.tile_reference(kind, i), c.n
        keep = np.flatnonzero(c.sizes > 0)
        blocks = [c.corr[c.offsets[k]:c.offsets[k + 1]] for k in keep]
        batch = R.LidarResidualBatch(kind, blocks, c.src[keep], c.tgt[keep], len(c.poses))
        res, js, jt = batch.evaluate(c.poses)
        _hold_rows("eval n=%d" % n, ref, res, js, jt)
        r2, js2, jtt = np.empty(2 * n), np.empty((2 * n, 3)), np.empty(2 * n)
        _lib.check(lib.nhip_resid_batch_eval_compact(batch._h, _lib.ptr(c.poses), _lib.ptr(r2), _lib.ptr(js2), _lib.ptr(jtt)))
        assert np.array_equal(r2, res) and np.array_equal(js2, js) and np.array_equal(jtt, jt[:, 2])
        _hold("lidar", "eval_compact n=%d jac_tgt theta" % n, jtt, ref.jt[:, 2], ref.m_jt[:, 2], RR.K_LIDAR)
        r3, js3, jt3 = batch.evaluate_q(c.poses)
        assert np.array_equal(r3, res) and np.array_equal(js3, js) and np.array_equal(jt3, jt)
        _hold_rows("eval_q n=%d" % n, ref, r3, js3, jt3)
        batch.close()


@pytest.mark.parametrize("shift", range(4))
@pytest.mark.parametrize("kind", KINDS)
def test_per_row_kernel_at_far_and_rotated_poses(gpu, kind, shift):
    """The four pose pairs of blocks_by_size -- near the origin, one pose twice, +-(pi - 1e-9) about 250 m out, 1e4 m out at
    1000.3 rad -- entry by entry."""
    b, ref = RR.blocks_by_size(kind, shift), RR.blocks_reference(kind, shift)
    res, js, jt, _ = _lidar_dev(kind, b)
    assert _status()[0] == _lib.NHIP_OK
    pair = np.repeat(np.repeat(b.src // 2, b.sizes), 2)
    for p in range(4):
        rows = pair == p
        _hold_rows("pose pair %d" % p, ref, res[rows], js[rows], jt[rows], rows)


# ------------------------------------------------------------------------------------------------ one block of a handle
@pytest.mark.parametrize("kind", KINDS)
def test_single_blocks_of_a_batch_at_other_poses(gpu, kind):
    lib = _lib.load()
    rng = np.random.default_rng(31 + kind)
    sizes = [1, 255, 256, 257, 700]
    src, tgt = np.arange(0, 10, 2, dtype=np.int32), np.arange(1, 10, 2, dtype=np.int32)
    old = np.concatenate([rng.normal(0, 2, (10, 2)), rng.uniform(-3, 3, (10, 1))], axis=1)
    new = np.concatenate([rng.normal(0, 30, (10, 2)), rng.uniform(-7, 7, (10, 1))], axis=1)
    new[8:] = RR.PAIR_POSES[6:]                                  # the last block far out
    blocks = [RR._rows_for_pair(rng, n, new[s], new[t]) for n, s, t in zip(sizes, src, tgt)]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    batch = R.LidarResidualBatch(kind, blocks, src, tgt, 10)
    at_old = batch.evaluate(old)
    ref = RR.lidar_reference(kind, batch.corr, off, src, tgt, new)
    got = [np.empty(2 * batch.n_corr), np.empty((2 * batch.n_corr, 3)), np.empty((2 * batch.n_corr, 3))]
    for b in reversed(range(5)):
        rows = slice(2 * off[b], 2 * off[b + 1])
        out = [np.ascontiguousarray(g[rows]) for g in got]
        _lib.check(lib.nhip_resid_batch_eval_block(batch._h, b, _lib.ptr(new[src[b]]), _lib.ptr(new[tgt[b]]), _lib.ptr(out[0]),
                                                   _lib.ptr(out[1]), _lib.ptr(out[2])))
        _hold_rows("eval_block %d rows" % sizes[b], ref, out[0], out[1], out[2], rows)
        for g, o in zip(got, out):
            g[rows] = o
        r_only = np.empty_like(out[0])
        _lib.check(lib.nhip_resid_batch_eval_block(batch._h, b, _lib.ptr(new[src[b]]), _lib.ptr(new[tgt[b]]), _lib.ptr(r_only), None, None))
        assert np.array_equal(r_only, out[0])
    for bad in (-1, 5):
        assert lib.nhip_resid_batch_eval_block(batch._h, bad, _lib.ptr(new[0]), _lib.ptr(new[1]), _lib.ptr(got[0]), None, None) == _lib.NHIP_ERR_ARG
    again = batch.evaluate(old)
    assert all(np.array_equal(a, b) for a, b in zip(again, at_old)), "single-block evaluations changed the batch"
    at_new = batch.evaluate(new)
    assert all(np.array_equal(a, b) for a, b in zip(at_new, got)), "a block alone differs from the block in its batch"
    batch.close()


def test_bad_block_id_under_a_block_base_is_reported_as_the_caller_wrote_it(gpu):
    """A slice of a batch keeps its rows' batch-wide block ids and passes the first of them as block_base: what
    nhip_resid_batch_eval_block does.  The handle never holds a wrong id, so this goes through the launcher it calls
    (nhip::launch_resid_lidar, nhip_common.h): an id outside [base, base + n_blocks) is reported with the value in the
    caller's array, its row is zero, and the other rows are what the same slice gives under base 0."""
    import torch
    fn = getattr(_lib.load(), "_ZN4nhip18launch_resid_lidarEiPKfPKilS3_S3_iPKdiPdS6_S6_S6_P12ihipStream_tS6_iS6_")
    vp, i32 = C.c_void_p, C.c_int32
    fn.restype, fn.argtypes = C.c_int, [C.c_int, vp, vp, C.c_int64, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, i32, vp]
    c = RR.tile_edges()[3]                                       # 257 rows in three blocks
    n, base = c.n, 40

    def run(ids, block_base):
        d_res = torch.full((2 * n,), SENTINEL, dtype=torch.float64, device="cuda:0")
        d_js = torch.full((6 * n,), SENTINEL, dtype=torch.float64, device="cuda:0")
        consts = torch.empty(24, dtype=torch.float64, device="cuda:0")
        a = [_dev(c.corr), _dev(ids.astype(np.int32)), _dev(c.src), _dev(c.tgt), _dev(c.poses)]
        _lib.check(fn(_lib.NHIP_LIDAR_NORMAL, a[0].data_ptr(), a[1].data_ptr(), n, a[2].data_ptr(), a[3].data_ptr(), 3, a[4].data_ptr(),
                      len(c.poses), consts.data_ptr(), d_res.data_ptr(), d_js.data_ptr(), None, _stream(), None, block_base, None))
        torch.cuda.synchronize()
        rc, info = _status()
        return rc, info, d_res.cpu().numpy().reshape(n, 2), d_js.cpu().numpy().reshape(n, 6)
    rc, _, r0, j0 = run(c.corr_block, 0)
    assert rc == _lib.NHIP_OK
    rc, _, r1, j1 = run(c.corr_block + base, base)
    assert rc == _lib.NHIP_OK and np.array_equal(r1, r0) and np.array_equal(j1, j0)
    for row, bad in ((200, base + 3), (256, base - 1), (7, 2)):
        ids = c.corr_block + base
        ids[row] = bad
        rc, info, r, j = run(ids, base)
        assert rc == _lib.NHIP_ERR_ARG and info[1:] == [8, bad, row], info
        keep = np.arange(n) != row
        assert np.array_equal(r[keep], r0[keep]) and np.array_equal(j[keep], j0[keep]) and not r[row].any() and not j[row].any()
    assert _status()[0] == _lib.NHIP_OK


# ------------------------------------------------------------------------------------------------ point to line
def _p2l_both_entries(a):
    """nhip_resid_point_to_line_dev and nhip_resid_point_to_line on segments_arrays(): [(res, jp, jl)] * 2."""
    import torch
    lib = _lib.load()
    m, nb = len(a.pts), len(a.segs)
    d = [_dev(a.segs), _dev(a.pts), _dev(a.pblock), _dev(a.bpose), _dev(a.bline), _dev(a.poses), _dev(a.lines)]
    o = [torch.full((k * m,), SENTINEL, dtype=torch.float64, device="cuda:0") for k in (1, 3, 3)]
    _lib.check(lib.nhip_resid_point_to_line_dev(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), m, d[3].data_ptr(), d[4].data_ptr(), nb,
                                                d[5].data_ptr(), nb, d[6].data_ptr(), nb, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(),
                                                _stream()))
    torch.cuda.synchronize()
    assert _status()[0] == _lib.NHIP_OK
    dev = (o[0].cpu().numpy(), o[1].cpu().numpy().reshape(m, 3), o[2].cpu().numpy().reshape(m, 3))
    r, j0, j1 = np.full(m, SENTINEL), np.full((m, 3), SENTINEL), np.full((m, 3), SENTINEL)
    _lib.check(lib.nhip_resid_point_to_line(_lib.ptr(a.segs), _lib.ptr(a.pts), _lib.ptr(a.pblock), m, _lib.ptr(a.bpose), _lib.ptr(a.bline), nb,
                                            _lib.ptr(a.poses), nb, _lib.ptr(a.lines), nb, _lib.ptr(r), _lib.ptr(j0), _lib.ptr(j1)))
    return [dev, (r, j0, j1)]


def test_point_to_line_on_every_branch(gpu):
    """Inside on both sides of the line, past either end, exactly on the line and on the ends, zero-length segments, and
    axis-aligned segments, where IsBetween(v, a, a) decides by two roundings: values and Jacobians within bounds of the
    definition, NaN exactly where the oracle has NaN, the oracle's outcome at every axis-aligned point."""
    cases = RR.segments()
    for entry, (res, jp, jl) in zip(("dev", "host"), _p2l_both_entries(RR.segments_arrays())):
        o = 0
        for c in cases:
            k, r = len(c.pts), c.ref
            g, g0, g1 = res[o:o + k], jp[o:o + k], jl[o:o + k]
            o += k
            wr, w0, w1 = O.point_to_line_block(c.seg, c.pts, c.pose, c.line)
            assert np.array_equal(np.isnan(g), np.isnan(wr)) and not np.isnan(wr).any() and np.all(g >= 0)
            assert np.array_equal(np.isnan(g0), np.isnan(w0)) and np.array_equal(np.isnan(g1), np.isnan(w1))
            what = "%s %s %s" % (entry, c.tag, c.seg.tolist())
            _hold("p2l", what + " res", g, r.res, r.m_res, RR.K_P2L)
            _hold("p2l", what + " jac_pose", g0, r.jp, r.m_jp, RR.K_P2L)
            _hold("p2l", what + " jac_line", g1, r.jl, r.m_jl, RR.K_P2L)
            if c.tag == "axis":
                sd, de = np.abs(r.sd).astype(np.float64), r.d_end.astype(np.float64)
                clear = de - sd > 1e-6
                assert np.array_equal((np.abs(g - sd) < np.abs(g - de))[clear], r.inside[clear])
            if c.tag in ("exact", "zero"):
                on = r.res == 0
                assert np.array_equal(g[on], np.zeros(on.sum())) and (on.any() or c.tag == "zero")


# ------------------------------------------------------------------------------------------------ odometry
def test_odometry_at_the_wrap(gpu):
    """d = th_i + r_odom - th_j at 0, +-pi, +-2 pi, one double step either side of +-pi, pi +- 1e-9, around th = 0 and
    th = 1e3, and 200 random factors; device-pointer and host-pointer entry, both weight pairs."""
    import torch
    lib = _lib.load()
    e = RR.odometry_edges()
    n = len(e.r_odom)
    poses = np.concatenate([e.pose_i, e.pose_j])
    pi, pj = np.arange(n, dtype=np.int32), np.arange(n, 2 * n, dtype=np.int32)
    for tw, rw in RR.ODOM_WEIGHTS:
        ref = RR.odometry_reference(e.t_odom, e.r_odom, tw, rw, e.pose_i, e.pose_j)
        d = [_dev(e.t_odom), _dev(e.r_odom), _dev(pi), _dev(pj), _dev(poses)]
        o = [torch.full((k * n,), SENTINEL, dtype=torch.float64, device="cuda:0") for k in (3, 9, 9)]
        _lib.check(lib.nhip_resid_odometry_dev(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), n, tw, rw, d[4].data_ptr(),
                                               2 * n, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), _stream()))
        torch.cuda.synchronize()
        assert _status()[0] == _lib.NHIP_OK
        dev = (o[0].cpu().numpy().reshape(n, 3), o[1].cpu().numpy().reshape(n, 3, 3), o[2].cpu().numpy().reshape(n, 3, 3))
        res, ji, jj = np.full((n, 3), SENTINEL), np.full((n, 3, 3), SENTINEL), np.full((n, 3, 3), SENTINEL)
        _lib.check(lib.nhip_resid_odometry(_lib.ptr(e.t_odom), _lib.ptr(e.r_odom), _lib.ptr(pi), _lib.ptr(pj), n, tw, rw, _lib.ptr(poses), 2 * n,
                                           _lib.ptr(res), _lib.ptr(ji), _lib.ptr(jj)))
        want_sign = np.array([np.sign(O.odometry_block(e.t_odom[f], e.r_odom[f], tw, rw, e.pose_i[f], e.pose_j[f])[0][2])
                              for f in range(e.n_edge)])
        assert np.array_equal(want_sign, np.sign(ref.w[:e.n_edge]))
        for entry, (g, g0, g1) in (("dev", dev), ("host", (res, ji, jj))):
            assert np.array_equal(np.sign(g[:e.n_edge, 2]), want_sign), "a wrap case came out on the other side"
            what = "%s weights %s" % (entry, (tw, rw))
            _hold("odometry", what + " res", g, ref.res, ref.m_res, RR.K_ODOM)
            _hold("odometry", what + " jac_i", g0, ref.ji, ref.m_ji, RR.K_ODOM)
            _hold("odometry", what + " jac_j", g1, ref.jj, ref.m_ji, RR.K_ODOM)
