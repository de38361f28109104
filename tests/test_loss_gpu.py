"""The robust-loss kernel on the GPU ("Robust loss"; nautilus_amd/csrc/nhip_loss.hip,
nhip_resid_odometry_robust_normal_eq_dev): rows bit for bit against numpy on the kernels' own r, J and weights, both forms of the
row store; rho, rho' and sqrt(rho') against the mpmath definition within the derived bounds (tests/loss_reference.py); and a pose
graph with a displaced closure under a loss, both linear solvers.  The CPU half: tests/test_loss_cpu.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from nautilus_amd import _lib, hostside, posegraph
from nautilus_amd.loss import KINDS, Loss
from tests import linsolve_reference as LR
from tests import loss_reference as LS
from tests import resid_reference as RR

pytestmark = pytest.mark.gpu

SENTINEL, PAD = -7.25, 256
SEAMS = [1, 63, 64, 65, 255, 256, 257, 513]  # wave and workgroup seams; for the staged store, the partial last workgroup
STORES = ["direct", "staged"]
TOL = 1e-10


@pytest.fixture(scope="module")
def backend(gpu):
    return posegraph.HipBackend()


@pytest.fixture(params=STORES)
def store(request, monkeypatch):
    """Both forms of the row store (the test process runs with NHIP_TUNABLES=1: tests/conftest.py)."""
    monkeypatch.setenv("NHIP_LOSS_STORE", request.param)
    return request.param


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).to("cuda:0")


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _status():
    info = (C.c_int32 * 4)()
    return _lib.load().nhip_dev_status(_stream(), info), list(info)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def odometry_case(n, seed=11):
    """tests/test_linsolve_gpu.py's factors: n over 9 poses, heading differences spread over more than [-pi, pi]; every fourth
    factor's translation closes to a few centimetres, so that every loss has inliers and outliers."""
    rng = np.random.default_rng(seed)
    poses = np.concatenate([rng.uniform(-20, 20, (9, 2)), rng.uniform(-np.pi, np.pi, (9, 1))], axis=1)
    pi, pj = rng.integers(0, 9, n).astype(np.int32), rng.integers(0, 9, n).astype(np.int32)
    t = rng.normal(size=(n, 2)).astype(np.float32)
    r = rng.uniform(-np.pi, np.pi, n).astype(np.float32)
    near = np.arange(n) % 4 == 0
    t[near] = (poses[pj[near], :2] - poses[pi[near], :2] + rng.normal(0, 0.05, (int(near.sum()), 2))).astype(np.float32)
    r[near] = (poses[pj[near], 2] - poses[pi[near], 2] + rng.normal(0, 0.05, int(near.sum()))).astype(np.float32)
    if n > 2:  # a difference of exactly +-pi and one of 0
        pj[1], r[1] = pi[1], np.float32(np.pi)
        pj[2], r[2] = pi[2], np.float32(0.0)
    return poses, pi, pj, t, r


def on_device(poses, pi, pj, t, r, spec, tw=1.5, rw=0.75, weights=True):
    """(rows by nhip_resid_odometry_robust_normal_eq_dev with PAD sentinels behind them, its weights likewise or None,
    nhip_resid_odometry_dev's own r, J_i, J_j)."""
    import torch
    lib, n = _lib.load(), len(pi)
    z = lambda a, dt: _dev(a) if len(a) else torch.zeros(2, dtype=dt, device="cuda:0")
    d_t, d_r, d_i, d_j, d_p = z(t, torch.float32), z(r, torch.float32), z(pi, torch.int32), z(pj, torch.int32), _dev(poses)
    d_out = torch.full((28 * n + PAD,), SENTINEL, dtype=torch.float64, device="cuda:0")
    d_w = torch.full((4 * n + PAD,), SENTINEL, dtype=torch.float64, device="cuda:0") if weights else None
    _lib.check(lib.nhip_resid_odometry_robust_normal_eq_dev(d_t.data_ptr(), d_r.data_ptr(), d_i.data_ptr(), d_j.data_ptr(), n, tw, rw,
                                                            C.byref(spec), d_p.data_ptr(), len(poses), d_out.data_ptr(),
                                                            d_w.data_ptr() if weights else None, _stream()))
    e = lambda k: torch.zeros(max(k, 1), dtype=torch.float64, device="cuda:0")
    d_res, d_ji, d_jj = e(3 * n), e(9 * n), e(9 * n)
    _lib.check(lib.nhip_resid_odometry_dev(d_t.data_ptr(), d_r.data_ptr(), d_i.data_ptr(), d_j.data_ptr(), n, tw, rw,
                                           d_p.data_ptr(), len(poses), d_res.data_ptr(), d_ji.data_ptr(), d_jj.data_ptr(), _stream()))
    plain = (d_res.cpu().numpy()[:3 * n].reshape(n, 3), d_ji.cpu().numpy()[:9 * n].reshape(n, 3, 3),
             d_jj.cpu().numpy()[:9 * n].reshape(n, 3, 3))
    return d_out.cpu().numpy(), d_w.cpu().numpy() if weights else None, plain


def plain_rows(poses, pi, pj, t, r, tw=1.5, rw=0.75):
    """nhip_resid_odometry_normal_eq_dev's rows of the same factors."""
    import torch
    n = len(pi)
    d_out = torch.full((28 * n + PAD,), SENTINEL, dtype=torch.float64, device="cuda:0")
    d_t, d_r, d_i, d_j, d_p = _dev(t), _dev(r), _dev(pi), _dev(pj), _dev(poses)  # (named: they live until the rows are down)
    _lib.check(_lib.load().nhip_resid_odometry_normal_eq_dev(d_t.data_ptr(), d_r.data_ptr(), d_i.data_ptr(), d_j.data_ptr(), n, tw, rw,
                                                             d_p.data_ptr(), len(poses), d_out.data_ptr(), _stream()))
    return d_out.cpu().numpy()[:28 * n].reshape(n, 28)


SCALE_OF = {"none": 1.0, "huber": 2.0, "soft_l1": 0.37, "cauchy": 3.0}


@pytest.mark.parametrize("n", SEAMS)
@pytest.mark.parametrize("kind", LS.KINDS)
def test_rows_are_bit_equal_to_numpy_on_the_kernels_own_values(gpu, store, kind, n):
    case = odometry_case(n)
    loss = Loss(kind, SCALE_OF[kind])
    out, wt, (r, ji, jj) = on_device(*case, loss.spec())
    rows, wt4 = out[:28 * n].reshape(n, 28), wt[:4 * n].reshape(n, 4)
    assert np.all(out[28 * n:] == SENTINEL) and np.all(wt[4 * n:] == SENTINEL), "the sentinels behind both outputs"
    assert _status()[0] == _lib.NHIP_OK
    want = LS.rows(r, ji, jj, wt4[:, 3], wt4[:, 1])
    assert np.array_equal(_bits(rows[:, :27]), _bits(want[:, :27]))
    assert np.array_equal(_bits(rows[:, 27]), _bits(wt4[:, 1])), "slot 27 is the kernel's own rho"
    assert np.array_equal(_bits(wt4[:, 0]), _bits(LS.squared_norm(r))), "s is the sum of the kernel's own r"
    if kind == "none":
        assert np.all(wt4[:, 2:] == 1.0) and np.array_equal(_bits(wt4[:, 1]), _bits(wt4[:, 0]))
        assert np.array_equal(_bits(rows), _bits(plain_rows(*case))), "NONE is the plain kernel's row"
    else:
        LS.check_values(kind, loss.scale, wt4[:, 0], wt4[:, 1], wt4[:, 2], wt4[:, 3], "device n=%d %s" % (n, store))
        if n >= 63:
            assert wt4[:, 2].min() < 0.5 < wt4[:, 2].max() <= 1.0, "inliers and outliers"
    # the host's arithmetic on the same r: the same weights within the bounds, the branch of huber included
    host = loss.weights(r)
    agree = _bits(host) == _bits(wt4)
    print("device == numpy bit for bit: s %d, rho %d, rho' %d, sqrt(rho') %d of %d" % (*agree.sum(axis=0), n))
    assert agree[:, 0].all()
    # without the weights output: the same rows
    out2, _, _ = on_device(*case, loss.spec(), weights=False)
    assert np.array_equal(_bits(out2), _bits(out))


@pytest.mark.parametrize("a", LS.SCALES)
@pytest.mark.parametrize("kind", LS.KINDS)
def test_values_meet_the_reference_on_the_case_list(gpu, store, kind, a):
    """Factors (pose_i = (u, v, 0), pose_j = 0, no odometry, weights 1) whose s is the case list's, exactly."""
    targets = LS.case_list(a)
    n = len(targets)
    uv = np.array([LS.components(v) for v in targets])
    poses = np.concatenate([np.zeros((1, 3)), np.concatenate([uv, np.zeros((n, 1))], axis=1)])
    pi, pj = np.arange(1, n + 1, dtype=np.int32), np.zeros(n, np.int32)
    loss = Loss(kind, a)
    out, wt, (r, ji, jj) = on_device(poses, pi, pj, np.zeros((n, 2), np.float32), np.zeros(n, np.float32), loss.spec(), tw=1.0, rw=0.75)
    wt4, rows = wt[:4 * n].reshape(n, 4), out[:28 * n].reshape(n, 28)
    assert np.array_equal(_bits(wt4[:, 0]), _bits(targets)), "the kernel's s is the case list"
    LS.check_values(kind, a, wt4[:, 0], wt4[:, 1], wt4[:, 2], wt4[:, 3], "device case list %s" % store)
    host = loss.weights(r)
    agree = _bits(host) == _bits(wt4)
    print("device == numpy bit for bit on the case list: rho %s, rho' %s, sqrt(rho') %s" % tuple(agree[:, k].tolist() for k in (1, 2, 3)))
    if kind == "huber":  # the seam: s == b and one ulp below take the inlier branch, exactly (one ulp above: the bounds)
        assert np.all(wt4[[2, 3], 2] == 1.0) and np.all(wt4[[2, 3], 3] == 1.0) and np.array_equal(_bits(wt4[[2, 3], 1]), _bits(targets[[2, 3]]))
    assert np.array_equal(_bits(rows[:, :27]), _bits(LS.rows(r, ji, jj, wt4[:, 3], wt4[:, 1])[:, :27]))
    assert np.array_equal(_bits(rows[:, 27]), _bits(wt4[:, 1])) and _status()[0] == _lib.NHIP_OK


def test_none_is_the_plain_row_at_the_odometry_wrap(gpu, store):
    E = RR.odometry_edges()
    n = len(E.r_odom)
    poses = np.concatenate([E.pose_i, E.pose_j])
    pi, pj = np.arange(n, dtype=np.int32), np.arange(n, 2 * n, dtype=np.int32)
    for tw, rw in RR.ODOM_WEIGHTS:
        out, wt, (r, _, _) = on_device(poses, pi, pj, E.t_odom, E.r_odom, Loss("none").spec(), tw=tw, rw=rw)
        plain = plain_rows(poses, pi, pj, E.t_odom, E.r_odom, tw=tw, rw=rw)
        assert np.array_equal(_bits(out[:28 * n].reshape(n, 28)), _bits(plain))
        assert np.array_equal(_bits(wt[:4 * n].reshape(n, 4)[:, 0]), _bits(plain[:, 27]))
        assert np.abs(r[:E.n_edge, 2]).max() > 3.14 * rw


def test_rows_of_a_bad_pose_index_are_zero_and_reported(gpu, store):
    poses, pi, pj, t, r = odometry_case(65)
    pj[40] = len(poses)
    clean = pj.copy()
    clean[40] = 0
    spec = Loss("cauchy", 3.0).spec()
    out, wt, _ = on_device(poses, pi, pj, t, r, spec)
    rc, info = _status()
    assert rc == _lib.NHIP_ERR_ARG and info[0] & 16 and info[1] == 16 and info[2] == len(poses) and info[3] == 40
    good, good_wt, _ = on_device(poses, pi, clean, t, r, spec)
    keep = np.arange(65) != 40
    rows, wt4 = out[:28 * 65].reshape(65, 28), wt[:4 * 65].reshape(65, 4)
    assert not rows[40].any() and not wt4[40].any()
    assert np.array_equal(_bits(rows[keep]), _bits(good[:28 * 65].reshape(65, 28)[keep]))
    assert np.array_equal(_bits(wt4[keep]), _bits(good_wt[:4 * 65].reshape(65, 4)[keep]))
    assert np.all(out[28 * 65:] == SENTINEL) and np.all(wt[4 * 65:] == SENTINEL) and _status()[0] == _lib.NHIP_OK


def test_no_factors_touch_nothing(gpu, store):
    poses = np.zeros((3, 3))
    e = np.zeros(0, np.int32)
    out, wt, _ = on_device(poses, e, e, np.zeros((0, 2), np.float32), np.zeros(0, np.float32), Loss("huber", 1.0).spec())
    assert np.all(out == SENTINEL) and np.all(wt == SENTINEL) and _status()[0] == _lib.NHIP_OK


# ------------------------------------------------------------------------------------------------ a pose graph
@pytest.fixture(scope="module")
def graph(backend):
    """tests/test_linsolve_gpu.py's 48-scan, window-10 graph with its device HITL constraint; its one true closure and one
    displaced by 2 m, both under Loss("cauchy", 1.0)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import slam_loop
    from nautilus_amd import csm, synth
    bag = synth.SynthBag(48, dense=True)
    xy, off = csm.pack_scans(bag.scans)
    nrm = np.concatenate(bag.normals).astype(np.float32)
    start = np.array(bag.odom, dtype=np.float64)
    pg = posegraph.PoseGraph(xy, nrm, off, bag.odom, window=10, kind=_lib.NHIP_LIDAR_NORMAL, backend=backend)
    bad = np.array(bag.true_relative(40, 3), dtype=np.float64)
    bad[0] += 2.0
    pg.add_loop_closures([47, 40], [0, 3], [bag.true_relative(47, 0), bad], loss=Loss("cauchy", 1.0))
    lines = hostside.hitl_segments(slam_loop.synthetic_hitl_message(bag, start, 2, 45))
    con = backend.hitl_select(xy, off, start, lines[0], lines[1])
    assert con.n_blocks >= 4 and con.n_points >= 100
    pg.add_hitl(con)
    return pg, bag, start, con


def test_device_and_host_systems_agree_under_a_loss(graph):
    pg, bag, start, con = graph
    system = pg._device_system()
    st, lines = system.st, np.array([[0.02, -0.01, 0.003]])
    assert st.n_rows == len(pg.icp.block_src) + 47 + 2 + con.n_blocks
    cost = pg._evaluate_device(system, start, lines, research=True)
    values, grad, cost2 = system.download()
    H, g, cost_host = pg._assemble(start, lines, research=False)
    print("GRAPH under cauchy: cost %.17g (host %.17g); |H - host| max %.3g of %.3g" % (
        cost, cost_host, np.abs(st.to_scipy(values) - H).max(), np.abs(H).max()))
    assert cost == cost2 and abs(cost - cost_host) <= 1e-12 * cost_host
    assert np.abs(st.to_scipy(values) - H).max() <= 1e-12 * np.abs(H).max() and np.abs(grad - g).max() <= 1e-12 * np.abs(g).max()
    # the loss is in the system: without it the displaced closure's 2 m at weight 10 costs 200
    loss, pg.lc.loss = pg.lc.loss, None
    try:
        _, _, cost_plain = pg._assemble(start, lines, research=False)
    finally:
        pg.lc.loss = loss
    assert cost_plain > cost_host + 150.0


def test_closure_weights_from_the_device_are_the_hosts(graph):
    pg, bag, start, con = graph
    wt = pg.closure_weights(start)
    r, _, _ = pg.lc.evaluate(pg.backend, start)
    host = pg.lc.loss.weights(r)
    assert wt.shape == (2, 4) and np.array_equal(_bits(wt[:, 0]), _bits(host[:, 0]))
    LS.check_values("cauchy", 1.0, wt[:, 0], wt[:, 1], wt[:, 2], wt[:, 3], "closure_weights")
    LS.check_values("cauchy", 1.0, host[:, 0], host[:, 1], host[:, 2], host[:, 3], "Loss.weights")
    print("closure weights at the start: rho' %s" % wt[:, 2].tolist())
    assert wt[1, 2] < 0.01 and wt[0, 2] > wt[1, 2]
    loss, pg.lc.loss = pg.lc.loss, None  # without a loss: s, s, 1, 1
    try:
        one = pg.closure_weights(start)
    finally:
        pg.lc.loss = loss
    assert np.array_equal(_bits(one[:, 0]), _bits(wt[:, 0])) and np.array_equal(_bits(one[:, 1]), _bits(one[:, 0])) and np.all(one[:, 2:] == 1.0)


def test_device_solver_beside_the_host_solver_under_a_loss(graph, monkeypatch):
    import scipy.sparse.linalg
    pg, bag, start, con = graph

    def solve(**kw):
        pg.poses, con.chosen_line_pose = start.copy(), np.zeros(3)
        for k in pg.linear_stats:
            pg.linear_stats[k] = 0
        return pg.solve(iterations=4, **kw)
    try:
        host, hist_host = solve()
        w_host = pg.closure_weights()
        dev, hist_dev = solve(linear_solver="device", cg_tol=TOL)
        stats, w_dev = dict(pg.linear_stats), pg.closure_weights()
        monkeypatch.setattr(scipy.sparse.linalg, "spsolve", lambda A, b: LR.pcg_matrix(A, b, TOL, 5000)[0])
        ref, hist_ref = solve()
    finally:
        pg.poses, con.chosen_line_pose = start.copy(), np.zeros(3)
    d_ref, d_dev = float(np.abs(ref - host).max()), float(np.abs(dev - host).max())
    print("END TO END under cauchy: d_ref %.3g m, device - host %.3g m (%.3g d_ref); linear_stats %r; errors host %.6f device %.6f; "
          "rho' host %s device %s" % (d_ref, d_dev, d_dev / d_ref if d_ref else np.inf, stats, posegraph.trajectory_error(host, bag.truth),
                                       posegraph.trajectory_error(dev, bag.truth), w_host[:, 2].tolist(), w_dev[:, 2].tolist()))
    assert stats["solves"] == 4 and stats["iterations"] > 0 and stats["not_converged"] == 0 and stats["breakdowns"] == 0
    for hist in (hist_host, hist_dev):
        assert all(b <= a for a, b in zip(hist, hist[1:])) and hist[-1] < hist[0]
    assert d_dev <= 10 * d_ref
    for w in (w_host, w_dev):  # the displaced closure stays switched off, the true one in
        assert w[1, 2] < 0.01 and w[0, 2] > 0.5
