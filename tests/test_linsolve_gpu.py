"""The device linear solver on the GPU ("Block-sparse system"; kernels nhip_linsolve.hip and the odometry
rows of nhip_resid.hip; nautilus_amd/linsolve.py, PoseGraph.solve(linear_solver="device")): odometry rows and the assembly bit
for bit against the numpy restatement (tests/linsolve_reference.py), the PCG by its true residual in longdouble and by the
reference's iteration count, and a pose graph solved end to end beside the host solver.  The CPU half: tests/test_linsolve_cpu.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from nautilus_amd import _lib, hostside, linsolve, posegraph
from tests import linsolve_reference as LR
from tests.linsolve_seams import check_pcg

pytestmark = pytest.mark.gpu

LAM, FLOOR, TOL = 1e-3, 1e-9, 1e-10
SENTINEL, PAD = -7.25, 256


@pytest.fixture(scope="module")
def backend(gpu):
    return posegraph.HipBackend()


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


# ------------------------------------------------------------------------------------------------ odometry rows
def odometry_case(n, seed=11):
    """n factors over 9 poses whose heading differences th_i + R_odom - th_j spread over more than [-pi, pi]."""
    rng = np.random.default_rng(seed)
    poses = np.concatenate([rng.uniform(-20, 20, (9, 2)), rng.uniform(-np.pi, np.pi, (9, 1))], axis=1)
    pi, pj = rng.integers(0, 9, n).astype(np.int32), rng.integers(0, 9, n).astype(np.int32)
    t = rng.normal(size=(n, 2)).astype(np.float32)
    r = rng.uniform(-np.pi, np.pi, n).astype(np.float32)
    if n > 2:  # a difference of exactly +-pi and one of 0
        pj[0], r[0] = pi[0], np.float32(np.pi)
        pj[1], r[1] = pi[1], np.float32(0.0)
    return poses, pi, pj, t, r


def odometry_on_device(poses, pi, pj, t, r, tw=1.5, rw=0.75):
    """(rows by nhip_resid_odometry_normal_eq_dev with PAD sentinels behind them, rows formed in numpy from
    nhip_resid_odometry_dev's own r and J)."""
    import torch
    lib, n = _lib.load(), len(pi)
    z = lambda a, dt: _dev(a) if len(a) else torch.zeros(2, dtype=dt, device="cuda:0")
    d_t, d_r, d_i, d_j, d_p = z(t, torch.float32), z(r, torch.float32), z(pi, torch.int32), z(pj, torch.int32), _dev(poses)
    d_out = torch.full((28 * n + PAD,), SENTINEL, dtype=torch.float64, device="cuda:0")
    _lib.check(lib.nhip_resid_odometry_normal_eq_dev(d_t.data_ptr(), d_r.data_ptr(), d_i.data_ptr(), d_j.data_ptr(), n, tw, rw,
                                                     d_p.data_ptr(), len(poses), d_out.data_ptr(), _stream()))
    e = lambda k: torch.zeros(max(k, 1), dtype=torch.float64, device="cuda:0")
    d_res, d_ji, d_jj = e(3 * n), e(9 * n), e(9 * n)
    _lib.check(lib.nhip_resid_odometry_dev(d_t.data_ptr(), d_r.data_ptr(), d_i.data_ptr(), d_j.data_ptr(), n, tw, rw,
                                           d_p.data_ptr(), len(poses), d_res.data_ptr(), d_ji.data_ptr(), d_jj.data_ptr(), _stream()))
    want = LR.odometry_rows(d_res.cpu().numpy()[:3 * n].reshape(n, 3), d_ji.cpu().numpy()[:9 * n].reshape(n, 3, 3),
                            d_jj.cpu().numpy()[:9 * n].reshape(n, 3, 3))
    return d_out.cpu().numpy(), want


@pytest.mark.parametrize("n", [0, 1, 65, 256, 257])
def test_odometry_rows_are_bit_equal_to_numpy_on_the_kernels_own_jacobians(gpu, n):
    out, want = odometry_on_device(*odometry_case(n))
    assert np.array_equal(_bits(out[:28 * n]), _bits(want.ravel()))
    assert np.all(out[28 * n:] == SENTINEL), "the sentinels behind the rows"
    assert _status()[0] == _lib.NHIP_OK
    if n:
        assert np.abs(want[:, :21]).max() > 0 and np.abs(want[:, 21:27]).max() > 0 and want[:, 27].min() >= 0


def test_odometry_rows_of_a_bad_pose_index_are_zero_and_reported(gpu):
    poses, pi, pj, t, r = odometry_case(65)
    pj[40] = len(poses)
    clean = pj.copy()
    clean[40] = 0
    out, _ = odometry_on_device(poses, pi, pj, t, r)
    rc, info = _status()
    assert rc == _lib.NHIP_ERR_ARG and info[0] & 16 and info[1] == 16 and info[2] == len(poses) and info[3] == 40
    good, _ = odometry_on_device(poses, pi, clean, t, r)
    rows, keep = out[:28 * 65].reshape(65, 28), np.arange(65) != 40
    assert not rows[40].any() and np.array_equal(_bits(rows[keep]), _bits(good[:28 * 65].reshape(65, 28)[keep]))
    assert np.all(out[28 * 65:] == SENTINEL) and _status()[0] == _lib.NHIP_OK


# ------------------------------------------------------------------------------------------------ assembly
def assembly_cases():
    arrow_u, arrow_v = LR.arrow_uv()
    chain_u, chain_v = LR.chain_uv(5, 2)
    return {"one_row": (2, np.array([0]), np.array([1])), "chain": (5, chain_u, chain_v), "arrow": (71, arrow_u, arrow_v),
            "no_rows": (4, np.zeros(0, np.int64), np.zeros(0, np.int64)), "one_block": (1, np.zeros(0, np.int64), np.zeros(0, np.int64))}


def assembled(backend, nb, u, v, rows, fixed=(0,)):
    st = linsolve.BlockStructure(nb, u, v)
    system = backend.device_system(st, fixed=fixed)
    system.d_values.fill_(SENTINEL)
    system.d_grad.fill_(SENTINEL)
    cost = system.assemble(_dev(rows.reshape(-1, 28)))
    values, grad, cost2 = system.download()
    assert cost == cost2 or (np.isnan(cost) and np.isnan(cost2))
    return st, system, values, grad, cost


@pytest.mark.parametrize("name", list(assembly_cases()))
def test_assembly_is_bit_equal_to_the_reference(backend, name):
    nb, u, v = assembly_cases()[name]
    rows = LR.random_rows(u, 21)
    st, system, values, grad, cost = assembled(backend, nb, u, v, rows)
    want_v, want_g, want_c = LR.assemble(st, rows)
    lens = np.diff(st.contrib_ptr)
    print("ASSEMBLE %s: %d blocks, %d rows, contributor lists up to %d" % (name, st.nnzb, st.n_rows, lens.max()))
    if name == "arrow":
        assert (lens > 128).sum() >= 3 and ((lens > 64) & (lens <= 128)).sum() >= 2
    assert np.array_equal(_bits(values), _bits(want_v)) and np.array_equal(_bits(grad), _bits(want_g))
    assert _bits(cost) == _bits(want_c)
    if st.n_rows == 0:
        assert not values.any() and not grad.any() and cost == 0.0
    # again on the same input: the same bits
    cost_b = system.assemble(_dev(rows.reshape(-1, 28)))
    values_b, grad_b, _ = system.download()
    assert np.array_equal(_bits(values_b), _bits(values)) and np.array_equal(_bits(grad_b), _bits(grad)) and _bits(cost_b) == _bits(cost)


def test_a_row_of_nans_reaches_only_its_own_blocks(backend):
    nb, u, v = assembly_cases()["arrow"]
    rows = LR.random_rows(u, 21)
    clean = assembled(backend, nb, u, v, rows)
    rows[3] = np.nan  # the row (3, 70)
    st, system, values, grad, cost = assembled(backend, nb, u, v, rows)
    hit = np.array([(r, c) in ((3, 3), (3, 70), (70, 3), (70, 70)) for r, c in zip(st.block_row, st.col)])
    assert np.isnan(values[hit]).all() and np.isnan(cost)
    assert np.array_equal(_bits(values[~hit]), _bits(clean[2][~hit]))
    g, g0 = grad.reshape(-1, 3), clean[3].reshape(-1, 3)
    own = np.isin(np.arange(nb), (3, 70))
    assert np.isnan(g[own]).all() and np.array_equal(_bits(g[~own]), _bits(g0[~own]))


@pytest.mark.parametrize("what", ["contributor", "column"])
def test_bad_ids_in_device_memory_give_a_zero_block_and_their_status_kind(backend, what):
    nb, u, v = assembly_cases()["chain"]
    rows = LR.random_rows(u, 21)
    st, system, values, grad, cost = assembled(backend, nb, u, v, rows)
    k = int(np.nonzero((st.block_row == 2) & (st.col == 3))[0][0])
    if what == "contributor":
        system.d_contrib[int(st.contrib_ptr[k])] = 4 * st.n_rows
        kind, value = 2048, 4 * st.n_rows
    else:
        system.d_col[k] = nb
        kind, value = 4096, nb
    system.d_values.fill_(SENTINEL)
    with pytest.raises(_lib.NhipError):
        system.assemble(_dev(rows))
    system.assemble(_dev(rows), sync=False)
    rc, info = _status()
    assert rc == _lib.NHIP_ERR_ARG and info[0] == kind and info[1:] == [kind, value, k]
    got = system.download()[0]
    keep = np.arange(st.nnzb) != k
    assert not got[k].any() and np.array_equal(_bits(got[keep]), _bits(values[keep]))
    assert _status()[0] == _lib.NHIP_OK


# ------------------------------------------------------------------------------------------------ PCG
@pytest.fixture(scope="module")
def arrow(backend):
    nb, u, v = assembly_cases()["arrow"]
    st, system, values, grad, cost = assembled(backend, nb, u, v, LR.random_rows(u, 7))
    return st, system, values, grad


def test_pcg_on_the_arrow_system(arrow):
    st, system, values, grad = arrow
    assert check_pcg(st, system, values, grad, [0], "arrow") > 3


def test_pcg_does_not_depend_on_check_every(arrow):
    st, system, values, grad = arrow
    runs = [system.solve(LAM, FLOOR, TOL, 5000, check_every=c) for c in (1, 7, 1000)]
    for x, res in runs[1:]:
        assert np.array_equal(_bits(x), _bits(runs[0][0]))
        assert (res.iterations, res.flag, res.relative_residual) == (runs[0][1].iterations, runs[0][1].flag, runs[0][1].relative_residual)
    assert runs[0][1].iterations > 3 and runs[0][1].flag == 0, "more than one batch at check_every 1"


def test_pcg_flags(backend, arrow):
    st, system, values, grad = arrow
    x, res = system.solve(LAM, FLOOR, TOL, 3)
    assert (res.iterations, res.flag) == (3, 1) and np.isfinite(x).all() and np.abs(x).max() > 0 and res.relative_residual > TOL
    # one negated diagonal block (the line block's): p^T A p <= 0
    k = int(np.nonzero((st.block_row == 70) & (st.col == 70))[0][0])
    system.d_values[9 * k:9 * k + 9] *= -1.0
    try:
        x, res = system.solve(LAM, FLOOR, TOL, 5000)
    finally:
        system.d_values[9 * k:9 * k + 9] *= -1.0
    print("negated diagonal block: %r" % res)
    assert res.flag == 2 and np.isfinite(x).all()
    # b = 0
    saved = system.d_grad.clone()
    system.d_grad.zero_()
    try:
        x, res = system.solve(LAM, FLOOR, TOL, 5000)
    finally:
        system.d_grad.copy_(saved)
    assert (res.iterations, res.flag, res.relative_residual) == (0, 0, 0.0) and not x.any()
    # a single block, fixed
    one = backend.device_system(linsolve.BlockStructure(1, [], []), fixed=[0])
    one.d_values.fill_(2.0)
    one.d_grad.fill_(1.0)
    x, res = one.solve(LAM, FLOOR, TOL, 50)
    assert (res.iterations, res.flag) == (0, 0) and x.shape == (3,) and not x.any()


# ------------------------------------------------------------------------------------------------ a pose graph
@pytest.fixture(scope="module")
def graph(backend):
    """The 48-scan, window-10 graph with one loop closure and a device HITL constraint, and its start."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import slam_loop
    from nautilus_amd import csm, synth
    bag = synth.SynthBag(48, dense=True)
    xy, off = csm.pack_scans(bag.scans)
    nrm = np.concatenate(bag.normals).astype(np.float32)
    start = np.array(bag.odom, dtype=np.float64)
    pg = posegraph.PoseGraph(xy, nrm, off, bag.odom, window=10, kind=_lib.NHIP_LIDAR_NORMAL, backend=backend)
    pg.add_loop_closures([47], [0], [bag.true_relative(47, 0)])
    lines = hostside.hitl_segments(slam_loop.synthetic_hitl_message(bag, start, 2, 45))
    con = backend.hitl_select(xy, off, start, lines[0], lines[1])
    assert con.n_blocks >= 4 and con.n_points >= 100
    pg.add_hitl(con)
    return pg, bag, start, con


def test_pcg_on_the_system_of_a_pose_graph(graph):
    pg, bag, start, con = graph
    system = pg._device_system()
    st = system.st
    assert st.n_blocks == 49 and st.n_rows == len(pg.icp.block_src) + 47 + 1 + con.n_blocks
    cost = pg._evaluate_device(system, start, np.array([[0.02, -0.01, 0.003]]), research=True)
    values, grad, cost2 = system.download()
    H, g, cost_host = pg._assemble(start, np.array([[0.02, -0.01, 0.003]]), research=False)
    print("GRAPH: %d blocks, %d rows; cost %.17g (host %.17g); |H - host| max %.3g of %.3g" % (
        st.nnzb, st.n_rows, cost, cost_host, np.abs(st.to_scipy(values) - H).max(), np.abs(H).max()))
    assert cost == cost2 and abs(cost - cost_host) <= 1e-12 * cost_host
    assert np.abs(st.to_scipy(values) - H).max() <= 1e-12 * np.abs(H).max() and np.abs(grad - g).max() <= 1e-12 * np.abs(g).max()
    check_pcg(st, system, values, grad, [0], "graph")


def test_device_solver_end_to_end_beside_the_host_solver(graph, monkeypatch):
    import scipy.sparse.linalg
    pg, bag, start, con = graph

    def solve(**kw):
        pg.poses, con.chosen_line_pose = start.copy(), np.zeros(3)
        for k in pg.linear_stats:
            pg.linear_stats[k] = 0
        return pg.solve(iterations=4, **kw)
    try:
        host, hist_host = solve()
        dev, hist_dev = solve(linear_solver="device", cg_tol=TOL)
        stats, line_dev = dict(pg.linear_stats), con.chosen_line_pose.copy()
        monkeypatch.setattr(scipy.sparse.linalg, "spsolve", lambda A, b: LR.pcg_matrix(A, b, TOL, 5000)[0])
        ref, hist_ref = solve()
    finally:
        pg.poses, con.chosen_line_pose = start.copy(), np.zeros(3)
    d_ref, d_dev = float(np.abs(ref - host).max()), float(np.abs(dev - host).max())
    print("END TO END: d_ref %.3g m, device - host %.3g m (%.3g d_ref); linear_stats %r; errors host %.6f device %.6f; costs %r / %r" % (
        d_ref, d_dev, d_dev / d_ref if d_ref else np.inf, stats, posegraph.trajectory_error(host, bag.truth),
        posegraph.trajectory_error(dev, bag.truth), hist_host, hist_dev))
    assert stats["solves"] == 4 and stats["iterations"] > 0 and stats["not_converged"] == 0 and stats["breakdowns"] == 0
    for hist in (hist_host, hist_dev):
        assert all(b <= a for a, b in zip(hist, hist[1:])) and hist[-1] < hist[0]
    assert np.abs(line_dev).max() > 1e-8
    assert d_dev <= 10 * d_ref
