"""The loop with relative-pose closures on the GPU (examples/slam_loop.py, --lc-factor relative; DESIGN.md section 3,
"Relative-pose factors"): the conditions of tests/test_relpose_cpu.py on HipBackend with both linear solvers, the two solvers
beside each other, closure_weights() from the kernel, and cross_covariances on a graph that holds such factors."""
import numpy as np
import pytest

from nautilus_amd import _lib, hostside, posegraph
from nautilus_amd.loss import Loss
from tests import loss_loop as LL
from tests import loss_reference as LS
from tests.relpose_reference import bits
from tests.test_relpose_cpu import check_loop_ratios

pytestmark = pytest.mark.gpu

# tests/test_loss_loop_gpu.py holds either solver's err_lc_m under a loss within 5 % of the run without one
# (tests/loss_loop.check_loop_conditions); the same 5 % is what the two solvers may differ by here
SOLVER_TOL = 0.05


@pytest.fixture(scope="module")
def backend(gpu):
    return posegraph.HipBackend()


@pytest.fixture(scope="module")
def hip_loops(backend):
    import examples.slam_loop as loop
    run = lambda **kw: loop.run(backend=backend, lc_refine="icp", **dict(LL.KW, **kw))
    return {solver: {(drift, factor): run(drift_th_deg=drift, lc_factor=factor, linear_solver=solver)
                     for drift in (0.3, 5.0) for factor in (None, "relative")} for solver in ("host", "device")}


@pytest.mark.parametrize("solver", ["host", "device"])
def test_loop_closes_tighter_with_relative_factors_on_the_device(hip_loops, solver):
    runs = hip_loops[solver]
    check_loop_ratios(runs)
    rel = runs[(5.0, "relative")]
    assert rel["linear_solver"] == solver and rel["backend"] == "hip"
    if solver == "device":
        assert rel["pcg_by_phase"]["lc"][0] > 0 and rel["pcg_not_converged"] == 0


def test_the_two_linear_solvers_agree_on_the_closed_loop(hip_loops):
    for key in ((0.3, "relative"), (5.0, "relative")):
        host, dev = hip_loops["host"][key], hip_loops["device"][key]
        print("drift %.1f: err_lc_m host %.6f device %.6f" % (key[0], host["err_lc_m"], dev["err_lc_m"]))
        assert abs(dev["err_lc_m"] - host["err_lc_m"]) <= SOLVER_TOL * host["err_lc_m"]
        assert dev["lc_accepted"] == host["lc_accepted"] and dev["lc_info_from_icp"] == host["lc_info_from_icp"]
        # (the refinement starts from lattice poses, which see the window solve's poses only through theta0: the same H up to
        # what the two solvers' last digits move the points' float affines by)
        for k in ("lc_info_eig_min", "lc_info_eig_max"):
            assert abs(dev[k] - host[k]) <= 1e-6 * host[k], k


@pytest.fixture(scope="module")
def graph(backend):
    """tests/test_covariance_gpu.py's 40-scan, window-3 graph, solved, with three relative-pose closures -- one displaced by 2 m --
    under Loss("cauchy", 3.0): informations of a room pair's size."""
    from nautilus_amd import csm, synth
    bag = synth.SynthBag(40, dense=True)
    xy, off = csm.pack_scans(bag.scans)
    nrm = np.concatenate(bag.normals).astype(np.float32)
    pg = posegraph.PoseGraph(xy, nrm, off, bag.odom, window=3, kind=_lib.NHIP_LIDAR_NORMAL, backend=backend)
    pg.solve(iterations=3)
    src, tgt = [39, 38, 37], [0, 1, 2]
    rel = np.array([bag.true_relative(s, t) for s, t in zip(src, tgt)], dtype=np.float64)
    rel[1, 0] += 2.0
    info = np.array([[420.0, -35.0, 610.0, 230.0, 95.0, 16000.0], [300.0, 20.0, -400.0, 500.0, 60.0, 9000.0], [0.0] * 6])
    pg.add_loop_closures(src, tgt, rel, loss=Loss("cauchy", 3.0), information=info)
    return pg


def test_closure_weights_are_the_kernels(graph):
    pg = graph
    assert isinstance(pg.lc, posegraph.RelativePoseFactors) and pg.lc.info[2].tolist() == [100.0, 0.0, 0.0, 100.0, 0.0, 100.0]
    wt = pg.closure_weights()
    r, ji, jj = pg.lc.evaluate(pg.backend, pg.poses)
    assert wt.shape == (3, 4) and np.array_equal(bits(wt[:, 0]), bits(LS.squared_norm(r))), "s of the kernel's own residuals"
    LS.check_values("cauchy", 3.0, wt[:, 0], wt[:, 1], wt[:, 2], wt[:, 3], "closure_weights, relative")
    host = hostside.relpose_rows(pg.lc.z, pg.lc.info, pg.lc.pose_i, pg.lc.pose_j, pg.poses, loss=pg.lc.loss)
    print("closure weights: rho' %s (host form %s)" % (wt[:, 2].tolist(), host[4][:, 2].tolist()))
    assert np.allclose(wt, host[4], rtol=1e-9, atol=0.0)
    assert wt[1, 2] < 0.01 and wt[0, 2] > 0.5 and wt[2, 2] > 0.5, "the displaced closure is switched off, the true ones are in"
    # the device system's rows of these factors are the kernel's, and its cost is the host assembly's
    system = pg._device_system()
    lines = np.zeros((0, 3))
    cost = pg._evaluate_device(system, pg.poses, lines, research=True)
    _, _, cost_host = pg._assemble(pg.poses, lines, research=False)
    assert abs(cost - cost_host) <= 1e-12 * cost_host


def test_cross_covariances_on_a_graph_with_relative_factors(graph):
    pg = graph
    pairs = [(30, 5), (5, 30), (12, 13), (1, 39)]
    host = pg.cross_covariances(pairs, dtype=np.float64)
    dev = pg.cross_covariances(pairs, linear_solver="device", dtype=np.float64)
    for (s_, t_), h, d in zip(pairs, host, dev):
        rel = np.abs(d - h).max() / np.abs(h).max()
        print("CROSS (%d, %d): device - host %.3g of the block's largest entry %.3g" % (s_, t_, rel, np.abs(h).max()))
        assert rel <= 2.0 ** -24  # (tests/test_covariance_gpu.py's tolerance)
    assert all(f == 0 for f in pg.covariance_stats["flags"]) and pg.covariance_stats["systems"] > 0
