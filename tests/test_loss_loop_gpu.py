"""The loop under a robust loss on the GPU (examples/slam_loop.py, --lc-loss): the conditions of tests/test_loss_cpu.py on
HipBackend with both linear solvers, and the same down-weighted records as the CPU backend."""
import pytest

from nautilus_amd import posegraph
from tests import loss_loop as LL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip_runs(gpu):
    return {solver: LL.five_runs(posegraph.HipBackend, linear_solver=solver) for solver in ("host", "device")}


@pytest.mark.parametrize("solver", ["host", "device"])
def test_the_loss_gives_back_what_displaced_closures_cost(hip_runs, solver):
    runs = hip_runs[solver]
    LL.check_loop_conditions(runs)
    assert runs["bad_cauchy"]["linear_solver"] == solver
    if solver == "device":
        assert runs["bad_cauchy"]["pcg_solves"] > 0 and runs["bad_cauchy"]["pcg_not_converged"] == 0


def test_hip_and_oracle_agree_on_the_downweighted_records(hip_runs):
    import examples.slam_loop as loop
    from oracle.cpu_backend import OracleBackend
    hit = {}
    cpu = loop.run(backend=OracleBackend(), _lc_corrupt=LL.displace_five(hit), lc_loss="cauchy", **LL.KW)
    for solver, runs in hip_runs.items():
        got = runs["bad_cauchy"]
        assert runs["hit"] == hit["pairs"]
        assert sorted(got["lc_downweighted_pairs"]) == sorted(cpu["lc_downweighted_pairs"]), solver
        assert got["lc_accepted"] == cpu["lc_accepted"] and got["lc_downweighted"] == cpu["lc_downweighted"] == 5
