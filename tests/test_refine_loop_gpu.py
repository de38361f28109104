"""The loop with refined loop closures (examples/slam_loop.py --lc-refine icp) on the loop tests' bag: the closures' relative
error falls to a fifth of the lattice's or below, and HipBackend.refine_matches equals hostside.refine_matches bit for bit on the
run's own pairs.  err_lc_m is printed, not asserted: what the trajectory gains depends on the solve."""
import numpy as np
import pytest

from nautilus_amd import hostside, posegraph
from tests import loss_loop as LL

pytestmark = pytest.mark.gpu

KW = LL.KW  # the loop tests' bag: 32 scans at 0.06 m, 66 closures pass the score gate


class Recording(posegraph.HipBackend):
    """HipBackend that keeps the arguments and the result of its refine_matches calls."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def refine_matches(self, *args, **kw):
        out = super().refine_matches(*args, **kw)
        self.calls.append((args, kw, out))
        return out


@pytest.fixture(scope="module")
def runs(gpu):
    import examples.slam_loop as loop
    backend = Recording()
    return loop.run(**KW), loop.run(backend=backend, lc_refine="icp", **KW), backend


def test_refined_closures_are_five_times_closer(runs):
    plain, refined, backend = runs
    its = backend.calls[0][2]["iterations"]
    print("lattice:", {k: plain[k] for k in ("lc_accepted", "lc_rel_err_m", "err_lc_m")})
    print("refined:", {k: refined[k] for k in ("lc_accepted", "lc_refined", "lc_refine_flags", "refine_s", "lc_rel_err_m", "err_lc_m")},
          "updates min/median/max", int(its.min()), float(np.median(its)), int(its.max()))
    assert sorted(set(refined) - set(plain)) == ["lc_refine_flags", "lc_refined", "refine_s"]
    assert refined["lc_accepted"] == plain["lc_accepted"] > 0
    assert refined["lc_refined"] + sum(v for k, v in refined["lc_refine_flags"].items() if k != "NOT_CONVERGED") == refined["lc_accepted"]
    assert refined["lc_refined"] > 0
    assert refined["lc_rel_err_m"] <= plain["lc_rel_err_m"] / 5


def test_backend_equals_the_host_route_on_the_runs_pairs(runs):
    _, _, backend = runs
    assert len(backend.calls) == 1
    (xy, nrm, off, src, tgt, theta0, rec, spec, search), kw, out = backend.calls[0]
    assert not kw and len(out) == len(src) > 0
    want = hostside.refine_matches(xy, nrm, off, src, tgt, theta0, rec, spec, search)
    assert out.tobytes() == want.tobytes()


def test_rejected_records_and_pair_origins_through_the_backend(runs):
    """The run's records once more with every pair's window moved by a pair_origin and ix, iy moved back (the same lattice
    poses), and every seventh record rejected: the rejected ones come back SKIPPED with NaNs, the others as in the run, and the
    backend equals the host route."""
    _, _, backend = runs
    (xy, nrm, off, src, tgt, theta0, rec, spec, search), _, out = backend.calls[0]
    rng = np.random.default_rng(11)
    origin = rng.integers(-3, 4, (len(src), 2)).astype(np.int32)
    moved = rec.copy()
    moved["ix"], moved["iy"] = rec["ix"] - origin[:, 0], rec["iy"] - origin[:, 1]
    moved["itheta"][::7] = -1
    got = backend.refine_matches(xy, nrm, off, src, tgt, theta0, moved, spec, search, pair_origin=origin)
    want = hostside.refine_matches(xy, nrm, off, src, tgt, theta0, moved, spec, search, pair_origin=origin)
    assert got.tobytes() == want.tobytes()
    rejected = np.zeros(len(src), bool)
    rejected[::7] = True
    assert np.all(got["flags"][rejected] == hostside.REFINE_SKIPPED) and np.isnan(got["c"][rejected]).all()
    assert not got["n_corr"][rejected].any() and not got["iterations"][rejected].any()
    assert got[~rejected].tobytes() == out[~rejected].tobytes()
