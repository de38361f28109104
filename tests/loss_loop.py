"""The loop (examples/slam_loop.py) under a robust loss with displaced loop-closure records: the runs and the conditions that
tests/test_loss_cpu.py holds on the CPU backend and tests/test_loss_loop_gpu.py on the GPU, with both linear solvers."""
import numpy as np

# the loop tests' 32-scan bag (tests/test_consistency_loop_gpu.py), its 8-bit tables: 66 accepted closures
KW = dict(n_scans=32, window=3, spacing=0.06, hitl=False, gate="geometric", iterations=2, cell_bits=8)
TIMING = ("_s",)  # keys that are wall-clock
SOLVER_COUNTS = ("pcg_by_phase", "pcg_solves", "pcg_iterations", "pcg_not_converged")


def displace_five(hit):
    """tests/test_consistency_loop_gpu.py's rule: five of the accepted records, evenly spread, +2 m in x."""
    def corrupt(src, tgt, rel, good):
        idx = np.nonzero(good)[0][::max(int(good.sum()) // 5, 1)][:5]
        rel[idx, 0] += 2.0
        hit["pairs"] = np.stack([src[idx], tgt[idx]], axis=1).tolist()
        return rel
    return corrupt


def five_runs(backend_factory, **kw):
    """The clean bag and the bag with five displaced records, each without a loss and with Cauchy at scale 1; and the clean
    bag with lc_loss=None spelled out."""
    import examples.slam_loop as loop
    hit = {}
    run = lambda **more: loop.run(backend=backend_factory(), **dict(KW, **dict(kw, **more)))
    out = {"plain": run(), "none": run(lc_loss=None), "clean_cauchy": run(lc_loss="cauchy", lc_loss_scale=1.0),
           "bad": run(_lc_corrupt=displace_five(hit)), "bad_cauchy": run(_lc_corrupt=displace_five(hit), lc_loss="cauchy")}
    out["hit"] = hit["pairs"]
    return out


def check_loop_conditions(runs):
    plain, none, clean, bad, robust, hit = (runs[k] for k in ("plain", "none", "clean_cauchy", "bad", "bad_cauchy", "hit"))
    print("err_lc_m: clean %.5f, clean + cauchy %.5f, 5 displaced %.5f (%.1f x), 5 displaced + cauchy %.5f (%.2f x)" % (
        plain["err_lc_m"], clean["err_lc_m"], bad["err_lc_m"], bad["err_lc_m"] / plain["err_lc_m"], robust["err_lc_m"],
        robust["err_lc_m"] / plain["err_lc_m"]))
    w = {(s, t): v for s, t, v in robust["lc_weights"]}
    print("displaced %s: rho' %s; the others >= %.4f; clean run's smallest weight %.4f" % (
        hit, [w[tuple(p)] for p in hit], min(v for k, v in w.items() if list(k) not in hit), clean["lc_weight_min"]))
    # lc_loss=None is the call without the parameter, and neither reports anything of a loss
    assert set(none) == set(plain) and not [k for k in plain if k.startswith(("lc_loss", "lc_weight", "lc_downweighted"))]
    for k in plain:
        if not k.endswith(TIMING):
            assert none[k] == plain[k], k
    assert len(hit) == 5 and plain["lc_accepted"] == bad["lc_accepted"] == robust["lc_accepted"] >= 20
    assert bad["err_lc_m"] >= 10 * plain["err_lc_m"]
    assert robust["err_lc_m"] <= 2 * plain["err_lc_m"]
    assert all(p in robust["lc_downweighted_pairs"] for p in hit) and all(w[tuple(p)] < 0.05 for p in hit)
    assert all(v > 0.5 for k, v in w.items() if list(k) not in hit)
    assert robust["lc_downweighted"] == 5 and robust["lc_downweighted_rel_err_m"] > 1.0
    assert robust["lc_weight_min"] == min(w.values())
    assert (robust["lc_loss"], robust["lc_loss_scale"]) == ("cauchy", 1.0)
    assert clean["lc_downweighted"] == 0 and clean["lc_downweighted_pairs"] == [] and clean["lc_downweighted_rel_err_m"] is None
    assert abs(clean["err_lc_m"] - plain["err_lc_m"]) <= 0.05 * plain["err_lc_m"]
    for k in plain:  # the loss changes nothing in front of the closure solve
        if not k.endswith(TIMING) and k not in ("err_lc_m",) + SOLVER_COUNTS:
            assert clean[k] == plain[k], k
