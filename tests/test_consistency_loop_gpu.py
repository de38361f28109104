"""The consistency filter inside HipBackend and the example loop ("Loop-closure consistency"): --lc-consistency
keeps the same records on the device as through the numpy host path, what it keeps and what it drops sum to the unfiltered run's
accepted records, and accepted records displaced by 2 m are all dropped."""
import numpy as np
import pytest

from nautilus_amd import consistency, posegraph

pytestmark = pytest.mark.gpu

KW = dict(n_scans=32, window=3, spacing=0.06, hitl=False, gate="geometric", iterations=2)  # (the other loop tests' bag)


class NoConsistentSet(posegraph.HipBackend):
    """The product's backend with consistent_set() hidden: the loop takes hostside.consistent_set."""
    @property
    def consistent_set(self):
        raise AttributeError("consistent_set")


def test_the_loop_keeps_on_the_device_what_the_host_path_keeps(gpu):
    import examples.slam_loop as loop
    assert not hasattr(NoConsistentSet(), "consistent_set") and hasattr(posegraph.HipBackend(), "consistent_set")
    off = loop.run(**KW)
    assert "lc_consistency" not in off and "consistency_s" not in off
    dev = loop.run(lc_consistency=True, **KW)
    host = loop.run(backend=NoConsistentSet(), lc_consistency=True, **KW)
    print("accepted %d; device: %d consistent, %d inconsistent, err_lc %.17g; host path: %d, %d, err_lc %.17g" % (
        off["lc_accepted"], dev["lc_consistent"], dev["lc_inconsistent"], dev["err_lc_m"], host["lc_consistent"],
        host["lc_inconsistent"], host["err_lc_m"]))
    assert dev["backend"] == host["backend"] == "hip" and dev["lc_consistency"] is True and dev["consistency_s"] > 0
    assert dev["lc_consistent_pairs"] == host["lc_consistent_pairs"] and dev["lc_inconsistent_pairs"] == host["lc_inconsistent_pairs"]
    assert dev["err_lc_m"] == host["err_lc_m"]
    assert dev["lc_consistent"] + dev["lc_inconsistent"] == off["lc_accepted"] > 0
    assert dev["lc_accepted"] == dev["lc_consistent"] == len(dev["lc_consistent_pairs"]) > 0
    # a set smaller than lc_min_set is not trusted: nothing is kept
    none = loop.run(lc_consistency=True, lc_min_set=10 ** 6, **KW)
    assert none["lc_consistent"] == 0 and none["lc_inconsistent"] == off["lc_accepted"] and none["lc_accepted"] == 0
    with pytest.raises(ValueError):
        loop.run(lc_consistency=True, world=2, **KW)


def test_displaced_records_are_dropped(gpu):
    import examples.slam_loop as loop
    hit = {}

    def corrupt(src, tgt, rel, good):
        idx = np.nonzero(good)[0][::max(int(good.sum()) // 5, 1)][:5]
        rel[idx, 0] += 2.0
        hit["pairs"] = np.stack([src[idx], tgt[idx]], axis=1).tolist()
        return rel
    out = loop.run(lc_consistency=True, _lc_corrupt=corrupt, **KW)
    print("displaced %s; inconsistent %s; rel err of the dropped %.3f m" % (hit["pairs"], out["lc_inconsistent_pairs"],
                                                                            out["lc_inconsistent_rel_err_m"]))
    assert len(hit["pairs"]) == 5
    assert all(p in out["lc_inconsistent_pairs"] for p in hit["pairs"])
    assert not any(p in out["lc_consistent_pairs"] for p in hit["pairs"])
    assert out["lc_inconsistent_rel_err_m"] > 1.0 > out["lc_rel_err_m"]
    host = loop.run(backend=NoConsistentSet(), lc_consistency=True, _lc_corrupt=corrupt, **KW)  # (a set that is not everything)
    assert host["lc_consistent_pairs"] == out["lc_consistent_pairs"] and host["lc_inconsistent_pairs"] == out["lc_inconsistent_pairs"]
    assert host["err_lc_m"] == out["err_lc_m"]
    # the backend's method is the host-memory form on prepared records
    poses = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [2.0, 0.0, 0.0], [2.0, 1.0, 0.0]])
    src, tgt = np.array([2, 3, 3]), np.array([0, 0, 1])
    rel = np.array([[2.0, 0.0, 0.0], [2.0, 1.0, 0.0], [9.0, 1.0, 0.0]])
    members, n, stats = posegraph.HipBackend().consistent_set(poses, src, tgt, rel)
    assert n == 2 and members.tolist() == [0, 1, -1] and consistency.keep(members, n, 3, 2).tolist() == [True, True, False]
    assert dict(zip(consistency.STATS_FIELDS, stats.tolist()))["edges"] == 1
