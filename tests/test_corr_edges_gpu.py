"""The correspondence search at one-ulp threshold edges: sources on an exact lattice at identity poses, one designed target
each whose distance is the last float that passes `dist < outlier_threshold` or the first that does not
(tests/threshold_edges.py; liveness against the oracle in tests/test_threshold_edges_cpu.py and again here), on the hashed
walk, the exhaustive walk and with more than one round per lane, without and with the normal gate (where a nearer decoy
with a failing normal leaves the decision to the gate inside the walks).  128 thresholds, rows compared as bytes."""
import numpy as np
import pytest

from tests import threshold_edges as E

THRESHOLDS = E.thresholds()


@pytest.mark.gpu
@pytest.mark.parametrize("gated", [False, True])
def test_corr_search_at_threshold_edges(gpu, gated):
    from nautilus_amd.correspondence import IcpBatch
    n_cases = n_flipped = 0
    failed = []
    for T in THRESHOLDS:
        c, (want, counts, cap), n_live = E.corr_case(T, gated)  # (asserts both roots in every block and 100 % live cases)
        batch = IcpBatch(c["xy"], c["nrm"], c["off"], c["bs"], c["bt"], outlier_threshold=T, min_abs_cosine=c["min_cos"] if gated else None)
        batch.set_poses(c["poses"])
        n = batch.search()
        rows, boff = batch.correspondences()
        kept = E.corr_kept(c, rows, np.diff(boff), boff[:-1])
        flipped = sum(int((k != lo).sum()) for k, lo in zip(kept, c["is_lo"]))
        n_cases += n_live
        n_flipped += flipped
        same = np.array_equal(np.diff(boff), counts) and n == counts.sum() and all(
            rows[boff[b]:boff[b + 1]].tobytes() == want[cap[b]:cap[b] + counts[b]].tobytes() for b in range(len(c["bs"])))
        if not same:
            failed.append((T, flipped))
    print("%s search: %d of %d designed cases decided differently from the oracle, at %d of %d thresholds %s" % (
        "gated" if gated else "plain", n_flipped, n_cases, len(failed), len(THRESHOLDS), failed[:8]))
    assert n_cases > 128 * 4 * 12 and not failed
