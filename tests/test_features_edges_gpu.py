"""The scan features at one-ulp threshold edges (tests/threshold_edges.py): the neighbourhood test of phase 1,
`norm <= max_neighbor_distance`, and the suppression of phase 2, `norm < distance_threshold`, both a float norm widened and
compared with a double.  64 thresholds, one launch per spec; compared with the numpy reference as tests/test_features_gpu.py
compares (scores as bit patterns, selections in order)."""
import numpy as np
import pytest

from nautilus_amd import features
from tests import threshold_edges as E
from tests.test_features_gpu import _assert_equal, _extract_dev

pytestmark = pytest.mark.gpu
THRESHOLDS = E.thresholds(64)


def _run(cases, what):
    """cases: (T, inputs, want) per launch.  Every launch is compared; the failures are counted before any is raised."""
    failed = []
    for T, c, want in cases:
        got, _ = _extract_dev(c["xy"], c["off"], features.feature_spec(**c["fields"]))
        try:
            _assert_equal(got, want, c["off"])
        except AssertionError as err:
            failed.append((T, str(err)[:80]))
    print("%s: %d of %d thresholds differ from the reference %s" % (what, len(failed), len(cases), failed[:4]))
    assert not failed


def test_neighbourhood_at_threshold_edges(gpu):
    """Left neighbour k = 0 and k = P - 1 of point i = P and of a later point at the designed offsets."""
    cases, n = [], 0
    for T in THRESHOLDS:
        c, want, n_live = E.feat_phase1_case(T)  # (asserts both roots and 100 % live cases)
        cases.append((T, c, want))
        n += n_live
    assert n > 64 * 16
    _run(cases, "feature neighbourhoods")


@pytest.mark.parametrize("edge", [False, True])
def test_suppression_at_threshold_edges(gpu, edge):
    """An accepted point and a still-eligible point at the designed offsets: a scan LDS holds and one of 2049 points, the
    suppressing point accepted in round 0 and in later rounds (over the thresholds), the planar and the edge walk."""
    cases = []
    first, later = [0, 0], [0, 0]
    for T in THRESHOLDS:
        c, want, rounds = E.feat_phase2_case(T, edge)  # (asserts both roots and 100 % live cases, in both scans)
        assert c["off"][1] <= 2048 and c["off"][2] - c["off"][1] == 2049
        cases.append((T, c, want))
        for s, r in enumerate(rounds):
            first[s] += sum(1 for v in r if v == 0)
            later[s] += sum(1 for v in r if v > 0)
    assert min(first) > 0 and min(later) > 64, (first, later)
    _run(cases, "feature suppression, %s walk" % ("edge" if edge else "planar"))
