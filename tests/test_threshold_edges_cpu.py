"""The designed threshold-edge cases (tests/threshold_edges.py), checked on the CPU: the generator finds both critical roots
and every d2 value between them at each of the 128 thresholds, and every case it designs for a gate is LIVE -- the gate's
CPU oracle decides it differently when the threshold moves one float32 step across the case's root.  A case that is not
live would test nothing on the device; none is tolerated."""
import numpy as np
import pytest

from tests import threshold_edges as E

THRESHOLDS = E.thresholds()
SITES = [("<", "f32"), ("<", "f64"), ("<=", "f64")]  # corr / pair gate; feature suppression; feature neighbourhood


def test_threshold_list():
    assert len(THRESHOLDS) == 128 == len(set(THRESHOLDS)) and THRESHOLDS[:8] == E.NAMED and THRESHOLDS[8:11] == [0.125, 0.25 / 3, 0.0625]
    assert min(THRESHOLDS) >= 0.01 and max(THRESHOLDS) <= 10.0 and E.thresholds(64) == THRESHOLDS[:64]


@pytest.mark.parametrize("op,kind", SITES)
def test_generator_reaches_both_roots_and_every_d2(op, kind):
    n_d2 = []
    for T in THRESHOLDS:
        e = E.Edge(T, op, kind).check(min_d2=3)
        # lo is the last root that passes the site's comparison, hi the first that does not
        assert E.passes(e.lo, T, op, kind) and not E.passes(e.hi, T, op, kind) and e.hi == np.nextafter(e.lo, np.float32(np.inf))
        # the thresholds moved across each root, in the site's own threshold type
        assert not E.passes(e.lo, e.T_down, op, kind) and E.passes(e.hi, e.T_up, op, kind) and not E.passes(np.nextafter(e.hi, np.float32(np.inf)), e.T_up, op, kind)
        # the d2 values are exactly the floats whose correctly rounded root (computed in double) is lo or hi
        r = np.sqrt(e.d2.astype(np.float64)).astype(np.float32)
        assert np.array_equal(r, e.d2_root) and np.all(np.diff(e.d2) > 0)
        below, above = np.nextafter(e.d2[0], np.float32(0)), np.nextafter(e.d2[-1], np.float32(np.inf))
        assert np.sqrt(np.float64(below)).astype(np.float32) < e.lo and np.sqrt(np.float64(above)).astype(np.float32) > e.hi
        assert np.all(np.diff(e.d2.view(np.uint32)) == 1)
        # ... and the offsets reach every one of them
        assert np.array_equal(np.unique(e.off_d2), e.d2)
        n_d2.append(len(e.d2))
    print("distinct d2 per threshold: %d..%d" % (min(n_d2), max(n_d2)))
    assert min(n_d2) >= 3


def test_lattice_offsets_survive_the_subtraction():
    """On the lattice the offset a kernel sees, fl(fl(q + o) - q), is the designed offset bit for bit."""
    for T in THRESHOLDS:
        S, Q = E.lattice_step(T)
        assert S >= 4 * T and S < 8 * T
        e = E.Edge(T, "<", "f32", quantum=Q).check()
        q = E.lattice(289, S)
        o = e.offsets[np.arange(289) % len(e.offsets)]
        assert np.array_equal(((q + o).astype(np.float32) - q).astype(np.float32), o)
        assert np.all(np.linalg.norm(q[:, None, :].astype(np.float64) - q[None, :, :], axis=2)[~np.eye(289, dtype=bool)] >= 4 * T)


@pytest.mark.parametrize("gated", [False, True])
def test_correspondence_cases_are_live(gated):
    n = sum(E.corr_case(T, gated)[2] for T in THRESHOLDS)
    assert n > 128 * 4 * 12


def test_pair_gate_cases_are_live():
    n = sum(E.pair_gate_case(T)[2] for T in THRESHOLDS)
    assert n > 128 * 12


def test_feature_neighbourhood_cases_are_live():
    n = sum(E.feat_phase1_case(T)[2] for T in THRESHOLDS[:64])
    assert n > 64 * 16


@pytest.mark.parametrize("edge", [False, True])
def test_feature_suppression_cases_are_live(edge):
    """... and over the thresholds the suppressing point is accepted in round 0 and in later rounds, in both scans."""
    first, later = [0, 0], [0, 0]
    for T in THRESHOLDS[:64]:
        for s, rounds in enumerate(E.feat_phase2_case(T, edge)[2]):
            first[s] += sum(1 for r in rounds if r == 0)
            later[s] += sum(1 for r in rounds if r > 0)
    assert min(first) > 0 and min(later) > 64, (first, later)
