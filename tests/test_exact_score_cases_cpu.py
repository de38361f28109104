"""The inputs of tests/test_exact_score_edges_gpu.py sit where they claim, and the definition they are held against is the
oracle's (tests/exact_score_cases.py): no GPU.

Every pair of every list at every blur radius is scored twice on the CPU -- the numpy definition with a longdouble mean, and
oracle.pose_score_exact -- at the forced pose or, for the lists that are searched, at the pose the oracle's search on
quantised cells returns.  From that table: the two agree as float32 everywhere; K is re-measured by the project's rule; the
share of cases whose interval [lo, hi] holds more than one float is under 1 %; and every category the GPU test relies on is
present (all 32 window shifts per radius, the rim and the corners, V = K^2, the empty window, both sides of the floor, of each
grid edge and of 1e9, the tie rule at multiples of res, distinct scores per list of pairs)."""
import functools

import numpy as np
import pytest

from tests import exact_score_cases as X
from tests import resid_reference as RR

LD = X.LD


@functools.lru_cache(maxsize=None)
def table(sigma):
    """One row per pair of every list: (list, pair, n points, pose, definition, oracle's double)."""
    rows = []
    for name, L in X.lists(sigma).items():
        for i in range(len(L.src)):
            pose = (0, 0, 0) if L.forced else X.oracle_pose(L, i)[0]
            rows.append((name, i, int(L.n_points[i]), pose, X.reference(L, i, pose), X.oracle_score(L, i, pose)))
    return rows


@pytest.mark.parametrize("sigma", X.SIGMAS)
def test_definition_and_oracle_agree_as_float(sigma):
    rows = table(sigma)
    assert len(rows) > 800
    bad = [(r[0], r[1]) for r in rows if np.float32(r[4]) != np.float32(r[5])]
    assert not bad, bad[:10]
    # ... and the oracle's double lies inside the interval's double bounds everywhere (K as written)
    for name, i, n, _, ref, orc in rows:
        assert abs(LD(orc) - ref) <= abs(ref) * LD((X.K_EXACT + n) * X.U), (name, i)


def test_k_is_what_the_cpu_measures():
    one, many, worst_n = 0.0, -np.inf, 0.0
    for sigma in X.SIGMAS:
        for name, i, n, _, ref, orc in table(sigma):
            if ref == 0:
                assert orc == 0.0
                continue
            ratio = float(abs(LD(orc) - ref) / (abs(ref) * LD(X.U)))
            if n <= 1:
                one = max(one, ratio)
            else:
                many, worst_n = max(many, ratio - n), max(worst_n, ratio)
    K = RR.k_rule(max(one, many))
    print("worst one-point ratio %.3f, worst (ratio - n) %.3f (worst n-point ratio %.1f): K = %d" % (one, many, worst_n, K))
    assert K <= X.K_EXACT


def test_boundary_cases_are_rare():
    n_all = n_wide = 0
    for sigma in X.SIGMAS:
        for name, i, n, _, ref, _ in table(sigma):
            lo, hi = X.interval(ref, n)
            assert lo <= hi and np.float32(ref) in (lo, hi)
            n_all += 1
            n_wide += lo != hi
    print("%d of %d intervals hold more than one float" % (n_wide, n_all))
    assert n_wide < 0.01 * n_all


@pytest.mark.parametrize("sigma", X.SIGMAS)
def test_probes_reach_every_window(sigma):
    R, S = X.radius(sigma), X.SIDE
    P = X.lists(sigma)["probes"]
    K2 = int(X.taps(sigma).sum()) ** 2
    V = X.blur(sigma)[P.cells[:, 1], P.cells[:, 0]]
    tags = np.array(P.tags)
    # the probe is the cell it claims: one point, the identity, the origin
    for i in range(len(P.src)):
        col, row, ok = X.lookup_cells(P.scans[i], *X.rotation(0.0, 0, 1, X.DEG), X.pose_shift(P, i, (0, 0, 0)))
        assert ok[0] and (col[0], row[0]) == tuple(P.cells[i])
    assert sorted(set(X.window_shifts(P).tolist())) == list(range(32))
    # three rows of 32 consecutive columns each, with windows that differ from column to column
    assert (tags == "shift").sum() == 96 and len(set(V[tags == "shift"].tolist())) > 48
    cells = set(map(tuple, P.cells.tolist()))
    assert {(0, 0), (S - 1, 0), (0, S - 1), (S - 1, S - 1)} <= cells
    for e in (0, S - 1):
        assert sum(c == e for c, _ in cells) >= 72 and sum(r == e for _, r in cells) >= 72
    # windows that hang into the zero border on every side, over hits: non-zero sums on all four rims and in all corners
    H = np.zeros((S, S), bool)
    H[X.target_cells(R)[:, 1], X.target_cells(R)[:, 0]] = True
    assert H[0, 0] and H[0, S - 1] and H[S - 1, 0] and H[S - 1, S - 1]
    rim = tags == "rim"
    for axis, e in ((0, 0), (0, S - 1), (1, 0), (1, S - 1)):
        assert (V[rim & (P.cells[:, axis] == e)] > 0).sum() >= 8
    for corner in ((0, 0), (S - 1, 0), (0, S - 1), (S - 1, S - 1)):
        assert X.blur(sigma)[corner[1], corner[0]] > 0
    assert (V[tags == "block"] == K2).sum() >= 1 and (V[tags == "block"] < K2).sum() >= 1
    assert X.reference(P, int(np.nonzero((tags == "block") & (V == K2))[0][0])) == 0
    assert np.all(V[tags == "empty"] == 0)
    assert np.float32(X.reference(P, int(np.nonzero(tags == "empty")[0][0]))) == np.float32(np.log(X.FLOOR_P))
    # every value of the origin's range, the lattice's rim |o| == max_shift included
    assert set(P.origin[:, 0].tolist()) == set(P.origin[:, 1].tolist()) == set(range(-X.MAX_SHIFT, X.MAX_SHIFT + 1))
    # both sides of the floor, with hits in the window on the clamped side too
    F = X.lists(sigma)["floor"]
    a, b = F.between
    VF = X.blur(sigma)[F.cells[:, 1], F.cells[:, 0]]
    assert a / K2 < F.floor_p < b / K2 and a in VF and b in VF
    assert ((VF > 0) & (VF / K2 < F.floor_p)).sum() >= 8 and (VF / K2 > F.floor_p).sum() >= 8
    ia, ib = int(np.nonzero(VF == a)[0][0]), int(np.nonzero(VF == b)[0][0])
    assert np.float32(X.reference(F, ia)) == np.float32(np.log(F.floor_p)) < np.float32(X.reference(F, ib))


@pytest.mark.parametrize("sigma", X.SIGMAS)
def test_edges_lie_on_both_sides(sigma):
    E = X.lists(sigma)["edges"]
    S = X.SIDE
    tags = np.array(E.tags)
    cf, sf = X.rotation(0.0, 0, 1, X.DEG)
    assert (cf, sf) == (1.0, 0.0)
    rows = []
    for i in range(len(E.src) - 1):
        p = E.scans[i]
        col, row, ok = X.lookup_cells(p, cf, sf, X.pose_shift(E, i, (0, 0, 0)))
        with np.errstate(invalid="ignore"):
            sane = bool(np.all(np.abs(p) < np.float32(1e9)))
        rows.append((int(col[0]), int(row[0]), bool(ok[0]), sane))
    col, row, ok, sane = map(np.array, zip(*rows))
    t = tags[:-1]
    assert not ok[t == "not_finite"].any() and not sane[t == "not_finite"].any()
    assert not sane[t == "at_1e9"].any() and sane[t == "below_1e9"].all() and not ok[t == "below_1e9"].any()
    assert (t == "at_1e9").sum() == (t == "below_1e9").sum() == 4
    # the rim: cells -1 | 0 and S - 1 | S on both axes, out and in
    for axis in (col, row):
        for edge_out, edge_in in ((-1, 0), (S, S - 1)):
            assert ((t == "rim") & (axis == edge_out) & ~ok).sum() >= 1 and ((t == "rim") & (axis == edge_in) & ok).sum() >= 1
    # multiples of res: float32(k res) lies in cell k or, rounded down, in cell k - 1 -- both happen
    k = np.repeat(np.arange(-(S // 2), S // 2 + 1), 2)
    m = t == "multiple"
    along = np.where(np.arange(m.sum()) % 2 == 0, col[m], row[m]) - S // 2
    assert np.all((along == k) | (along == k - 1)) and (along == k).sum() >= 10 and (along == k - 1).sum() >= 10
    # and the looked-up cells hold different sums: a wrong cell shows
    V = X.blur(sigma)
    seen = V[row[m & ok], col[m & ok]]
    assert len(set(seen.tolist())) > 30
    assert len(E.scans[-1]) == sum(1 for o in E.origin[:-1] if tuple(o) == (0, 0)) > 250


@pytest.mark.parametrize("sigma", X.SIGMAS)
def test_lists_of_pairs_have_distinct_scores_and_counts_move(sigma):
    by = {}
    for name, i, n, pose, ref, _ in table(sigma):
        by.setdefault(name, []).append((n, pose, np.float32(ref)))
    for n in X.PAIR_LISTS:
        sc = [r[2] for r in by["pairs%d" % n]]
        assert len(sc) == n == len(set(sc)), (n, sc)
        assert all(np.isfinite(s) and s > np.float32(np.log(X.FLOOR_P)) for s in sc)
    for j in (0, 1):
        rows = by["counts%d" % j]
        assert [r[0] for r in rows] == list(X.COUNTS)
        assert by["counts%d_short" % j] == rows[:-1]
        poses = {r[1] for r in rows if r[0] >= 63}
        assert len({p[0] for p in poses}) >= 2 and len({p[1] for p in poses}) >= 2 and len({p[2] for p in poses}) >= 2, poses
        assert all(r[2] > np.float32(np.log(X.FLOOR_P)) for r in rows if r[0] >= 63)
    assert all(r[2] > np.float32(np.log(X.FLOOR_P)) for r in by["shift_ok"])
    L = X.lists(sigma)
    assert np.all(np.abs(L["shift_ok"].origin).max(axis=1) + 1 == X.MAX_SHIFT)
    assert np.all(np.abs(L["shift_beyond"].origin).max(axis=1) + 1 == X.MAX_SHIFT + 1)
    assert not L["counts0"].short and L["counts0_short"].short and all(L[k].short for k in L if not k.startswith("counts"))


def test_radii_are_the_three_instantiations():
    assert [X.radius(s) for s in X.SIGMAS] == [2, 3, 6, 8, 15] and X.radius(5.3) == 16
