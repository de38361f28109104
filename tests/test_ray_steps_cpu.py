"""tests/ray_steps.py holds what it is for (no GPU): the float32 model of the ray's estimate gives the counts the lists were
chosen by, every listed step is off by exactly one with the right cell the references', and -- the mutant check -- each of
the four compared outputs (K14's planes, K15's counts and free plane, K21's signatures) differs from the reference's as soon
as the uncorrected estimate stands in the place of the references' floor division.  The hostside numpy forms are held to the
references on the same cases."""
import numpy as np
import pytest

from nautilus_amd import csm, hostside
from tests import freespace_reference as FR
from tests import occupancy_reference as OR
from tests import rangesig_reference as RR
from tests import ray_steps as S


def errors_of_every_minor(n):
    """(2 n + 1, n) int8: the estimate's error at step k (column) of the beam with minor offset m - n (row)."""
    k = np.arange(n, dtype=np.int64)[None, :]
    out = np.zeros((2 * n + 1, n), np.int8)
    for lo in range(0, 2 * n + 1, 512):
        minor = np.arange(lo, min(lo + 512, 2 * n + 1), dtype=np.int64)[:, None] - n
        out[lo:lo + 512] = S.estimate_rdiv(k * minor, n) - (2 * k * minor + n) // (2 * n)
    return out


# ---------------------------------------------------------------- the model
def test_too_low_steps_start_at_14_and_number_248_up_to_64():
    total, first = 0, None
    for n in range(1, 65):
        d = errors_of_every_minor(n)
        assert d.max() <= 0 and d.min() >= -1
        total += int((d != 0).sum())
        if first is None and d.any():
            first = (n, sorted((int(m) - n, int(k)) for m, k in np.argwhere(d)))
    assert total == 248
    assert first == (14, [(-13, 7), (-7, 7), (-7, 13)])


def test_too_high_steps_start_at_2457():
    assert errors_of_every_minor(2456).max() == 0
    d = errors_of_every_minor(2457)
    assert d.max() == 1 and (2374 + 2457, 2383) in {(int(m), int(k)) for m, k in np.argwhere(d > 0)}
    k, e = S.estimate_error(2457, 2374)
    assert k.tolist() == [2383] and e.tolist() == [1]


@pytest.mark.parametrize("n,off,high", [(4093, 2147, 1665), (4001, 883, 777)])
def test_near_the_top_many_minors_have_an_off_step_and_none_is_two_off(n, off, high):
    d = errors_of_every_minor(n)
    assert int((d != 0).any(axis=1).sum()) == off and int((d > 0).any(axis=1).sum()) == high
    assert d.max() == 1 and d.min() == -1


def test_the_estimate_is_exact_at_4096():
    for minor in (-4096, -4095, -2731, -3, 1, 1000, 2047, 4095, 4096):
        assert not len(S.estimate_error(4096, minor)[0])


# ---------------------------------------------------------------- the lists
@pytest.mark.parametrize("name", ["LOW", "HIGH"])
def test_lists_name_every_off_step_with_the_references_cells(name):
    lst = getattr(S, name)
    for beam, steps in lst:
        n, x_major, major, minor = S.parts(beam)
        assert n != 4096 and steps
        k, d = S.estimate_error(n, minor)
        assert k.tolist() == [s[0] for s in steps] and np.abs(d).max() == 1, beam
        cells, cells_fs = OR.ray_cells(*beam), FR.ray(*beam)
        for (kk, right, est), dd in zip(steps, d.tolist()):
            assert tuple(cells[kk].tolist()) == right == cells_fs[kk], (beam, kk)
            assert est == ((right[0], right[1] + dd) if x_major else (right[0] + dd, right[1])), (beam, kk)
            assert est[0 if x_major else 1] == major * kk
    steps = S.off_steps(lst)
    ns = {S.parts(b)[0] for b, _ in lst}
    forms = {(S.parts(b)[1], S.parts(b)[2], S.parts(b)[3] > 0) for b, _ in lst}
    assert len(forms) == 8  # x- and y-major, both signs of the major step, both signs of the minor offset
    if name == "LOW":
        assert len(steps) == 153 and all(s[4] == -1 for s in steps) and len(ns) == 8
        assert min(ns) == 14 and sum(n <= 64 for n in ns) == 3 and sum(570 <= n <= 640 for n in ns) == 3
    else:
        assert sum(s[4] == 1 for s in steps) == 41 and sum(s[4] == -1 for s in steps) == 1 and len(ns) == 7
        assert min(ns) == 2457 and max(ns) == 4095 and {4093, 4091, 4001, 3001} <= ns
        beams = [b for b, _ in lst]
        assert (2457, 2374) in beams and (4093, -2170) in beams
        for n in (4093, 4091, 4001):
            assert sum(len(st) == 2 for b, st in lst if S.parts(b)[0] == n) >= 2
    assert len(steps) >= 32 and len(ns) >= 6


# ---------------------------------------------------------------- K14
def occupancy_mutant_differs(case, monkeypatch):
    name, packed, spec, walked = case
    want = OR.occupancy(*packed, spec)
    with monkeypatch.context() as m:
        m.setattr(OR, "rdiv", S.estimate_rdiv)
        mutant = OR.occupancy(*packed, spec)
    assert not np.array_equal(mutant[2], want[2]), name  # (misses: the plane the ray writes)
    assert np.array_equal(mutant[1], want[1])
    return walked


def test_occupancy_low_cases_catch_a_missing_correction(monkeypatch):
    cases = S.occupancy_low_cases()
    walked = [occupancy_mutant_differs(c, monkeypatch) for c in cases]
    assert walked[0] == [2 * 153, 0]  # every LOW step, in the beam's own scan and in the scan of all beams
    assert walked[1] == [sum(len(st) for b, st in S.LOW if S.parts(b)[0] <= 112), 0]
    for name, (xy, off, poses), spec, _ in cases:  # the whole rays lie inside the window: no miss is cut off
        got = OR.occupancy(xy, off, poses, spec)
        assert got[3][:5].tolist() == [len(poses), 0, len(xy), 0, 0] and got[1].sum() == len(xy)
    # the scans give the beams they were built for
    name, (xy, off, poses), spec, _ = cases[0]
    for i, (beam, _) in enumerate(S.LOW):
        o, d, _ = OR.beams(xy[off[i]:off[i + 1]], OR.pose_affines(poses)[i], spec)
        assert o.tolist() == [0, 0] and d.tolist() == [list(beam)]


@pytest.mark.parametrize("i", range(len(S.HIGH)))
def test_occupancy_high_cases_catch_a_missing_correction(monkeypatch, i):
    cases = S.occupancy_high_cases(i)
    assert len(cases) == len(S.HIGH[i][1])
    for case in cases:
        name, (xy, off, poses), spec, walked = case
        occupancy_mutant_differs(case, monkeypatch)
        assert sum(walked) >= 2 and 3 <= spec.height <= 8 and spec.width <= 16384 and spec.max_ray_cells == 4096
        in_window = [spec.cell_x0 <= np.floor(p[0] / spec.res) < spec.cell_x0 + spec.width and
                     spec.cell_y0 <= np.floor(p[1] / spec.res) < spec.cell_y0 + spec.height for p in poses]
        assert in_window == [False, False, True]
        o, d, counts = OR.beams(xy[off[1]:off[2]], OR.pose_affines(poses)[1], spec)
        assert d.tolist() == [list(b) for b, _ in S.HIGH] and counts == (len(S.HIGH), 0, 0)
        # the narrowing of k is made at a large (2 ra - 1) n: the window's rows lie far from the origin's
        assert abs(spec.cell_y0) * S.parts(S.HIGH[i][0])[0] > 4000000


def test_occupancy_high_cases_walk_every_listed_step():
    walked = np.sum([c[3] for i in range(len(S.HIGH)) for c in S.occupancy_high_cases(i)], axis=0)
    assert walked[0] >= 2 and walked[1] >= 2 * 41  # each step in its beam's own scan and in the scan of all beams


# ---------------------------------------------------------------- K15: the check
@pytest.mark.parametrize("case", S.check_cases(), ids=lambda c: c["name"])
def test_check_cases_count_the_right_cell_and_not_the_estimates(monkeypatch, case):
    places = set()
    for fs in case["fs"]:
        want = S.check_counts(case, fs)
        assert np.array_equal(S.check_counts(case, fs, hostside.freespace_counts), want)
        with monkeypatch.context() as m:
            m.setattr(FR, "rdiv", S.estimate_rdiv)
            mutant = S.check_counts(case, fs)
        for i, (beam, k, variant, d) in enumerate(case["steps"]):
            place = S.chunk_place(S.parts(beam)[0], k, fs[1])
            assert want[i, 0] == 1 and want[i, 6] == (variant == "right" and place is not None), (beam, k, variant, fs)
            if place is not None:
                assert mutant[i, 6] == 1 - want[i, 6], (beam, k, variant, fs)
                places.add(place)
    if case["name"] == "low":  # one chunk; two, the step in either; groups of four, two and one behind each other
        assert {(1, 0), (2, 0), (2, 1), (4, 0), (4, 3)} <= places
        spans = {(S.parts(b)[0] - 3 + 63) >> 6 for b, _, _, _ in case["steps"]}
        assert 1 in spans and 2 in spans and max(spans) > 3
    else:
        assert {(4, 0), (4, 1), (4, 2), (4, 3)} <= places
    assert all(abs(v) < 2 ** 31 for v in case["origin"].reshape(-1).tolist())


# ---------------------------------------------------------------- K15: the trace
def test_trace_targets_catch_a_missing_correction(monkeypatch):
    sides = []
    for side, reach, targets in S.trace_targets():
        spec = csm.grid_spec(reach, FR.RES, 2.0, 1e-10, 8, 16)
        assert FR.grid_side(spec) == side
        for pts in targets:
            want = FR.free_plane(pts, side, FR.RES)
            assert np.array_equal(hostside._freespace_planes(pts, side, FR.RES)[1], want.astype(bool))
            with monkeypatch.context() as m:
                m.setattr(FR, "rdiv", S.estimate_rdiv)
                assert not np.array_equal(FR.free_plane(pts, side, FR.RES), want)
        sides.append((side, len(targets)))
    assert sides == [(120, 9), (1200, 1)]


def trace_walked(side):
    return sum(len(st) for b, st in S.LOW if S.parts(b)[0] < side // 2)


def test_trace_targets_hold_low_steps_only():
    """no HIGH beam fits a grid whose half side is below 2457"""
    assert trace_walked(120) == 22 and trace_walked(1200) == 153 - 19


# ---------------------------------------------------------------- K21
@pytest.mark.parametrize("pair", range(S.N_MAP_CASES // 2))
def test_map_cases_catch_a_missing_correction(pair):
    right, swapped = S.map_cases()[2 * pair:2 * pair + 2]
    exact = {}
    for name, grid, spec, rays, entries in (right, swapped):
        anchors, sig, stats = RR.anchors_and_signatures(grid, spec, rays)
        assert len(anchors) == 1 and stats[3:6].sum() == 64
        h_anchors, h_sig, h_stats = hostside.range_signatures(grid, spec, rays)
        assert np.array_equal(h_anchors, anchors) and np.array_equal(h_sig, sig) and h_stats.tolist() == stats.tolist()
        anchor = tuple(anchors[0, :2].tolist())
        vals, ends = S.walk(grid, spec, anchor, rays, OR.rdiv)
        assert vals == sig[0].tolist(), name  # (walk() restates the reference: its mutant below is the reference's)
        exact[name] = (vals, ends, S.walk(grid, spec, anchor, rays, S.estimate_rdiv)[0])
    assert len(right[4]) >= 2 and [b for b, _ in right[4]] == [b for b, _ in swapped[4]]
    walled = 0
    for t, ((beam, first), (_, every)) in enumerate(zip(right[4], swapped[4])):
        vals, ends, mutant = exact[right[0]]
        if first:
            assert ends[t] == first[0][0] and vals[t] != mutant[t], (beam, "the walk ends on the off step's wall")
        vals, ends, mutant = exact[swapped[0]]
        if every:
            assert ends[t] > every[-1][0] and vals[t] != mutant[t], (beam, "the walk passes every off step")
        walled += bool(first) + bool(every)
    assert walled >= 2 * len(right[4]) - 4  # (a beam that lies along another one has no cell of its own for a wall)


def map_walked():
    """[low, high] off steps with a wall on one of their two cells, over the maps"""
    n = [0, 0]
    for name, grid, spec, rays, walls in S.map_cases():
        for beam, k, right, est, d in S.off_steps(walls):
            n[d > 0] += 1
    return n


def test_map_cases_walk_high_steps_of_six_lengths():
    assert map_walked()[0] >= 100 and map_walked()[1] >= 2 * 15
    ns = {S.parts(b)[0] for c in S.map_cases() if c[0].startswith("high") for b, _ in c[4]}
    assert len(ns) >= 6
