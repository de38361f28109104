"""The run list of level-2 entries and the strip bounds over it, in numpy (tests/level2_runs.py): the head rule, the cut at
every 64-point chunk start and the counts; the strip bound over runs equals, integer for integer, the bound over the cells
and over the raw points; and the hand-placed scans of tests/test_bnb_level2_runs_gpu.py sit where they claim -- how many
runs, which totals per group of 8 lanes, which rotations fall back and why."""
import math

import numpy as np
import pytest

from tests import level2_runs as M

LATTICE = 8  # hx = hy of the 17 x 17 lattice the hand-placed scans run at
TINY = 1e-6  # their rotation step: 15 m * 1e-6 is far inside a cell, the three rotations see the same cells


@pytest.fixture(scope="module")
def scan(small_bag):
    return small_bag.scans[3]


@pytest.fixture(scope="module")
def table():
    return np.random.default_rng(5).integers(0, 256, (M.POOL4_ROWS, M.POOL4_PITCH), dtype=np.uint8)


def _rotations(pts, th0=0.0, n_theta=3, step=TINY, h=LATTICE):
    for k in range(n_theta):
        cf, sf = M.rotation(th0, k, n_theta, step)
        yield M.origins(pts, cf, sf, h, h)


def test_head_rule_chunk_cut_and_counts():
    row = np.full(200, 700)
    col = np.r_[np.full(70, 800), np.full(10, 801), np.full(50, 804), np.full(10, 800), np.full(60, 812)]
    r, c, n = M.cell_list(row, col)
    # cells: 800 x 64 | 800 x 6, 801 x 10, 804 x 48 | 804 x 2, 800 x 10, 812 x 52 | 812 x 8   (| = chunk start)
    assert list(zip(c, n)) == [(800, 64), (800, 6), (801, 10), (804, 48), (804, 2), (800, 10), (812, 52), (812, 8)]
    r2, c2, n2 = M.run_list(row, col)
    # entries: 200 x 64 | 200 x 16, 201 x 48 | 201 x 2, 200 x 10 (A, B, A: not merged with the first), 203 x 52 | 203 x 8
    assert list(zip(c2, n2)) == [(200, 64), (200, 16), (201, 48), (201, 2), (200, 10), (203, 52), (203, 8)]
    assert np.all(r2 == 175) and n.sum() == n2.sum() == 200 and n2.max() <= M.CHUNK
    # a change of the row's entry alone is a head too
    assert len(M.run_list(np.r_[700, 701, 703, 704], np.full(4, 800))[2]) == 2
    # entry i sits in lane i % 64: totals per group of 8 lanes
    assert list(M.group_totals(np.r_[np.full(8, 30), np.ones(56, int), np.full(8, 2)])) == [256, 8, 8, 8, 8, 8, 8, 8]


def test_strip_bounds_over_runs_cells_and_points_agree(scan, table):
    sets = [pts for pts, _, _ in M.cases(scan).values()]
    sets += [scan, np.resize(scan, (1081, 2))]
    checked = 0
    for pts in sets:
        rots = list(_rotations(pts)) + list(_rotations(pts, 0.3, 3, math.radians(1.0), 4))
        for row, col in rots[::2]:
            runs, cells = M.run_list(row, col), M.cell_list(row, col)
            ones = np.ones(len(row), np.int64)
            for (Y, X0, length) in ((0, 0, 1), (1, 0, 3), (2, 1, 2), (0, 2, 1)):
                want = M.strip_bound(table, row >> 2, col >> 2, ones, Y, X0, length, 257)
                assert np.array_equal(M.strip_bound(table, cells[0] >> 2, cells[1] >> 2, cells[2], Y, X0, length, 257), want)
                assert np.array_equal(M.strip_bound(table, *runs, Y, X0, length, 257), want)
                if M.status(row, col) == "runs":  # ... and through the 16-bit fields, which the check keeps whole
                    assert np.array_equal(M.strip_bound_packed(table, *runs, Y, X0, length, 257), want)
                checked += 1
    assert checked >= 100


def test_the_field_check_is_needed_and_tight(scan):
    """On a saturated table 257 points per group fill a field to the last bit; 258, or a patch's 512, overflow it."""
    full = np.full((M.POOL4_ROWS, M.POOL4_PITCH), 255, np.uint8)
    C = M.cases(scan)
    for name, exact in (("group257", True), ("group258", False), ("patch", False)):
        row, col = next(_rotations(C[name][0]))
        runs = M.run_list(row, col)
        plain, packed = M.strip_bound(full, *runs, 0, 0, 3), M.strip_bound_packed(full, *runs, 0, 0, 3)
        assert np.array_equal(plain, packed) == exact, name
        assert np.all(plain == 255 * len(row))


def test_hand_placed_scans_sit_where_they_claim(scan):
    C = M.cases(scan)
    assert [len(C["len%d" % n][0]) for n in (1, 63, 64, 65, 1081, 1088)] == [1, 63, 64, 65, 1081, 1088]
    for name, (pts, what, n_runs) in C.items():
        for row, col in _rotations(pts):
            assert M.status(row, col) == what, name
            assert row.min() >= 0 and col.min() >= 0 and max(row.max(), col.max()) < 8192
            if n_runs is not None:
                assert len(M.run_list(row, col)[2]) == n_runs, name
    first = lambda name: next(_rotations(C[name][0]))
    chunks = lambda name: -(-len(M.run_list(*first(name))[2]) // M.CHUNK)
    assert [chunks(n) for n in ("alt64", "alt65", "alt512", "alt513")] == [1, 2, 8, 9]
    assert [chunks("len%d" % n) for n in (1, 65, 1081, 1088)] == [1, 1, 7, 7]  # (386 / 387 runs: the round of 8 chunks)
    assert chunks("len1081") > 6 and chunks("boundary") == 1 and 4 < chunks("alt512") <= 8
    # alternating entries: both parities of col >> 2, i.e. both alignments of the strip load
    r2, c2, n = M.run_list(*first("alt65"))
    assert set(c2 & 1) == {0, 1} and np.all(n == 1) and len(set(zip(r2, c2))) == 2
    # the run that straddles point 64 is cut there; its cell is one
    row, col = first("straddle")
    assert len(set(zip(row[60:70], col[60:70]))) == 1
    heads = np.cumsum(M.run_list(row, col)[2])
    assert 64 in heads and 60 in heads and 70 in heads
    # the patch: one entry, 17 runs of 64 (the last: 57), 512 points in lanes 0..7; its CELL list passes its own check
    row, col = first("patch")
    assert len(set(zip(row >> 2, col >> 2))) == 1 and len(set(zip(row, col))) == 16
    assert list(M.run_list(row, col)[2]) == [64] * 16 + [57]
    assert M.group_totals(M.run_list(row, col)[2]).max() == 512 and M.group_totals(M.cell_list(row, col)[2]).max() <= M.GROUP_LIMIT
    # exactly 257 and 258 points in the first group, and only the run list sees them
    for name, total in (("group257", 257), ("group258", 258)):
        row, col = first(name)
        assert M.group_totals(M.run_list(row, col)[2]).max() == total
        assert M.group_totals(M.cell_list(row, col)[2]).max() < 64
    # same entry, different cells: one run; cells 3 | 4: a run each
    row, col = first("boundary")
    n = M.run_list(row, col)[2]
    assert n[0] == 41 and np.all(n[1:] == 1) and set(col[40:] & 3) == {3, 0} and set(col[:40] & 3) == {0, 1}


def test_ordinary_pairs_take_the_run_path(small_bag):
    """Every rotation of real pairs: no fall-back (the GPU test asserts the counters show the same)."""
    src, _, th0 = small_bag.sample_pairs(per_target=2, targets=[9, 30], min_sep=2)
    n_runs, n_cells = [], []
    for s, t in zip(src[:3], th0[:3]):
        for row, col in _rotations(small_bag.scans[int(s)], float(t), 5, math.radians(1.0), 4):
            assert M.status(row, col) == "runs"
            n_runs.append(len(M.run_list(row, col)[2]))
            n_cells.append(len(M.cell_list(row, col)[2]))
    assert max(n_runs) <= M.RUN_CAPACITY and 2 * np.mean(n_runs) < np.mean(n_cells)
