"""The inputs of tests/test_saturated_gpu.py hold what they claim (tests/saturated_cases.py), by the oracle and numpy alone:
the targets are saturated where stated and near-saturated beside it, every coincident source stays in one cell of the stated
alignment class under every searched rotation, the oracle's score volumes are the closed forms, the corner sources have one
best translation, the cell lists put 256 | 257 | 258 points into one group of 8 lanes, and the longest admitted scans are the
longest whose sums an int32 holds."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import oracle as O
from tests import level2_runs as M
from tests import saturated_cases as S

BITS = (8, 16)


def _ospec(bits):
    return O.grid_spec(S.RANGE, S.RES, S.SIGMA, S.FLOOR_P, bits)


def _osearch(lattice):
    return O.search_spec(*S.LATTICES[lattice])


@pytest.fixture(scope="module")
def images():
    """(bits, target) -> the oracle's table."""
    return {(b, t): O.grid_build(S.target(t, b), _ospec(b)) for b in BITS for t in S.TARGETS}


def test_geometry_is_the_specs():
    assert O.grid_side(_ospec(16)) == S.SIDE and int(np.ceil(3.0 * S.SIGMA)) == S.R
    assert S.PAD == ((2 * S.MAX_SHIFT + 16) + 3) & ~3
    assert [n * x * y for n, x, y, _ in S.LATTICES.values()] == [7 * 625, 5 * 169, 9]
    assert S.reach(16) == 0 and S.reach(8) == 2


@pytest.mark.parametrize("bits", BITS)
def test_plateau_is_saturated_and_a_weaker_one_is_noticed(images, bits):
    lo, hi = S.plateau_square()
    top = S.levels(bits)
    img = images[bits, "plateau"]
    assert hi - lo == S.TOP and np.all(img[lo:hi, lo:hi] == top) and img.max() == top
    # every lookup of every source at every pose of L and S is inside the square
    for lattice in ("L", "S"):
        for s in S.sources().values():
            for row, col in S.rotations(s.points, lattice):
                h = (S.LATTICES[lattice][1] - 1) // 2
                assert min(row.min(), col.min()) - S.PAD >= lo and max(row.max(), col.max()) - S.PAD + 2 * h < hi, (lattice, s.name)
    # a weakened input is noticed.  One hit less takes at most the centre tap's (0.1995^2 =) 4 % from a window: at 16 bits
    # that is 115 levels; at 8 bits log(0.96) is 0.45 steps, which still rounds to 255 -- there the smallest weakening that
    # can be noticed at all is two hits side by side (0.90 steps), and it is.
    pts = S.target("plateau", bits)
    cells = S.target_cells("plateau", bits)
    drop = lambda *c: pts[~np.any([(cells[:, 0] == x) & (cells[:, 1] == y) for x, y in c], axis=0)]
    one = O.grid_build(drop((S.CENTRE, S.CENTRE)), _ospec(bits))[lo:hi, lo:hi]
    two = O.grid_build(drop((S.CENTRE, S.CENTRE), (S.CENTRE + 1, S.CENTRE)), _ospec(bits))[lo:hi, lo:hi]
    assert two.min() < top
    assert (one.min() < top) == (bits == 16)


@pytest.mark.parametrize("bits", BITS)
def test_corner_and_half_hold_top_and_near_top_cells(images, bits):
    top = S.levels(bits)
    margin = 64 * (256 if bits == 16 else 1)
    w = slice(S.CENTRE - S.MAX_SHIFT - 2, S.CENTRE + S.MAX_SHIFT + 2)  # the cells the sources reach on L
    for t in ("corner", "corner_lo", "half"):
        win = images[bits, t][w, w]
        assert np.any(win == top), t
        assert np.any((win >= top - margin) & (win < top)), t
    # the level by the definition's arithmetic (S.level_of) is the oracle's, along the corner's diagonal and its edge
    img = images[bits, "corner"]
    x0 = S.target_cells("corner", bits)[:, 0].min()
    for m in range(S.R + 1):
        assert img[x0 + S.R - m, x0 + S.R - m] == S.level_of(m, m, bits)
        assert img[x0 + S.R, x0 + S.R - m] == S.level_of(m, 0, bits)


def _all_sources():
    return list(S.sources().values()) + [S.long_source(16)]


@pytest.mark.parametrize("lattice", ["L", "S"])
def test_coincident_sources_stay_in_one_cell_of_the_claimed_class(lattice):
    seen = set()
    hx = (S.LATTICES[lattice][1] - 1) // 2
    for s in _all_sources():
        if s.cell is None:
            continue
        for row, col in S.rotations(s.points, lattice):
            assert len(row) == s.n and np.all(row == s.cell[1] - hx + S.PAD) and np.all(col == s.cell[0] - hx + S.PAD), s.name
            assert (int(col[0]) & 3) == S.class_of(s.cell, lattice)
            if lattice == "L":
                assert (int(col[0]) & 3) == s.cls, s.name
        if s.name.startswith("co"):
            seen.add((s.n, S.class_of(s.cell, lattice)))
    assert seen == {(n, j) for n in S.COUNTS for j in range(4)}
    four = S.sources()["four"]
    for row, col in S.rotations(four.points, lattice):
        assert sorted(np.bincount(col & 3)) == [300] * 4 and len(set(row)) == 1
        assert len({int(c) & 3 for c in col[:64]}) == 1  # dealt chunk by chunk
    assert len(np.unique(S.sources()["spread1081"].points, axis=0)) == 1081
    # the staggered clusters: points of the main class added before the last chunk starts, and in all
    for name, before, total in (("stagger191", 191, 255), ("stagger194", 194, 258)):
        s = S.sources()[name]
        for row, col in S.rotations(s.points, lattice):
            main = (col & 3) == (int(col[-1]) & 3)
            assert s.n % 64 == 0 and np.count_nonzero(main[:-64]) == before and np.count_nonzero(main) == total and np.all(main[64:])
            assert len(set(row)) == 1 and len(set(col)) == 2
    # 64 runs of 64 points and two of one, in the pooled entries (8 x 8 cells) the bounds kernel keys its runs by
    s = S.sources()["lanes258"]
    for row, col in S.rotations(s.points, lattice):
        key = (row >> 3) * 4096 + (col >> 3)
        first, cnt = M._lists(key, key)
        assert list(cnt) == [64] * 64 + [1, 1] and key[4096] != key[4095] == key[4097]


def test_longest_8_bit_scan_stays_in_its_cell():
    s = S.long_source(8)
    assert s.n == 8421504
    for row, col in S.rotations(s.points[:4], "T"):  # (the points are one point: four stand for all)
        assert np.all(row == s.cell[1] - 1 + S.PAD) and np.all(col == s.cell[0] - 1 + S.PAD)
    assert np.all(s.points == s.points[0])


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("lattice", ["L", "S"])
def test_oracle_volumes_are_the_closed_forms(images, bits, lattice):
    """n coincident points: n times the volume of one, which is the image around the cell -- for the oracle too.  The oracle
    runs every length on `half` (top level and ramp), and the lengths at the limits on every target."""
    jobs = [(s, t) for s in _all_sources() if s.cell is not None for t in S.TARGETS if t == "half" or s.n in (257, 258, 2049)]
    with ThreadPoolExecutor(8) as pool:  # (the oracle call releases the interpreter lock)
        vols = list(pool.map(lambda j: O.csm_scores(j[0].points, images[bits, j[1]], _ospec(bits), 0.0, _osearch(lattice)), jobs))
    n_done = 0
    for (s, t), vol in zip(jobs, vols):
        want = S.closed_volume(images[bits, t], s.n, s.cell, lattice)
        assert np.array_equal(vol, want), (s.name, t)
        if t == "plateau":
            assert np.all(vol == s.n * S.levels(bits))
        n_done += 1
    assert n_done >= 80
    for name in ("four", "spread1081"):
        s = S.sources()[name]
        vol = O.csm_scores(s.points, images[bits, "plateau"], _ospec(bits), 0.0, _osearch(lattice))
        assert np.all(vol == s.n * S.levels(bits)), name
        m = O.csm_match(s.points, images[bits, "plateau"], _ospec(bits), 0.0, _osearch(lattice))
        assert (m.itheta, m.ix, m.iy, m.sum) == (0, 0, 0, s.n * S.levels(bits))


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("lattice", ["L", "S"])
@pytest.mark.parametrize("name", sorted(S.CORNER_POSE))
def test_corner_sources_have_one_best_translation(images, bits, lattice, name):
    s = S.sources()[name]
    t, org, pose = S.corner_pose(name, lattice)
    n_theta = S.LATTICES[lattice][0]
    vol = O.csm_scores(s.points, images[bits, t], _ospec(bits), 0.0, _osearch(lattice), origin=org)
    assert np.array_equal(vol, S.closed_volume(images[bits, t], s.n, s.cell, lattice, org))
    best = np.argwhere(vol == vol.max())
    assert vol.max() == s.n * S.levels(bits)
    assert [tuple(b) for b in best] == [(k,) + pose[1:] for k in range(n_theta)]  # one translation, at every rotation
    assert S.first_maximum(vol) == (pose, s.n * S.levels(bits))
    m = O.csm_match(s.points, images[bits, t], _ospec(bits), 0.0, _osearch(lattice), origin=org)
    assert (m.itheta, m.ix, m.iy, m.sum) == pose + (s.n * S.levels(bits),)
    # the translations next to it lie on the near-saturated rim (the ramp is 2 R cells wide, the lattice wider: further out
    # the sums fall to zero)
    rest = vol[vol < vol.max()] // s.n
    margin = 64 * (256 if bits == 16 else 1)
    assert np.count_nonzero(rest >= S.levels(bits) - margin) >= 2 * n_theta and rest.max() >= S.levels(bits) - margin // 8
    if lattice == "L":
        assert org == (0, 0)


def test_cell_lists_fill_one_group_to_the_limit():
    for n, status in ((256, "runs"), (257, "runs"), (258, "field")):
        for j in range(4):
            s = S.sources()["co%d@%d" % (n, j)]
            for lattice in ("L", "S"):
                for row, col in S.rotations(s.points, lattice):
                    cnt = M.cell_list(row, col)[2]
                    assert list(cnt) == [64] * 4 + ([n - 256] if n > 256 else [])
                    assert M.group_totals(cnt).max() == n
                    assert M.status(row, col) == status


def test_a_field_holds_257_saturated_cells_and_no_more():
    cell = np.uint16(255)
    with np.errstate(over="ignore"):
        assert np.uint16(257) * cell == 65535 and int(np.uint16(258) * cell) == 258 * 255 - 65536
    full = np.full((M.POOL4_ROWS, M.POOL4_PITCH), 255, np.uint8)
    for n, exact in ((257, True), (258, False)):
        row, col = next(S.rotations(S.sources()["co%d@0" % n].points, "L"))
        runs = M.run_list(row, col)
        plain, packed = M.strip_bound(full, *runs, 0, 0, 3), M.strip_bound_packed(full, *runs, 0, 0, 3)
        assert np.all(plain == 255 * n) and np.array_equal(plain, packed) == exact


def test_longest_admitted_scans():
    assert S.max_pts(16) == 32768 and S.max_pts(8) == 8421504
    for bits in BITS:
        assert S.max_pts(bits) * S.levels(bits) < 2 ** 31 <= (S.max_pts(bits) + 1) * S.levels(bits)
    assert (S.max_pts(16) + 1) * S.levels(16) == 2147516415
    assert S.long_source(16).n == 32768 and S.long_source(16).points.shape == (32768, 2)


def test_every_case_is_live():
    src = S.sources()
    assert len(src) == 4 * len(S.COUNTS) + 7 and len(S.COUNTS) == 20
    g = S.groups()
    assert sorted(g["short"] + g["long"]) == sorted(src) and not set(g["short"]) & set(g["long"])
    assert max(src[k].n for k in g["short"]) == S.SHORT and min(src[k].n for k in g["long"]) == S.SHORT + 1
    for lattice, extra in (("L", 0), ("S", 2)):
        n = sum(len(S.pairs(g[k], lattice)) for k in g)
        assert n == len(src) * len(S.TARGETS) + extra
    assert all(len(s.points) == s.n and s.points.dtype == np.float32 for s in src.values())
