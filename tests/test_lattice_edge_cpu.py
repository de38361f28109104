"""The statement and the inputs of tests/test_lattice_edge_gpu.py hold what they claim (tests/lattice_edge.py), by numpy and
the oracle alone: the valid sub-blocks enumerate exactly the lattice, the counts of the bench's 81 x 81 lattice are the
stated ones, the constants are the headers', and every placed scan has its optimum where its name says -- with larger sums
beyond the lattice's edge where it says so."""
import os
from collections import Counter

import numpy as np
import pytest

from oracle import oracle as O
from tests import lattice_edge as L
from tests import saturated_cases as S

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nautilus_amd", "csrc")
BITS = (8, 16)
SIDES = list(range(1, 18)) + [81, 88]


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_constants_are_the_headers():
    common, bnb, exact = _src("nhip_common.h"), _src("nhip_bnb.hip"), _src("nhip_bnb_exact.h")
    assert "constexpr int BNB_B = %d;" % L.B in common and "constexpr int BNB_B4 = %d;" % L.B4 in common
    assert "constexpr int WHOLE_MIN = %d;" % L.WHOLE_MIN in bnb
    assert "return min(max(n - BNB_B * B, 0), BNB_B);" in exact          # block_extent
    assert "return BNB_B4 * sx < vx && BNB_B4 * sy < vy;" in exact       # sub_valid
    assert L.PAD == ((2 * L.MAX_SHIFT + 16) + 3) & ~3 and L.MAX_SHIFT >= L.half(81)
    assert O.grid_side(O.grid_spec(L.RANGE, L.RES, L.SIGMA, L.FLOOR_P, 16)) == L.SIDE


@pytest.mark.parametrize("nx", SIDES)
def test_valid_sub_blocks_enumerate_exactly_the_lattice(nx):
    for ny in SIDES:
        seen = Counter(L.covered(nx, ny))
        assert set(seen) == {(ix, iy) for ix in range(nx) for iy in range(ny)}, (nx, ny)  # none lost, none added
        assert set(seen.values()) == {1}, (nx, ny)                                         # none twice
        for Y, X, sy, sx, nr, nc in L.valid_sub_blocks(nx, ny):
            assert 1 <= nr <= L.B4 and 1 <= nc <= L.B4
        c = L.counts(nx, ny)
        # a block has 1, 2 or 4 sub-blocks with a pose -- never exactly WHOLE_MIN -- and fewer than WHOLE_MIN as soon as
        # one of its extents is at most 4
        for Y, X, vy, vx in L.blocks(nx, ny):
            n_valid = sum(L.sub_valid(vy, vx, sy, sx) for sy in (0, 1) for sx in (0, 1))
            assert n_valid == (1 + (vx > L.B4)) * (1 + (vy > L.B4)) >= 1
            assert (n_valid >= L.WHOLE_MIN) == (vx > L.B4 and vy > L.B4)
        sat = L.saturated_counts(nx, ny, 1)
        assert 4 * sat["blocks_whole"] + sat["sub_blocks"] == 4 * c["blocks"] - c["without_pose"]
        if nx % L.B <= L.B4 and ny % L.B <= L.B4:
            assert sat["edge_blocks_whole"] == 0, (nx, ny)
        if nx % L.B == 0 and ny % L.B == 0:
            assert c["edge_blocks"] == 0 and c["without_pose"] == 0


def test_counts_of_the_bench_lattice():
    c = L.counts(81, 81)
    assert c == {"blocks": 121, "edge_blocks": 21, "sub_blocks": 484, "without_pose": 43, "valid_edge": 41}
    ext = Counter((nr, nc) for Y, X, sy, sx, nr, nc in L.valid_sub_blocks(81, 81) if X == 10 or Y == 10)
    assert ext == {(4, 1): 20, (1, 4): 20, (1, 1): 1}
    assert L.saturated_counts(9, 9, 1) == {"blocks_whole": 1, "sub_blocks": 5, "candidates_refined": 4, "edge_blocks_refined": 3,
                                           "sub_blocks_without_pose": 0, "edge_blocks_whole": 0, "blocks_total": 4}
    assert L.counts(9, 9)["without_pose"] == 7
    assert L.saturated_counts(8, 8, 3)["edge_blocks_refined"] == 0 and L.saturated_counts(8, 8, 3)["blocks_whole"] == 3


def test_case_list_is_the_stated_one():
    assert {nx % 8 for nx, _ in L.LATTICES} >= {0, 1, 4, 5} and {ny % 8 for _, ny in L.LATTICES} >= {0, 1, 4}
    assert (81, 81) in L.LATTICES and (81, 81, 1) in L.groups() and (81, 81, 3) not in L.groups()
    assert len(L.groups()) == 2 * len(L.LATTICES + L.ODD_NEIGHBOURS) - 1
    assert all(L.admitted(*v) for v in L.ODD_NEIGHBOURS) and [v for v in L.LATTICES if not L.admitted(*v)] == [(4, 4), (5, 4), (8, 8), (12, 9), (13, 16)]
    ext = {L.extent(n, L.n_blocks(n) - 1) for v in L.LATTICES + L.ODD_NEIGHBOURS if L.admitted(*v) for n in v}
    assert ext == {1, 3, 5, 7}
    assert set(L.LENGTHS) >= {1, 63, 64, 65} and max(L.LENGTHS) >= 190
    names = set(L.placements(9, 9, 8))
    assert names >= {"x_last", "y_last", "corner", "x_tie", "x_first", "y_first", "flat"} | {"%s_beyond%d" % (a, d) for a in "xy" for d in (1, 4, 8)}


@pytest.fixture(scope="module")
def images():
    return {(b, t): O.grid_build(L.target(t), O.grid_spec(L.RANGE, L.RES, L.SIGMA, L.FLOOR_P, b)) for b in BITS for t in L.TARGETS}


@pytest.mark.parametrize("bits", BITS)
def test_targets_hold_the_stated_levels(images, bits):
    top, T, TL = S.levels(bits), L.top_column(bits), L.top_column_lo(bits)
    rows = slice(L.CENTRE - 60, L.CENTRE + 60)
    xhi, xlo = images[bits, "xhi"][rows], images[bits, "xlo"][rows]
    assert np.all(xhi[:, T:T + 60] == top) and np.all(xhi[:, T - 1] < top) and np.all(np.diff(xhi[:, T - 10:T + 1].astype(np.int64), axis=1) > 0)
    assert np.all(xlo[:, TL - 60:TL + 1] == top) and np.all(xlo[:, TL + 1] < top)
    assert np.array_equal(images[bits, "yhi"], images[bits, "xhi"].T) and np.array_equal(images[bits, "ylo"], images[bits, "xlo"].T)
    c, TC = images[bits, "corner"], L.top_diagonal(bits)
    assert c[TC, TC] == top and np.count_nonzero(c[:TC + 1, :TC + 1] == top) == 1
    assert L.reach_half(16) == 0 and L.reach_half(8) >= S.reach(8)
    assert np.all(images[bits, "plateau"][60:180, 60:180] == top)


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("lattice", L.LATTICES + L.ODD_NEIGHBOURS, ids=lambda v: "%dx%d" % v)
def test_every_placed_scan_sits_where_it_claims(images, bits, lattice):
    nx, ny = lattice
    hx, hy = L.half(nx), L.half(ny)
    for name, (t, cell, claim) in L.placements(nx, ny, bits).items():
        img = images[bits, t]
        plane = L.volume(img, cell, 1, nx, ny, 1)[0]
        (_, ix, iy), best = S.first_maximum(plane[None])
        assert (ix, iy) == claim and best > 0, (name, lattice, (ix, iy), claim)
        row, col = L.lookup_origin(S.cluster_point(cell), 0, 1, hx, hy)
        assert (row, col) == (cell[1] - hy, cell[0] - hx)
        if "beyond" in name:  # the cells the poses just past the upper edge would read hold MORE than any pose of the lattice
            d = int(name[name.index("beyond") + 6:])
            # (no less in any row or column, and more than the optimum itself in the optimum's)
            if name[0] in "xc":
                past = img[row:row + ny, col + nx:col + nx + d]
                assert np.all(past >= img[row:row + ny, col + nx - 1:col + nx]) and past[iy].min() > best, name
            if name[0] in "yc":
                past = img[row + ny:row + ny + d, col:col + nx]
                assert np.all(past >= img[row + ny - 1:row + ny, col:col + nx]) and past[:, ix].min() > best, name
        if name == "x_tie" and nx > 1:
            assert plane[nx - 2, 0] == plane[nx - 1, 0] == best and plane[max(nx - 3, 0), 0] < best or nx == 2
        if name == "flat":
            assert np.all(plane == S.levels(bits))
    # every rotation's lookups of every source stay inside the image (volume() asserts it)
    for _, t, cell, n in L.sources(nx, ny, bits)[::len(L.LENGTHS)]:
        L.volume(images[bits, t], cell, n, nx, ny, 3)
