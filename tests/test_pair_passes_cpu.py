"""The statement and the inputs of tests/test_pair_passes_gpu.py hold what they claim (tests/pair_passes.py), by numpy and the
oracle alone: the walk over a mask, the strips, the passes of a strip cover every live valid sub-block exactly once, the
saturated prediction of the listed lattices, the constants are the sources', and the three added ties sit where they claim."""
import itertools
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import lattice_edge as L
from tests import pair_passes as M
from tests import saturated_cases as S

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nautilus_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_constants_are_the_sources():
    bnb, host = _src("nhip_bnb.hip"), _src("nhip_bnb_host.hip")
    assert "while (len < %d && X0 + len < NB)" % M.STRIP in bnb
    assert "constexpr int WHOLE_MIN = %d;" % L.WHOLE_MIN in bnb
    assert 'tunable("NHIP_BNB_PAIR_SUBS")' in host and "((int32_t)p.pair_subs << 2)" in host
    # the kernel that works a pair from start to end does not pair; the candidates' kernels do
    assert "rotation_pass<CB, false, false>(" in bnb and bnb.count("rotation_pass<CB, true, true, true>(") == 2
    assert list(M.OFF) == ["NHIP_BNB_PAIR_SUBS"]
    assert "#define NHIP_BNB_PAIR_CROSS %d\n" % M.ACROSS in bnb and "constexpr bool PAIR_CROSS = NHIP_BNB_PAIR_CROSS != 0;" in bnb


def test_walk_pairs_adjacent_bits_from_the_left():
    assert M.walk(0) == (0, 0, 0)
    # with pairs across a block boundary
    assert M.walk(0b1, True) == (0, 0, 1) and M.walk(0b11, True) == (1, 0, 0) and M.walk(0b110, True) == (1, 1, 0)
    assert M.walk(0b111, True) == (1, 0, 1)         # (0, 1) pair up, 2 is left alone
    assert M.walk(0b1110, True) == (1, 1, 1)        # (1, 2) across the boundary, 3 alone
    assert M.walk(0b111111, True) == (3, 0, 0) and M.walk(0b011110, True) == (2, 2, 0) and M.walk(0b101010, True) == (0, 0, 3)
    # inside a block only: bits 2 t and 2 t + 1
    assert M.walk(0b11, False) == (1, 0, 0) and M.walk(0b110, False) == (0, 0, 2) and M.walk(0b1110, False) == (1, 0, 1)
    assert M.walk(0b011110, False) == (1, 0, 2) and M.walk(0b111111, False) == (3, 0, 0)
    for mask in range(64):
        for ab in (False, True):
            p, a, s = M.walk(mask, ab)
            assert 2 * p + s == bin(mask).count("1") and a <= p and (ab or a == 0)
        assert M.walk(mask, False)[0] == sum((mask >> (2 * t)) & 3 == 3 for t in range(3))


def test_strips_are_runs_of_up_to_three_neighbours():
    assert M.strips([]) == [] and M.strips([0, 1, 2, 3]) == [[0, 1, 2], [3]]
    assert M.strips([0, 2, 3, 4, 5, 9, 10]) == [[0], [2, 3, 4], [5], [9, 10]]


@pytest.mark.parametrize("lattice", M.LATTICES + ((5, 5), (7, 13), (23, 7)), ids=lambda v: "%dx%d" % v)
def test_passes_of_a_strip_cover_its_live_sub_blocks_once(lattice):
    """Whatever is alive: 4 per whole block + 2 per pair + 1 per single is the number of live valid sub-blocks, a block goes
    whole exactly from WHOLE_MIN on, and a pair never joins sub-blocks of different sy."""
    nx, ny = lattice
    rng = np.random.default_rng(17)
    for Y in range(L.n_blocks(ny)):
        for xs in M.strips(list(range(L.n_blocks(nx)))):
            for _ in range(40):
                dead = {(X, sy, sx) for X in xs for sy in (0, 1) for sx in (0, 1) if rng.random() < 0.4}
                live = lambda Y_, X, sy, sx: (X, sy, sx) not in dead
                got = M.strip_passes(nx, ny, Y, xs, live)
                per_block = [sum(L.sub_valid(L.extent(ny, Y), L.extent(nx, X), sy, sx) and live(Y, X, sy, sx) for sy in (0, 1) for sx in (0, 1)) for X in xs]
                assert got["whole"] == sum(v >= L.WHOLE_MIN for v in per_block)
                assert 2 * got["pairs"] + got["singles"] == sum(v for v in per_block if v < L.WHOLE_MIN)
                assert got["across"] <= got["pairs"]


def test_saturated_prediction_of_the_listed_lattices():
    want = {(9, 9): (1, 0), (13, 9): (1, 0), (17, 3): (2, 0), (21, 3): (2, 0), (19, 5): (0, 0), (81, 81): (10, 0)}
    for (nx, ny), (pairs, across) in want.items():
        for form in M.PAIRING_FORMS:
            got = M.saturated_pairs(nx, ny, 1, form)
            assert (got["pair_passes"], got["pair_passes_across_blocks"]) == (pairs, across), (nx, ny, form, got)
            assert M.saturated_pairs(nx, ny, 3, form)["pair_passes"] == 3 * pairs
            assert got["passes"] == L.saturated_counts(nx, ny, 1)["sub_blocks"] - pairs
            assert M.saturated_pairs(nx, ny, 1, form, switch=False)["pair_passes"] == 0
        assert M.saturated_pairs(nx, ny, 1, "fused")["pair_passes"] == 0
    # (9, 9): the edge-row blocks hold one pose row; block (1, 0)'s two sub-blocks are the pair, block (1, 1) is the seed
    assert M.strip_passes(9, 9, 1, [0]) == {"whole": 0, "pairs": 1, "across": 0, "singles": 0}
    # a pair across a boundary needs a left neighbour that is dead: sub-block (0, 0) of the strip's first block
    dead = lambda Y, X, sy, sx: (X, sx) != (0, 0)
    assert M.strip_passes(17, 3, 0, [0, 1, 2], dead, True) == {"whole": 0, "pairs": 2, "across": 2, "singles": 0}
    assert M.strip_passes(17, 3, 0, [0, 1, 2], dead, False) == {"whole": 0, "pairs": 1, "across": 0, "singles": 2}
    # (19, 5): with block 1 not whole, its right sub-block and block 2's left one reach one column past nx = 19
    got = M.strip_passes(19, 5, 0, [1, 2], lambda Y, X, sy, sx: (X, sx) != (1, 0), True)
    assert got["across"] == 2 and 8 * 1 + 4 + 8 == 19 + 1


def test_case_list_is_the_stated_one():
    assert M.LATTICES == ((9, 9), (13, 9), (17, 3), (21, 3), (19, 5), (81, 81)) and all(L.admitted(*v) for v in M.LATTICES)
    assert (81, 81, 1) in M.groups() and (81, 81, 3) not in M.groups() and len(M.groups()) == 2 * len(M.LATTICES) - 1
    assert M.LENGTHS == (1, 63, 64, 65, 129, 193) and M.TARGETS == ("plateau", "xhi", "yhi", "corner", "xlo", "ylo")
    assert {t for t, _, _ in M.placements(9, 9, 8).values()} == set(M.TARGETS)
    assert set(M.placements(9, 9, 8)) == set(L.placements(9, 9, 8)) | {"tie_halves", "tie_rows", "tie_pair_single"}
    names = set(M.variants())
    assert names == {f + i + o for f, i, o in itertools.product(M.FORMS, ("", "_instr"), ("", "_off"))}
    assert all(("NHIP_BNB_PAIR_SUBS" in e) == v.endswith("_off") for v, e in M.variants().items())


@pytest.fixture(scope="module")
def images():
    return {(b, t): O.grid_build(L.target(t), O.grid_spec(L.RANGE, L.RES, L.SIGMA, L.FLOOR_P, b)) for b in (8, 16) for t in ("xhi", "yhi")}


@pytest.mark.parametrize("bits", (8, 16))
@pytest.mark.parametrize("lattice", M.LATTICES, ids=lambda v: "%dx%d" % v)
def test_the_ties_sit_where_they_claim(images, bits, lattice):
    nx, ny = lattice
    p = M.placements(nx, ny, bits)
    top = S.levels(bits)
    for name in ("tie_halves", "tie_rows", "tie_pair_single"):
        t, cell, claim = p[name]
        plane = L.volume(images[bits, t], cell, 1, nx, ny, 1)[0]   # [ix, iy]
        (_, ix, iy), best = S.first_maximum(plane[None])
        assert (ix, iy) == claim and best == top, (name, lattice, (ix, iy), claim)
        tied = np.argwhere(plane == best)
        if name == "tie_rows":
            assert {int(v) for v in tied[:, 1]} == set(range(claim[1], ny)) and np.all(plane[:, :claim[1]] < best)
            assert ny - claim[1] >= 2          # at least two rows of one half
        else:
            assert {int(v) for v in tied[:, 0]} == set(range(claim[0], nx)) and np.all(plane[:claim[0]] < best)
    # the halves of a pair: columns 2, 3 and 4 ..; a pair and a single: the last full block's columns and the edge block's
    assert p["tie_halves"][2][0] == 2 and nx > 4
    if nx % L.B == 1:
        X = nx // L.B
        got = M.strip_passes(nx, ny, 0, [X - 1, X], lambda Y, X_, sy, sx: sy == 0 and (X_, sx) != (X - 1, 0))
        assert got["singles"] + got["pairs"] >= 1 and p["tie_pair_single"][2][0] == nx - 4 == L.B * (X - 1) + 5
    for _, t, cell, n in M.sources(nx, ny, bits)[::len(M.LENGTHS)]:
        if t in ("xhi", "yhi"):
            L.volume(images[bits, t], cell, n, nx, ny, 3)   # (every rotation's lookups stay inside the image)
