"""Preconditions of the drop-in call's seam tests (tests/test_dropin_seams_gpu.py), without a GPU: every input of
tests/dropin_seams.py is the case it claims to be -- the oracle's two-level search puts the coarse optimum where the family
designed it, the restated plan gives the flow the family is named for, and the constants the restatement uses are the
library's.  An edit of the inputs that stops exercising a seam fails HERE, not silently on the device.  A precondition that
fails means the input is wrong.  (nhip_dropin.hip, nhip_csm_plan.hip.)"""
import math
import os
import time

import numpy as np
import pytest

from tests import dropin_seams as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CLOCK = {}


@pytest.fixture(autouse=True, scope="module")
def _started():
    _CLOCK["t0"] = time.perf_counter()          # when the first test of this file began


def _src(name):
    with open(os.path.join(ROOT, "nautilus_amd", "csrc", name)) as f:
        return f.read()


def test_the_library_constants_are_the_ones_the_flows_were_restated_from():
    dropin, small, params = _src("nhip_dropin.hip"), _src("nhip_csm_small.hip"), _src("nhip_bnb_params.h")
    for line in ("constexpr int DROPIN_CHAIN_ROT_MAX = %d;" % S.CHAIN_ROT_MAX, "constexpr int DROPIN_PARTS_MAX = %d;" % S.PARTS_MAX,
                 "(2 * h1 + 1) <= %d ? NHIP_SEARCH_EXHAUSTIVE : 0" % S.EXHAUSTIVE_SIDE_MAX,
                 "const bool cacheable = reach_max <= %d && n_b > 0;" % S.REACH_CACHE_MAX,
                 "lround((double)h1 * p->low_res / p->high_res) + ratio + 2;", "if ((r & 1) && r <= %d) {" % S.PART_ROT_MAX,
                 "if (plan.form == MATCH_BNB && s.n_theta > %d)" % S.PART_ROT_MAX,
                 "std::max<size_t>((size_t)n_a, %d)" % S.SCRATCH_FIRST, "s1.n_theta <= DROPIN_CHAIN_ROT_MAX && c1.parts == 1",
                 "const nhip_search_t s2 = {21, 2 * ratio + 1, 2 * ratio + 1,", "const double coarse_step = M_PI / 180.0;"):
        assert line in dropin, line
    assert "spec->max_shift <= %d" % S.MAX_SHIFT_MAX in _src("nhip_layout.hip")
    assert "constexpr int SMALL_PASSES = %d;" % (S.SMALL_LANES_X_PASSES // 64) in small
    assert "constexpr int64_t SMALL_TILED_MAX_BLOCKS = %d;" % S.TILED_BLOCKS_MAX in small
    assert "constexpr int MAX_ROT = %d;" % S.BNB_ROT_MAX in params
    assert "constexpr int BNB_B = %d;" % S.BNB_BLOCK in _src("nhip_common.h")
    assert "constexpr int BNB_MAX_NB = %d;" % S.BNB_BLOCKS_MAX in _src("nhip_common.h") and "constexpr int NB = BNB_MAX_NB;" in params
    with open(os.path.join(ROOT, "include", "nautilus_hip.h")) as f:
        assert "#define NHIP_SHORT_SCAN_POINTS %d" % S.SHORT_SCAN in f.read()


def test_every_constructor_meets_the_arithmetic_condition_of_its_flow():
    """Plane sizes against 256 and 21, n_theta against 8 and 512, reach_max against 4096 (the rules at the top of
    tests/dropin_seams.py), for every (constructor, restriction) the families use."""
    f = S.flow(S.WALK, 3 * S.DEG)
    assert (f.n_theta1, f.side1, f.side2, f.ratio, f.coarse, f.fine_form, f.chained, f.fused) == (7, 9, 7, 3, "poses", 2, True, True)
    assert f.side1 ** 2 <= 256 and f.side2 ** 2 <= 256 and f.reach_max == 10 + 3 + 2
    assert S.flow(S.WALK, 20 * S.DEG)[:4] == (4, 9, 41, "poses") and S.flow(S.WALK, 20 * S.DEG).fused
    f = S.flow(S.STRIPS, 3 * S.DEG)
    assert (f.side1, f.coarse, f.side2, f.fine_form, f.chained, f.fused) == (17, "strips", 7, 2, True, False)
    assert 256 < f.side1 ** 2 and f.side1 <= 21
    f = S.flow(S.BNB1, 3 * S.DEG)
    assert (f.side1, f.n_theta1, f.coarse, f.parts, f.side2, f.fine_form, f.chained, f.fused) == (25, 7, "bnb", 1, 7, 2, True, False)
    assert f.side1 > 21 and f.n_theta1 <= 8 and 3 * S.DEG < 4 * S.DEG
    f = S.flow(S.DEFAULT, 3 * S.DEG)
    assert (f.side1, f.coarse, f.ratio, f.side2, f.fine_form, f.chained, f.fused) == (13, "poses", 30, 61, 2, True, True)
    assert f.side2 ** 2 > 256 and 21 * math.ceil(61 / (256 // 61)) <= 2048 and f.reach_max == 180 + 30 + 2
    f = S.flow(S.ROT, 20 * S.DEG)
    assert (f.side1, f.n_theta1, f.coarse, f.parts, f.per, f.chained) == (49, 41, "bnb", 6, 7, False)
    assert f.parts * f.per == f.n_theta1 + 1, "one copy of the last rotation behind the table"
    assert math.ceil(f.side1 / 8) <= 11 and f.cacheable
    f = S.flow(S.ROT, 3 * S.DEG)
    assert (f.n_theta1, f.coarse, f.parts, f.chained, f.fused) == (7, "bnb", 1, True, False)
    f = S.flow(S.NOCACHE, S.DEG)
    assert (f.h1, f.ratio, f.reach_max, f.cacheable, f.chained) == (38, 105, 4097, False, False) and f.reach_max > 4096
    assert (f.side1, f.n_theta1, f.coarse, f.parts, f.side2, f.fine_form) == (77, 3, "bnb", 1, 211, 1)
    assert f.reach_max - 2 == 4095 <= S.MAX_SHIFT_MAX, "the corner's fine table is one a grid spec admits"
    f = S.flow(S.REFUSED, S.DEG)
    assert (f.h1, f.ratio, f.cacheable, f.coarse, f.parts) == (40, 100, False, "bnb", 1) and f.reach_max - 2 == 4100 > S.MAX_SHIFT_MAX
    # the issue's example is cacheable after all: 4.8 / 0.1 is below 48 in double
    assert S.flow((3.0, 4.8, 0.1, 0.00119), S.DEG).h1 == 47 and S.flow((3.0, 4.8, 0.1, 0.00119), S.DEG).cacheable
    # an empty target is never cached, whatever its reach
    assert not S.flow(S.WALK, 3 * S.DEG, n_b=0).chained
    # the rotation counts: 511 against 513 around DROPIN_CHAIN_ROT_MAX, a single rotation (half1 = 0)
    for case, n, chained in S.rotation_counts():
        f = S.flow_of(case)
        assert (f.n_theta1, f.chained, f.coarse) == (n, chained, "poses"), case.name
    assert [n for _, n, _ in S.rotation_counts()] == [1, 1, 511, 513, 721]
    # half-degree restrictions are far from the floor's steps
    for deg in (0.5, 255.5, 256.5):
        assert abs(math.radians(deg) / S.DEG - round(math.radians(deg) / S.DEG - 0.5) - 0.5) < 1e-9


def test_lround_halves_occur_in_the_bridge():
    """tx1 / high_res of the WALK constructor is exactly +-2.5, +-7.5 for the odd coarse translations: the device's lround
    must round them away from zero as the host's and the oracle's do."""
    for k in (-3, -1, 1, 3):
        q = float(np.float32(k * 0.25)) / 0.1
        assert q == k * 2.5 and abs(q) % 1.0 == 0.5
        assert S.lround(q) == (3 if abs(k) == 1 else 8) * (1 if k > 0 else -1)
        assert S.lround(q) != math.floor(q + 0.5) if k < 0 else S.lround(q) == math.floor(q + 0.5)
    assert 0.25 / 0.1 == 2.5 and S.flow(S.WALK, 0).ratio == 3


def test_translation_walk_reaches_every_coarse_translation_and_clamps_beyond():
    """The transform is minus the shift: for every in-lattice (i, j) the oracle's (tx, ty) lies within low_res / 2 + high_res
    of it; round(t / low_res) covers -h1 .. h1 on both axes; the outermost ring returns border values.  The oracle's coarse
    record is on the designed cell for every in-lattice shift of the odd translations (the exact halves)."""
    walk = S.translation_walk()
    h1, low, high = 4, 0.25, 0.1
    assert len(walk) == (2 * h1 + 3) ** 2
    seen_x, seen_y = set(), set()
    for (i, j), case in walk.items():
        (tx, ty), _ = S.want(case)[1]
        if max(abs(i), abs(j)) <= h1:
            assert abs(float(tx) + i * low) <= low / 2 + high + 1e-6 and abs(float(ty) + j * low) <= low / 2 + high + 1e-6, (i, j, tx, ty)
            seen_x.add(round(float(tx) / low))
            seen_y.add(round(float(ty) / low))
        else:
            # beyond the lattice: the coarse optimum is ON the border (the fine search runs at the farthest reach)
            _, ix, iy, _ = S.coarse(case)
            assert abs(i) <= h1 or ix == (0 if i > 0 else 2 * h1), (i, j, ix)
            assert abs(j) <= h1 or iy == (0 if j > 0 else 2 * h1), (i, j, iy)
    assert seen_x == set(range(-h1, h1 + 1)) and seen_y == set(range(-h1, h1 + 1))
    # every exact half is a coarse optimum of some call, on both axes and both signs
    cx = {S.coarse(c)[1] - h1 for c in walk.values()}
    cy = {S.coarse(c)[2] - h1 for c in walk.values()}
    assert {-3, -1, 1, 3} <= cx and {-3, -1, 1, 3} <= cy
    # the rings of the other constructors: the coarse optimum on the border of each, in all 8 directions
    for ctor, bits in ((S.STRIPS, 16), (S.BNB1, 16), (S.WALK, 8)):
        h = S.flow(ctor, 3 * S.DEG).h1
        ringed = S.translation_walk(ctor, bits, False)
        assert sorted(ringed) == sorted(S.ring(h)) and len(ringed) == 8
        for (i, j), case in ringed.items():
            _, ix, iy, _ = S.coarse(case)
            for shift, cell in ((i, ix), (j, iy)):      # on the border along a shifted axis, within a cell of the centre along the other
                assert cell == h - np.sign(shift) * h if shift else abs(cell - h) <= 1, (ctor, bits, i, j, ix, iy)


def test_rotation_walk_wins_at_every_rotation_of_every_part():
    """The oracle's theta rounds to every degree in -20 .. 20 and to +-20 or +-21 beyond; its coarse winner is rotation
    k + 20 (0 and 40 beyond): each of the 6 parts of 7 wins at its first and its last rotation, and rotation 40 -- whose copy
    is entry 41 of the table -- wins twice."""
    for bits in (16, 8):
        walk = S.rotation_walk(bits)
        for k in range(-21, 22):
            deg = round(math.degrees(float(S.want(walk[k])[1][1])))
            assert deg == k if abs(k) <= 20 else deg in (k, k - np.sign(k)), (bits, k, deg)
            assert S.coarse(walk[k])[0] == min(max(k + 20, 0), 40), (bits, k)
        assert S.coarse(walk["empty"])[:3] == (0, 0, 0) and len(walk["empty"].a) == 0
    f = S.flow(S.ROT, 20 * S.DEG)
    winners = {S.coarse(c)[0] for c in S.rotation_walk(16).values()}
    assert all(q * f.per in winners and min(q * f.per + f.per - 1, 40) in winners for q in range(f.parts))


def test_angle_wraps_are_live():
    w = S.angle_wraps()
    th = {k: float(S.want(c)[1][1]) for k, c in w.items()}
    assert S.angle_diff(math.pi, 0.0) == math.pi and S.angle_diff(0.0, math.pi) == -math.pi, "rint ties to even: neither wraps"
    assert abs(th[(math.pi, 0.0)] - th[(0.0, math.pi)] - 2 * math.pi) < 1e-6
    assert abs(S.angle_diff(3.0, -3.0) - (6.0 - 2 * math.pi)) < 1e-15 and abs(th[(3.0, -3.0)] - (6.0 - 2 * math.pi)) < 2.5 * S.DEG
    assert abs(S.angle_diff(-3.0, 3.0) + (6.0 - 2 * math.pi)) < 1e-15 and abs(S.angle_diff(7.0, 0.5) - (6.5 - 2 * math.pi)) < 1e-15
    assert S.angle_diff(math.pi - 1e-9, -1e-9) in (math.pi, np.nextafter(math.pi, 0), np.nextafter(math.pi, 4))
    # the coarse winner's angle beyond +pi: theta0 + (k - half) * 1 deg is handed to the fine level unwrapped
    k = S.coarse(w["beyond"])[0]
    assert 3.13 + (k - 5) * S.DEG > math.pi and th["beyond"] > math.pi


def test_length_sequence_crosses_the_scratch_and_short_scan_seams():
    for ctor in (S.WALK, S.ROT):
        seq = S.length_sequence(ctor)
        assert tuple(len(c.a) for c in seq) == S.LENGTHS
        assert [S.flow_of(c).n_theta1 for c in seq] == [7, 41] * 4 + [7], "the kept rotation table is replaced and replaced back"
    n = S.LENGTHS
    assert n[0] == S.SCRATCH_FIRST + 1 and n[2] == S.SCRATCH_FIRST and n[7] > n[0] and n[1] < n[0] and n[8] < n[7]
    assert n[3] == S.SHORT_SCAN + 1 and n[4] == S.SHORT_SCAN and 0 in n and 1 in n
    rot = [S.flow_of(c) for c in S.length_sequence(S.ROT)]
    assert [f.parts for f in rot] == [1, 6] * 4 + [1] and [f.chained for f in rot] == [True, False] * 4 + [True]
    assert all(S.flow_of(c).fused for c in S.length_sequence(S.WALK))
    # short scans meet both a dealt and an undealt branch-and-bound search, and so do long ones
    assert {(len(c.a) <= S.SHORT_SCAN, f.parts) for c, f in zip(S.length_sequence(S.ROT), rot)} == {(True, 1), (True, 6), (False, 1), (False, 6)}


def test_non_cacheable_target_and_its_cost():
    nc = S.non_cacheable()
    t = time.perf_counter()
    (tx, ty), _ = S.want(nc["corner"])[1]
    dt = time.perf_counter() - t
    print("oracle call of the non-cacheable constructor %r: %.2f s" % (S.NOCACHE, dt))
    assert len(nc["match"].b) > 0 and not S.flow_of(nc["match"]).cacheable
    assert S.coarse(nc["match"])[1:3] == (38, 38) and S.coarse(nc["corner"])[1:3] == (0, 0)
    assert S.lround(float(np.float32(-38 * 0.21)) / 0.002) == -3990, "origin -3990: max_shift = 3990 + ratio = 4095 exactly"
    assert abs(float(tx) + 7.98) <= 0.21 + 1e-6 and abs(float(ty) + 7.98) <= 0.21 + 1e-6
    refused = S.non_cacheable(S.REFUSED)
    assert S.coarse(refused["match"])[1:3] == (40, 40) and S.coarse(refused["corner"])[1:3] == (0, 0)
    assert S.lround(float(np.float32(-40 * 0.2)) / 0.002) == -4000
    assert S.want(nc["match"])[1][0] == (0.0, 0.0)
    assert dt < 5.0


def test_cache_targets_differ():
    t = S.cache_targets()
    assert len({c.b.tobytes() for c in t.values()}) == 3 and all(S.flow_of(c).cacheable for c in t.values())


def test_zz_the_whole_file_runs_in_under_a_minute():
    dt = time.perf_counter() - _CLOCK["t0"]
    print("tests/test_dropin_seams_cpu.py: %.1f s since its first test began" % dt)
    assert dt < 60.0
