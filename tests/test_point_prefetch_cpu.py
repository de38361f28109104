"""The case lists of tests/test_point_prefetch_gpu.py (tests/point_prefetch.py), without a GPU: the slot counts are the
headers', every seam of both loops has a scan on either side of it and on it, some scan ends in every body of a turn, and
the forms are the ones the hooks select."""
import os
import re

import numpy as np

from tests import point_prefetch as M

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nautilus_amd", "csrc")


def _constant(header, name):
    text = open(os.path.join(CSRC, header)).read()
    found = re.findall(r"constexpr int %s = (\d+);" % name, text)
    assert len(found) == 1, (header, name, found)
    return int(found[0])


def test_slot_counts_are_the_headers():
    assert M.BOUNDS_SLOTS == _constant("nhip_bnb_bounds.h", "PD")
    assert M.ORIGIN_SLOTS == _constant("nhip_bnb_origin.h", "D")
    assert M.BY_ROTATION_MAX == M.CHUNK * _constant("nhip_bnb_params.h", "OCL")


def test_lengths_sit_on_the_seams():
    L = set(M.LENGTHS)
    assert M.LENGTHS == sorted(L) and min(L) == 1
    assert {1, 63, 64, 65, 127, 128, 129, 1081, 1087, 1088} <= L
    for slots in (M.BOUNDS_SLOTS, M.ORIGIN_SLOTS):
        for t in range(1, 4):
            m = 64 * slots * t
            assert {m - 1, m, m + 1} <= L, (slots, t)
            # m - 1 and m end in the last body of turn t - 1 (m fills it), m + 1 opens turn t with one point
            assert M.ends_in(m - 1, slots) == (t - 1, slots - 1, False)
            assert M.ends_in(m, slots) == (t - 1, slots - 1, True)
            assert M.ends_in(m + 1, slots) == (t, 0, False)
        # some scan ends inside every body of a turn, and some fills it
        inside = {M.ends_in(n, slots)[1] for n in L if not M.ends_in(n, slots)[2]}
        full = {M.ends_in(n, slots)[1] for n in L if M.ends_in(n, slots)[2]}
        assert inside == full == set(range(slots)), (slots, inside, full)
    # a scan that ends inside a slot's second body, one that ends exactly on a turn of both loops
    assert M.ends_in(100, M.BOUNDS_SLOTS)[1:] == (1, False) and M.ends_in(100, M.ORIGIN_SLOTS)[1:] == (1, False)
    both = 64 * M.BOUNDS_SLOTS * M.ORIGIN_SLOTS
    assert both in L and M.ends_in(both, M.BOUNDS_SLOTS)[1:] == (M.BOUNDS_SLOTS - 1, True)
    assert M.ends_in(both, M.ORIGIN_SLOTS)[1:] == (M.ORIGIN_SLOTS - 1, True)
    # the by-rotation form's last turn: 1088 = 17 chunks ends in body 0 of turn 8 (bounds) and body 1 of turn 5 (origins)
    assert M.ends_in(M.BY_ROTATION_MAX, M.BOUNDS_SLOTS) == (8, 0, True)
    assert M.ends_in(M.BY_ROTATION_MAX, M.ORIGIN_SLOTS) == (16 // M.ORIGIN_SLOTS, 16 % M.ORIGIN_SLOTS, True)
    assert [n for n in M.LENGTHS if n > M.BY_ROTATION_MAX] == [1089, 1151, 1152, 1153]  # (the general kernel's pairs)


def test_scans_have_the_lengths(small_bag):
    scans = M.scans_of(small_bag)
    assert [len(s) for s in scans[len(small_bag.scans):]] == M.LENGTHS
    src = small_bag.scans[M.SRC_SCAN]
    for s in scans[len(small_bag.scans):]:
        assert s.dtype == np.float32 and np.array_equal(s[:len(src)], src[:len(s)])
    assert np.abs(src).max() < M.RANGE_M and int(round(2 * M.RANGE_M / M.RES)) == 400


def test_forms():
    assert sorted(f for _, f in M.FORMS.values()) == [0, 0, 1, 3]
    assert M.FORMS["hand_over"][0]["NHIP_BNB_KERNELS"] == "2" and M.FORMS["split"][0]["NHIP_BNB_SPLIT"] == "1"
    assert set(M.INSTR) == {"NHIP_BNB_INSTRUMENT", "NHIP_BNB_STATS"} and len(M.EVERY_ADD) == 3
