"""The case lists of tests/test_rotation_round_trips_gpu.py (tests/rotation_round_trips.py), without a GPU: the constants
are the headers', the rotation counts give every kind of wave, the scan lengths sit on the chunk seams, the table sides
give the pooled-table sizes the module says (by csm.grid_layout) and no side gives one nearer a seam of the staging loop,
the global-pool side is the smallest, and the edge scans put window origins on the last and the lowest rows."""
import os
import re

import numpy as np

from nautilus_amd import csm
from tests import rotation_round_trips as M

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nautilus_amd", "csrc")


def _constant(header, name):
    text = open(os.path.join(CSRC, header)).read()
    found = re.findall(r"constexpr int %s = (\d+);" % name, text)
    assert len(found) == 1, (header, name, found)
    return int(found[0])


def _layout(side, max_shift, bits=16):
    class _Csm:  # (spec_of wants the module)
        grid_spec = staticmethod(csm.grid_spec)
    L = csm.grid_layout(M.spec_of(_Csm, side, max_shift, bits))
    assert L.side == side, (L.side, side)
    return L


def test_constants_are_the_headers():
    assert M.PD == _constant("nhip_bnb_bounds.h", "PD")
    assert M.WAVES == _constant("nhip_bnb_params.h", "BNB_WAVES") == _constant("nhip_bnb_params.h", "SPLIT_WAVES")
    params = open(os.path.join(CSRC, "nhip_bnb_params.h")).read()
    assert M.QCAP == _constant("nhip_bnb_params.h", "QCAP") and "LDS_TAIL_BYTES = %d;" % M.LDS_TAIL_BYTES in params
    assert M.ORG_LDS == M.WAVES * _constant("nhip_bnb_params.h", "OCL") * 64 * 4
    host = open(os.path.join(CSRC, "nhip_bnb_host.hip")).read()
    assert "constexpr size_t LDS_MAX = 160 * 1024;" in host and M.LDS_MAX == 160 * 1024
    assert max(M.N_THETAS) <= _constant("nhip_bnb_params.h", "MAX_ROT") <= 64 * M.WAVES  # (a wave's rotations fit its lanes)


def test_rotation_counts_give_every_kind_of_wave():
    assert M.N_THETAS == (1, 7, 8, 9, 15, 16, 17, 61)
    kinds = {n: set(M.wave_rotations(n)) for n in M.N_THETAS}
    assert kinds[1] == {0, 1} and kinds[7] == {0, 1} and kinds[8] == {1}      # waves without a rotation; exactly one each
    assert kinds[9] == {1, 2} and kinds[15] == {1, 2} and kinds[16] == {2}   # the last rotation of some waves only
    assert kinds[17] == {2, 3} and kinds[61] == {7, 8}
    for n in M.N_THETAS:
        per = M.wave_rotations(n)
        assert sum(per) == n and per == sorted(per, reverse=True)
        # the lanes past a wave's last rotation read that rotation again: its index is the wave's own, inside the table
        for w, c in enumerate(per):
            assert c == 0 or w + M.WAVES * (c - 1) < n
    assert M.wave_rotations(M.N_THETA) == [2] + [1] * 7


def test_scan_lengths_sit_on_the_chunk_seams(small_bag):
    assert M.LENGTHS == (0, 1, 63, 64, 65, 127, 128, 129, 1081, 1088)
    turn = M.CHUNK * M.PD
    assert {turn - 1, turn, turn + 1} <= set(M.LENGTHS) and {M.CHUNK - 1, M.CHUNK, M.CHUNK + 1} <= set(M.LENGTHS)
    assert max(M.LENGTHS) == M.CHUNK * _constant("nhip_bnb_params.h", "OCL")  # the longest scan of the by-rotation form
    todo, tgt = M.groups(small_bag)
    by_name = {g[0]: g for g in todo}
    assert [len(s) for s in by_name["lengths"][3]] == list(M.LENGTHS)
    assert sorted(by_name) == sorted(["rot%d" % n for n in M.N_THETAS] + ["lengths", "rows"] +
                                     ["pool%d" % s for s in list(M.POOL_SIDES) + [M.GLOBAL_SIDE]])
    assert all(g[4] == M.N_THETA for g in todo if not g[0].startswith("rot")) and np.array_equal(tgt, small_bag.scans[M.TGT_SCAN])
    assert np.abs(small_bag.scans[M.SRC_SCAN]).max() < M.RANGE_M


def test_table_sides_give_the_pooled_sizes():
    assert _layout(M.BASE_SIDE, M.MAX_SHIFT).pad == M.pad_of(M.MAX_SHIFT) and _layout(M.BASE_SIDE, M.EDGE_SHIFT).pad == M.pad_of(M.EDGE_SHIFT)
    for bits in (8, 16):
        for side, residue in M.POOL_SIDES.items():
            L = _layout(side, M.MAX_SHIFT, bits)
            assert L.pool_bytes % 16 == 0 and L.pool_bytes // 16 == M.pooled_words(side, L.pad), (side, L.pool_bytes)
            assert (L.pool_bytes // 16) % M.ROUND == residue and M.pool_in_lds(L.pool_bytes // 16), (side, L.pool_bytes)
    # the residues of the issue's windows that some side gives are all in the list, and the list is the nearest on either
    # side of each seam that ANY side gives
    near = M.nearest_residues()
    assert near == {(0, "below"): None, (0, "above"): 16, (512, "below"): 510, (512, "above"): 513, (1536, "below"): 1530,
                    (1536, "above"): 1540, (M.ROUND, "below"): 2044, (M.ROUND, "above"): None}
    assert sorted(M.POOL_SIDES.values()) == sorted(r for r in near.values() if r is not None)
    windows = set([0, 1, 511, 512, 513, 1535, 1536, 1537, 2046, 2047])
    reachable = {M.pooled_words(s, M.pad_of(M.MAX_SHIFT)) % M.ROUND for s in range(8, 4096)
                 if M.pool_in_lds(M.pooled_words(s, M.pad_of(M.MAX_SHIFT)))}
    assert windows & reachable == {513}
    # more than one round, and a last round of every fill
    words = {s: M.pooled_words(s, M.pad_of(M.MAX_SHIFT)) for s in M.POOL_SIDES}
    assert min(words.values()) < M.THREADS and max(words.values()) > 3 * M.ROUND, words


def test_global_side_is_the_smallest():
    at, before = _layout(M.GLOBAL_SIDE, M.MAX_SHIFT), _layout(M.GLOBAL_SIDE - 1, M.MAX_SHIFT)
    assert not M.pool_in_lds(at.pool_bytes // 16) and M.pool_in_lds(before.pool_bytes // 16)
    assert all(M.pool_in_lds(M.pooled_words(s, M.pad_of(M.MAX_SHIFT))) for s in range(8, M.GLOBAL_SIDE))
    # (the matcher still takes it: bnb_fits asks for the bounds beside a global pool, and offsets below 1 << 25)
    assert M.ORG_LDS + M.N_THETA * 512 + M.QCAP * 8 + M.LDS_TAIL_BYTES <= M.LDS_MAX and at.pool_bytes < (1 << 25)


def test_edge_scans_reach_the_last_and_the_lowest_rows(small_bag):
    L = _layout(M.BASE_SIDE, M.EDGE_SHIFT)
    image_rows = (L.side + 2 * L.pad + 7) // 8          # pooled rows of the stored image; NB + 1 = 12 rows of zeros follow
    assert L.pool_rows == image_rows + 12
    h = M.NXY // 2
    for scan in (small_bag.scans[M.SRC_SCAN], small_bag.scans[M.TGT_SCAN]):
        pts = M.edge_scan(scan)
        assert pts.dtype == np.float32 and 64 * 17 >= len(pts) > 64 * 8  # (the by-rotation form; several passes of the gather)
        rows = M.origin_rows(pts, L.side, M.EDGE_SHIFT)
        top, low = int(rows.max()), int(rows.min())
        assert top == (L.side + L.pad) >> 3 and top + 10 >= image_rows and top + 10 < L.pool_rows, (top, image_rows)
        assert low == (L.pad - 2 * h - 1) >> 3 == 1, low   # (the clamp keeps 2 h + 1 stored rows above: row 0 is never an origin)
    # with the default border the rows of the last origin stay inside the image: this is what EDGE_SHIFT is for
    Ld = _layout(M.BASE_SIDE, M.MAX_SHIFT)
    assert ((Ld.side + Ld.pad) >> 3) + 10 < (Ld.side + 2 * Ld.pad + 7) // 8
