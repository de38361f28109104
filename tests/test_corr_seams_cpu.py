"""Preconditions of the correspondence-search seam tests (tests/test_corr_seams_gpu.py), without a GPU: every input of
tests/corr_seams.py is the case it claims to be -- the restated path conditions give the path its family is named for, the
oracle keeps the designed rows and matches the designed targets, and every designed feature is load-bearing (the oracle's
rows change when it is removed).  An edit of the inputs that stops exercising a seam fails HERE, not silently on the device.
A precondition that fails means the input is wrong.  (nhip_corr.hip, K5.)"""
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import corr_seams as S

ID = [1, 0, 0, 0]


def _block(src, tgt, tgt_nrm=None, thr=S.THR):
    """The oracle on one block at zero poses, with this module's normals: (rows, matched indices)."""
    nrm = S.normals_of(len(tgt)) if tgt_nrm is None else tgt_nrm
    return O.corr_search_block(src, S.normals_of(len(src)), tgt, nrm, ID, ID, thr)


def _rows_of(case, b):
    """Rows and matched indices of block b by the per-block entry point; they are the batch's rows."""
    src, sn, tgt, tn = case.block(b)
    rows, idx = O.corr_search_block(src, sn, tgt, tn, ID, ID, case.thr)
    assert rows.tobytes() == S.block_rows(case.name, False, b).tobytes()
    assert np.array_equal(S.matched_index(rows), idx), "a row names the matched index through its target normal"
    return rows, idx


def test_the_kernel_constants_are_the_ones_the_inputs_were_cut_for():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = ""
    for unit in ("nhip_corr_shared.h", "nhip_corr.hip"):  # the search K5 shares with the refinement, and K5's own unit
        with open(os.path.join(root, "nautilus_amd", "csrc", unit)) as f:
            src += f.read()
    for line in ("constexpr int CT = %d;" % S.LANES, "constexpr int TGT_CHUNK = %d;" % S.STAGE,
                 "constexpr int MAX_PER_LANE = %d;" % S.ROUNDS, "constexpr int NB = %d;" % S.BUCKETS,
                 "constexpr float CELL_LIMIT = %.1ff;" % S.CELL_LIMIT, "base += %d)" % S.SCAN_STEP, "__fmul_rn(thr, 1.001f)",
                 "* 73856093u) ^ ((uint32_t)cy * 19349663u)"):
        assert line in src, line
    assert S.PASS == 2048 and S.LANES // S.WAVE == 4


def test_zero_poses_are_the_identity_and_normals_name_indices():
    assert np.array_equal(O.pose_affines(np.zeros((3, 3))), np.tile(np.float32(ID), (3, 1)))
    nrm = S.normals_of(4098, failing=(7,))
    assert nrm.dtype == np.float32 and len(np.unique(nrm[:, 1])) == 4098
    assert np.array_equal(S.matched_index(np.concatenate([np.zeros((4098, 6), np.float32), nrm], axis=1)), np.arange(4098))
    # the gate's dot product with a source normal (1, sy > 0): at least 1 where the target's is (1, ty), at most 0.51^2 where (0, ty)
    assert nrm[:, 1].max() <= 0.51 and 0.51 * 0.51 < S.MIN_COS < 1.0 and nrm[7, 0] == 0 and np.all(np.delete(nrm[:, 0], 7) == 1)


def test_a_every_mask_is_the_oracles_kept_set_on_the_hashed_walk():
    c = S.family_a()
    blocks = c.design["blocks"]
    assert sorted({ns for ns, _, _, _ in blocks}) == sorted(S.A_LENGTHS) and len(c.scans[0]) == S.A_TARGET
    names = {}
    for b, (ns, name, mask, j) in enumerate(blocks):
        names.setdefault(ns, []).append(name)
        src = c.scans[c.bs[b]]
        assert len(src) == ns == len(mask) and c.bt[b] == 0
        assert S.paths(c, b) == (True, [False] * -(-ns // S.PASS)), (ns, name)
        rows, idx = _rows_of(c, b)
        assert rows[:, :2].tobytes() == src[mask].tobytes(), (ns, name, "the kept set is the mask, in source order")
        assert np.array_equal(idx, j[mask]), (ns, name)
        assert S.block_rows("a", True, b).tobytes() == rows.tobytes(), "the gate passes every designed match"
    assert names[4097] == ["all", "none", "alternating", "half", "lone@0", "lone@63", "lone@64", "lone@255", "lone@256",
                           "lone@2047", "lone@2048", "lone@4096"]
    assert names[0] == ["all"] and names[1] == ["all", "none"] and "lone@63" in names[64] and "lone@64" not in names[64]
    assert names[2049][-3:] == ["lone@256", "lone@2047", "lone@2048"], "the last point of a pass and the first of the next"
    rows, counts, cap = S.expected("a", False)
    print("family a: %d blocks, %d source points, %d rows" % (len(blocks), cap[-1], counts.sum()))
    assert len(blocks) > 120 and (counts == 1).sum() >= 60 and (counts == 0).sum() >= 15


def test_b_nearest_neighbours_at_the_ends_and_across_the_stage_seams():
    c = S.family_b()
    blocks = c.design["blocks"]
    assert sorted({nt for nt, _, _, _ in blocks}) == sorted(S.B_LENGTHS)
    seen = set()
    for b, (nt, variant, sets, j) in enumerate(blocks):
        src, _, tgt, tn = c.block(b)
        assert len(tgt) == nt and len(src) == S.B_SOURCES
        assert S.paths(c, b) == (nt <= S.STAGE, [nt > S.STAGE]), (nt, variant)
        rows, idx = _rows_of(c, b)
        lowest = S.lowest_coincident(tgt)
        assert rows[:, :2].tobytes() == src[j >= 0].tobytes(), (nt, variant)
        assert np.array_equal(idx, lowest[j[j >= 0]]), (nt, variant, "the designed target, the lowest of a coincident set")
        assert S.block_rows("b", True, b).tobytes() == rows.tobytes()
        assert (np.arange(nt) != lowest).sum() == len(sets) and all(lowest[hi] == lo for lo, hi in sets)
        if nt == 0:
            assert len(rows) == 0
            continue
        assert j[0] == 0 and j[1] == nt - 1
        for lo, hi in sets:
            seen.add((variant, lo, hi, nt > S.STAGE))
            assert hi in j[:4] and tn[lo].tobytes() != tn[hi].tobytes()
            # load-bearing: a tie that went to the higher index would change the row
            swapped = tn.copy()
            swapped[[lo, hi]] = tn[[hi, lo]]
            assert _block(src, tgt, swapped)[0].tobytes() != rows.tobytes(), (nt, variant, lo, hi)
        if variant == "ends":
            assert idx[1] == nt - 1 and lowest[nt - 1] == nt - 1, "a unique nearest neighbour is the last point"
            assert idx[0] == 0
            assert _block(src, tgt[:-1])[0].tobytes() != rows.tobytes(), "load-bearing: the last target point"
        if variant == "wrap":
            assert idx[1] == 0 and (0, nt - 1) in sets
        if variant == "seam":
            assert idx[2] == 2047 and (nt < 4097 or idx[3] == 4095)
    assert {("seam", 2047, 2048, True), ("seam", 4095, 4096, True), ("ends", 2047, 2048, True), ("wrap", 0, 2048, True),
            ("wrap", 0, 4096, True), ("wrap", 0, 2047, False), ("wrap", 0, 1, False)} <= seen, "(variant, lower, higher, exhaustive)"
    by = {(nt, v): S.paths(c, b)[0] for b, (nt, v, _, _) in enumerate(blocks)}
    assert by[(2048, "ends")] and by[(2048, "wrap")] and not by[(2049, "ends")] and not by[(2049, "seam")]
    rows, counts, cap = S.expected("b", False)
    print("family b: %d blocks, %d source points, %d rows; hashed %d, exhaustive %d" % (
        len(blocks), cap[-1], counts.sum(), sum(by.values()), len(by) - sum(by.values())))


@pytest.mark.parametrize("thr", S.C_THRESHOLDS)
def test_c_every_neighbour_cell_at_every_residue_on_both_sides_of_zero(thr):
    c = S.family_c(thr)
    d = c.design
    q, _, t, _ = c.block(0)
    assert len(q) == len(t) == 90 and S.paths(c, 0) == (True, [False])
    qc, tc = S.cells(q, thr), S.cells(t[d["target_of"]], thr)
    assert np.array_equal(qc, np.stack([d["cx"], d["cy"]], axis=1)), "every query in its designed cell"
    assert np.array_equal(tc - qc, np.stack([d["ox"], d["oy"]], axis=1)), "target cell - query cell is the designed offset"
    assert {(int(x), (int(a), int(b))) for x, a, b in zip(d["cx"], d["ox"], d["oy"])} == {(x, o) for x in S.C_CX for o in S.C_OFFSETS}
    assert set(d["cx"] & 3) == {0, 1, 2, 3} and set(d["cx"][d["cx"] < 0] & 3) == {0, 1, 2, 3} == set(d["cx"][d["cx"] >= 0] & 3)
    assert (d["cy"] < 0).any() and (d["cy"] > 0).any() and np.abs(np.diff(d["cy"])).min() >= 10
    two = S.two_runs(d["cx"])
    assert two.any() and (~two).any() and {int(x) for x in d["cx"][two]} == {-5, -4, -1, 0, 3, 4}
    # the target's bucket lies in the run the kernel visits it in: the first run ends at the group's last cell
    in_second = two & (((d["cx"] + d["ox"]) >> 2) != ((d["cx"] - 1) >> 2))
    assert in_second.any() and (two & ~in_second).any()
    assert np.all(S.bucket(tc[:, 0], tc[:, 1]) < S.BUCKETS)
    rows, idx = _rows_of(c, 0)
    assert len(rows) == 90 and np.array_equal(idx, d["target_of"]), "all 90 rows kept, each on its own target"
    dist = np.linalg.norm(t[d["target_of"]].astype(np.float64) - q, axis=1) / (float(np.float32(thr)) * 1.001)
    assert dist.max() < 0.86 and dist[(d["ox"] != 0) & (d["oy"] != 0)].min() > 0.84
    for n in (0, 44, 89):  # load-bearing: without its own target a query keeps no row
        assert len(_block(q[n:n + 1], np.delete(t, d["target_of"][n], axis=0), thr=thr)[0]) == 0
    assert S.block_rows(c.name, True, 0).tobytes() == rows.tobytes()
    print("family c thr %g: 1 block, 90 rows; two-run queries %d (target in the second run %d), one-run %d" % (
        thr, two.sum(), in_second.sum(), (~two).sum()))


def test_d_one_bucket_holds_the_stage_and_2048_cells_hold_one_point_each():
    c = S.family_d()
    q, _, one, _ = c.block(0)
    assert len(one) == S.STAGE and S.paths(c, 0) == (True, [False])
    oc = S.cells(one, c.thr)
    assert np.all(oc == S.D_CELL) and len(np.unique(S.bucket(oc[:, 0], oc[:, 1]))) == 1
    lowest = S.lowest_coincident(one)
    assert (lowest != np.arange(S.STAGE)).sum() == sum(len(s) - 1 for s in S.D_COINCIDENT), "distinct but for the designed sets"
    rows, idx = _rows_of(c, 0)
    kept = {p.tobytes(): i for p, i in zip(rows[:, :2], idx)}
    for query, want in c.design["on_sets"]:
        assert q[query].tobytes() == one[want].tobytes() and kept[q[query].tobytes()] == want == lowest[want]
        members = np.nonzero(lowest == want)[0]
        assert len(members) >= 2 and len({c.normals[1][m].tobytes() for m in members}) == len(members)
    qc = S.cells(q[len(S.D_COINCIDENT):], c.thr) - S.D_CELL
    assert {tuple(v) for v in qc} == set(S.C_OFFSETS) and len(q) == 2 + 9 * S.D_PER_CELL
    per_cell = {o: sum(1 for v, p in zip(qc, q[2:]) if tuple(v) == o and p.tobytes() in kept) for o in S.C_OFFSETS}
    assert all(n > 0 for n in per_cell.values()) and 2 + sum(per_cell.values()) == len(rows) < len(q), per_cell
    src, _, spread, _ = c.block(1)
    sc = S.cells(spread, c.thr)
    assert S.paths(c, 1) == (True, [False]) and len(np.unique(sc, axis=0)) == S.STAGE == len(spread)
    j = c.design["all_cells_designed"]
    rows1, idx1 = _rows_of(c, 1)
    assert rows1[:, :2].tobytes() == src[j >= 0].tobytes() and np.array_equal(idx1, j[j >= 0])
    buckets = np.bincount(S.bucket(sc[:, 0], sc[:, 1]), minlength=S.BUCKETS)
    for b in (0, 1):
        assert S.block_rows("d", True, b).tobytes() == S.block_rows("d", False, b).tobytes()
    print("family d: 2 blocks, %d + %d rows; one cell: %s kept per neighbour cell; 2048 cells: %d buckets used, fullest %d" % (
        len(rows), len(rows1), sorted(per_cell.values()), (buckets > 0).sum(), buckets.max()))


def test_e_a_query_beyond_the_limit_switches_its_pass_to_the_scan_of_the_hashed_target():
    c = S.family_e()
    want_paths = {"none": (True, [False, False]), "pass0": (True, [True, False]), "pass1": (True, [False, True]),
                  "both": (True, [True, True]), "huge pass0": (True, [True, False]), "huge pass1": (True, [False, True]),
                  "huge both": (True, [True, True]), "target beyond": (False, [True, True])}
    tgt = c.scans[0]
    lowest = S.lowest_coincident(tgt)
    assert len(tgt) == S.STAGE and [tuple(np.nonzero(lowest == s[0])[0]) for s in S.E_SETS] == [tuple(s) for s in S.E_SETS]
    assert np.abs(S.scaled(tgt, c.thr)).max() < S.CELL_LIMIT - 0.2 and tgt[:, 0].min() == 1000.0
    base = c.design["base"]
    none_rows = None
    for b, v in enumerate(c.design["variants"]):
        src = c.scans[c.bs[b]]
        assert len(src) == S.E_SOURCES == S.PASS + 300 and S.paths(c, b) == want_paths[v], v
        rows, idx = _rows_of(c, b)
        assert S.block_rows("e", True, b).tobytes() == rows.tobytes()
        kept = {p.tobytes(): i for p, i in zip(rows[:, :2], idx)}
        big = np.nonzero((np.abs(S.scaled(src, c.thr)) >= S.CELL_LIMIT).any(axis=1))[0]
        assert big.tolist() == [at for at, _ in c.design["far"][b]], "only the designed queries are beyond the limit"
        for at, want in c.design["far"][b]:
            assert kept.get(src[at].tobytes(), -1) == want, (v, at, "kept and matched to the lowest index of its set")
            if want >= 0:
                d = np.linalg.norm(tgt[want].astype(np.float64) - src[at])
                assert 0.14 < d < 0.16 and np.sort(np.linalg.norm(tgt.astype(np.float64) - src[at], axis=1))[4] > 0.3
                swapped = c.normals[0].copy()  # load-bearing: a tie that went to another member of the set changes the row
                swapped[[want, lowest.tolist().index(want, want + 1)]] = swapped[[lowest.tolist().index(want, want + 1), want]]
                assert _block(src, tgt, swapped)[0].tobytes() != rows.tobytes()
        if v == "none":
            none_rows = rows
            assert src.tobytes() == base.tobytes() and len(rows) == S.E_SOURCES
        elif v != "target beyond":
            assert rows.tobytes() != none_rows.tobytes(), "load-bearing: the far query"
            assert len(rows) == S.E_SOURCES - (len(c.design["far"][b]) if v.startswith("huge") else 0)
    beyond = c.scans[1]
    assert (beyond != tgt).any(axis=1).sum() == 1 and S.scaled(beyond[S.E_BEYOND], c.thr)[0] >= S.CELL_LIMIT
    assert S.E_AT[0] < S.PASS <= S.E_AT[1] < S.E_SOURCES
    _, counts, cap = S.expected("e", False)
    print("family e: %d blocks, %d source points, %d rows; paths %s" % (c.n_blocks, cap[-1], counts.sum(), want_paths))


def test_g_the_nearest_target_fails_the_gate_and_the_second_nearest_is_the_match():
    c = S.family_g()
    near, second = c.design["near"], c.design["second"]
    assert S.paths(c, 0) == (True, [False])
    rows, idx = _rows_of(c, 0)
    assert np.array_equal(idx, near) and len(rows) == S.G_SOURCES
    gated = S.block_rows("g", True, 0)
    assert len(gated) == S.G_SOURCES and np.array_equal(S.matched_index(gated), second)
    assert gated[:, :2].tobytes() == rows[:, :2].tobytes() and gated.tobytes() != rows.tobytes()
    assert np.all(c.normals[1][near, 0] == 0) and np.all(c.normals[1][second, 0] == 1)
    print("family g: 1 block, 300 rows plain (nearest), 300 rows gated (second nearest)")


@pytest.mark.parametrize("n", S.F_BLOCKS)
def test_f_blocks_without_rows_at_both_ends_and_across_every_step_seam(n):
    c = S.family_f(n)
    assert c.n_blocks == n and [len(s) for s in c.scans] == list(range(6)) * 3
    empty = c.design["empty"]
    for gated in (False, True):
        rows, counts, cap = S.expected(c.name, gated)
        boff, packed, cblock = S.compacted(c.name, gated)
        assert np.all(counts[empty] == 0) and np.all(counts[:S.F_EDGE_RUN] == 0) and np.all(counts[-S.F_EDGE_RUN:] == 0)
        assert counts[~empty].max() == 5 and (counts[~empty] > 0).mean() > 0.2
        for seam in range(S.SCAN_STEP, n + 1, S.SCAN_STEP):
            lo, hi = seam - S.F_SEAM_RUN, min(seam + S.F_SEAM_RUN, n)
            assert np.all(counts[lo:hi] == 0) and np.all(boff[lo:hi + 1] == boff[seam]) and 0 < boff[seam], "constant across the seam, carried"
            assert seam == n or boff[seam] < boff[-1] or n - seam <= S.F_SEAM_RUN
        assert boff[-1] == counts.sum() == len(packed) == len(cblock) and len(boff) == n + 1
        assert packed.tobytes() == np.concatenate([rows[cap[b]:cap[b] + counts[b]] for b in range(n)]).tobytes()
    capacity = np.diff(cap)
    assert (capacity[empty] == 0).any() and (capacity[empty] > 0).any(), "without rows for want of sources and for want of matches"
    assert all(S.paths(c, b)[0] for b in range(0, n, 97))
    print("family f %d: %d blocks, %d source points, %d rows" % (n, n, cap[-1], S.expected(c.name, False)[1].sum()))


def test_the_shared_inputs_are_read_only():
    for name in S.CASES:
        c = S.case(name)
        for a in [c.xy, c.nrm, c.off, c.bs, c.bt, c.aff] + list(S.expected(name, False)) + list(S.expected(name, True)):
            assert not a.flags.writeable
            with pytest.raises(ValueError):
                a[...] = 0
