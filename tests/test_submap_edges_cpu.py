"""Preconditions of the submap edge tests (tests/test_submap_edges_gpu.py), without a GPU: every input of tests/submap_edges.py
still makes the loop of nhip_submap.hip it was crafted for run more than once.  An edit of the inputs that stops exercising a
loop fails HERE, not silently on the device.  ("Submaps"; K10.)"""
import os

import numpy as np
import pytest

from tests import submap_edges as E
from tests import submap_reference as R

CHUNK, BATCH, STEP = E.GATHER_CHUNK, E.GATHER_THREADS, E.OFFSETS_STEP


def test_the_kernel_constants_are_the_ones_the_inputs_were_cut_for():
    assert (E.GATHER_THREADS, E.GATHER_CHUNK) == (R.GATHER_THREADS, R.GATHER_CHUNK)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "nautilus_amd", "csrc", "nhip_submap.hip")) as f:
        src = f.read()
    for line in ("constexpr int SUB_T = %d;" % BATCH, "constexpr int SUB_CHUNK = %d;" % CHUNK,
                 "constexpr int SUB_MAX_GRID = %d;" % E.GATHER_MAX_GRID, "base += %d)" % STEP):
        assert line in src, line


def test_the_mini_bag():
    xy, off = E.mini_packed()
    assert np.diff(off).tolist() == E.MINI_LENGTHS == [0, 1, 2, 3, 5, 8, 13, 21, 34, 40, 64, 1081, 65535, 65536]
    assert xy.dtype == np.float32 and len(xy) == off[-1] and np.isfinite(xy).all()
    assert [E.MINI_LENGTHS[i] for i in (E.EMPTY, E.S1081, E.S65535, E.S65536)] == [0, 1081, 65535, 65536]
    assert not xy.flags.writeable and not off.flags.writeable


def test_many_members_start_chunks_in_the_third_and_fourth_batch():
    member_scan, aff, moff = E.many_members()
    mxy, off = E.many_members_merged()
    assert len(off) == 3 and moff.tolist() == [0, E.MANY_MEMBERS, E.MANY_MEMBERS + 4] and len(aff) == len(member_scan)
    first = member_scan[:E.MANY_MEMBERS]
    lengths = np.asarray(E.MINI_LENGTHS)[first]
    assert set(first[lengths > 0]) <= set(range(1, 10)), "drawn from the scans of 1 .. 40 points"
    assert lengths[255] == 0 and lengths[512] == 0 and np.all(lengths[256:512] == 0), "empty: 255, batch 2, 512"
    assert lengths[254] > 0 and lengths[513] > 0
    starts = E.member_starts(first)
    assert starts[-1] == off[1] == len(mxy) - (off[2] - off[1]) and off[1] > 10000
    # the member each chunk of target 0 begins in
    begins = [int(np.searchsorted(starts, q, side="right") - 1) for q in range(CHUNK, int(off[1]), CHUNK)]
    print("chunks begin in members", begins)
    assert any(2 * BATCH <= m < 3 * BATCH for m in begins), "a chunk begins in the third batch"
    assert any(3 * BATCH <= m for m in begins), "a chunk begins in the fourth batch"
    assert starts[2 * BATCH] - starts[BATCH] == 0, "the second batch contributes no point"
    assert np.any(starts[1:-1] % BATCH != 0), "a member seam off a multiple of 256"
    # the target seam inside a chunk, the second target ragged
    assert 0 < off[1] < off[2] and off[1] % CHUNK != 0 and off[2] % CHUNK != 0
    (bad, _, _), (a, b) = E.many_members_bad_ids()
    assert 2 * BATCH <= a < 3 * BATCH <= b < E.MANY_MEMBERS and bad[a] == -1 and bad[b] == len(E.MINI_LENGTHS)
    assert lengths[a] > 0 and lengths[b] > 0 and (bad != member_scan).sum() == 2


def test_many_targets_cross_the_steps_of_the_offsets_kernel():
    member_scan, aff, moff = E.many_targets()
    mxy, off = E.many_targets_merged()
    n = E.MANY_TARGETS
    assert len(moff) == n + 1 == 2501 and n > 2 * STEP and n % STEP, "two full steps and a ragged one"
    counts = np.diff(moff)
    assert counts.max() == 2 and set(member_scan) <= set(range(6)), "0 .. 2 members of the scans of 0 .. 8 points"
    assert np.all(counts[:5] == 0) and np.all(counts[-7:] == 0) and np.all(counts[1000:2100] == 0)
    assert counts[5:1000].any() and counts[2100:-7].any()
    total = int(off[-1])
    assert total == len(mxy) > 2 * CHUNK
    assert np.all(off[1000:2101] == off[1000]), "out_offsets is constant across the empty run, over the step seam"
    assert 0 < off[STEP] < total, "the carry into the second step is not 0"
    assert 1000 < STEP < 2 * STEP < 2100, "both step seams inside the run: the second step adds nothing to the carry"
    ok = False
    for q in range(CHUNK, total, CHUNK):
        lo, hi = np.searchsorted(off, q, side="right") - 1, np.searchsorted(off, min(q + CHUNK, total), side="left")
        shared = np.nonzero(off[:-1] == q)[0]
        in_chunk = int(hi - lo)
        print("chunk at %d: targets %d .. %d (%d), %d targets start at it" % (q, lo, hi, in_chunk, len(shared)))
        ok |= len(shared) > 1 or in_chunk > 100
    assert ok
    # prefixes for the launches over 1024 and 1025 targets
    for k in (STEP, STEP + 1):
        ms, af, mo = E.first_targets(E.many_targets(), k)
        assert len(mo) == k + 1 and mo[-1] == len(ms) == len(af)


def test_grid_stride_gives_some_workgroups_a_second_chunk():
    member_scan, aff, moff = E.grid_stride()
    mxy, off = E.grid_stride_merged()
    assert np.all(member_scan == E.S1081) and len(moff) == 401 and np.all(np.diff(moff) == 10)
    assert len(np.unique(aff, axis=0)) == len(aff) == 4000, "each member under its own affine"
    assert off[-1] == len(mxy) == 4324000
    assert off[-1] > E.GATHER_MAX_GRID * CHUNK and off[-1] % CHUNK, "beyond one chunk per workgroup, ragged last chunk"
    chunks = -(-int(off[-1]) // CHUNK)
    assert E.GATHER_MAX_GRID < chunks < 2 * E.GATHER_MAX_GRID, "some workgroups take two chunks, the others one"


def test_the_four_totals_beyond_int32():
    lengths = [int(v) for v in E.MINI_LENGTHS]
    want = {"a": (2 ** 32 + 1081, 1, 2 ** 31 - 1), "b": (2 ** 32 + 1081, 2048, 2 ** 31 - 1), "c": (2 ** 31, 1, 2 ** 31 - 1),
            "d": (2 ** 31 - 1, 1, 2 ** 31 - 1)}
    assert E.BEYOND_CASES == sorted(want)
    for case in E.BEYOND_CASES:
        (member_scan, aff, moff), total, value = E.beyond_int32(case)
        assert sum(lengths[i] for i in member_scan) == total == want[case][0]
        assert len(moff) - 1 == want[case][1] and value == want[case][2] and len(aff) == len(member_scan) == moff[-1]
        assert total > E.BEYOND_CAPACITY
    assert (2 ** 32 + 1081) % 2 ** 32 == 1081 <= E.BEYOND_CAPACITY, "a: a 32-bit sum would fit the capacity"
    (member_scan, _, moff), _, _ = E.beyond_int32("b")
    assert sum(lengths[i] for i in member_scan[:moff[STEP]]) == 2 ** 31, "b: 2^31 exactly at the step seam"
    assert sum(lengths[i] for i in member_scan[:moff[STEP - 1]]) < 2 ** 31
    assert np.int64(2 ** 31).astype(np.int32) < 0, "c: negative as int32"
    assert E.beyond_int32("d")[1] == E.INT32_MAX == E.beyond_int32("d")[2], "d: fits int32, reported unclamped"


def test_the_empty_members():
    member_scan, aff, moff = E.empty_members()
    assert np.all(member_scan == E.EMPTY) and moff.tolist() == [0, 2, 2, 5] and len(aff) == 5


def test_the_numeric_scan_reaches_every_edge():
    xy, off = E.numeric_packed()
    member_scan, aff, moff = E.numeric()
    assert len(E.SPECIALS) == 17 and len(xy) == 17 * 17 + 2000 and off.tolist() == [0, len(xy)]
    assert {(float(a), float(b)) for a, b in xy[:289] if a == a and b == b} >= {(0.0, float("inf")), (float("-inf"), 0.0)}
    want = np.float32([0.0, 2.0 ** -149, 1e-39, np.finfo(np.float32).tiny, 1.0, 3e38, np.finfo(np.float32).max, np.inf])
    assert np.array_equal(np.unique(np.abs(E.SPECIALS[:-1])), want) and np.isnan(E.SPECIALS[-1])
    assert np.signbit(E.SPECIALS[:-1]).sum() == 8, "both signs, the zeros too"
    e = np.frexp(xy[289:].astype(np.float64))[1] - 1
    assert e.min() <= -145 and e.max() >= 123, "random exponents over the whole range"
    assert moff.tolist() == [0, E.NUMERIC_MEMBERS] and E.NUMERIC_MEMBERS == 48 and np.all(member_scan == 0)
    for slot in range(4):
        assert np.array_equal(np.sort(aff[:17, slot].view(np.uint32)), np.sort(E.SPECIALS.view(np.uint32))), "every special value in slot %d" % slot
    assert np.array_equal(aff[17:20].view(np.uint32), np.float32([[1, 0, 0, 0], [0, 1, 0, 0], [-0.0, -1, -0.0, 0]]).view(np.uint32))
    big = aff[20:30]
    assert np.all(big[:, 2:] == 0) and np.all(np.abs(big[:, :2]) >= 2.0 ** -30) and np.all(np.abs(big[:, :2]) < 2.0 ** 31)

    cloud, coff = E.numeric_merged()
    assert coff.tolist() == [0, 48 * len(xy)]
    fin = np.isfinite(cloud)
    subnormal = fin & (cloud != 0) & (np.abs(cloud) < E.FLT_MIN)
    zero = cloud == 0
    neg0, pos0 = int((zero & np.signbit(cloud)).sum()), int((zero & ~np.signbit(cloud)).sum())
    finite_in = np.tile(np.isfinite(xy).all(axis=1), 48) & np.repeat(np.isfinite(aff).all(axis=1), len(xy))
    overflow = int((finite_in & ~fin.all(axis=1)).sum())
    nan = int(np.isnan(cloud).any(axis=1).sum())
    fused = R.fused_clouds(xy, off, member_scan, aff, None)
    differ = int(((fused.view(np.uint32) != cloud.view(np.uint32)).any(axis=1) & fin.all(axis=1)).sum())
    print("subnormal outputs %d, -0 %d, +0 %d, overflows %d, NaN points %d, fused differs in %d finite points"
          % (subnormal.sum(), neg0, pos0, overflow, nan, differ))
    assert subnormal.sum() >= 1000
    assert neg0 >= 10 and pos0 >= 100
    assert overflow >= 1000, "points non-finite although point and affine are finite"
    assert nan >= 1000
    assert differ >= 1000, "a contracted kernel would not pass"
    flushed = E.flushed(cloud)
    assert not R.same_cloud(flushed, cloud), "a kernel that flushes subnormal results would not pass"
    assert np.array_equal(np.isfinite(flushed), fin) and R.same_cloud(cloud.copy(), cloud)
    # ... nor one that loses the sign of a zero
    assert not R.same_cloud(np.where(zero, np.float32(0.0), cloud), cloud)


def test_the_shared_inputs_are_read_only():
    for arrays in (E.mini_packed(), E.many_members(), E.many_members_merged(), E.many_targets(), E.many_targets_merged(),
                   E.grid_stride(), E.numeric_packed(), E.numeric(), E.numeric_merged(), E.beyond_int32("a")[0], E.empty_members()):
        for a in arrays:
            assert not a.flags.writeable
            with pytest.raises(ValueError):
                a[...] = 0
