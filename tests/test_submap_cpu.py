"""Submaps without a GPU ("Submaps"): the host helper of the C ABI against its numpy statement, the
membership window, the numpy restatement of the point transform against double precision -- and against the FUSED
evaluation a contracted kernel would give, which must differ on the crafted bag or the GPU test could not tell the two
apart -- and the loop's fallback route through a backend without a device gather."""
import ctypes as C
import inspect
import math

import numpy as np
import pytest

from nautilus_amd import _lib, csm, hostside
from oracle import oracle as O
from oracle.cpu_backend import OracleBackend
from tests import submap_reference as R


def test_member_affines_equal_the_numpy_statement_bit_for_bit():
    rng = np.random.default_rng(5)
    poses = np.concatenate([rng.uniform(-60, 60, (400, 2)), rng.uniform(-7, 7, (400, 1))], axis=1)
    anchor, member = rng.integers(0, 400, 3000), rng.integers(0, 400, 3000)
    anchor[:50] = member[:50]  # a scan in its own frame: exactly (1, 0, 0, 0)? cos^2 + sin^2 rounds to 1 in float
    got = csm.submap_member_affines(poses, anchor, member)
    want = hostside.submap_member_affines(poses, anchor, member)
    assert got.dtype == np.float32 and got.shape == (3000, 4)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got[:50], np.tile(np.float32([1, 0, 0, 0]), (50, 1)))
    # the statement itself: inverse(A(anchor)) * A(member) as 3 x 3 matrices in double
    for m in range(0, 3000, 97):
        A = lambda p: np.array([[math.cos(p[2]), -math.sin(p[2]), p[0]], [math.sin(p[2]), math.cos(p[2]), p[1]], [0, 0, 1]])
        T = np.linalg.inv(A(poses[anchor[m]])) @ A(poses[member[m]])
        assert np.allclose(got[m], [T[0, 0], T[1, 0], T[0, 2], T[1, 2]], rtol=0, atol=2e-5)


def test_member_affines_reject_bad_ids():
    lib = _lib.load()
    poses = np.zeros((4, 3))
    out = np.full((2, 4), 7.0, dtype=np.float32)
    for anchor, member in [([0, 4], [1, 1]), ([0, 1], [-1, 1]), ([0, -2], [1, 1]), ([0, 1], [1, 4])]:
        a, m = np.array(anchor, dtype=np.int32), np.array(member, dtype=np.int32)
        rc = lib.nhip_submap_member_affines(_lib.ptr(poses), 4, _lib.ptr(a), _lib.ptr(m), 2, _lib.ptr(out))
        assert rc == _lib.NHIP_ERR_ARG and len(lib.nhip_last_error()) > 0
        assert np.all(out == 7.0), "nothing is written"
    assert lib.nhip_submap_member_affines(None, 0, None, None, 0, None) == _lib.NHIP_OK


def test_submap_members_clip_at_both_ends_of_the_bag():
    scan, off = hostside.submap_members(10, [0, 1, 5, 8, 9], 2)
    assert off.dtype == scan.dtype == np.int32
    assert off.tolist() == [0, 3, 7, 12, 16, 19]
    assert scan.tolist() == [0, 1, 2, 0, 1, 2, 3, 3, 4, 5, 6, 7, 6, 7, 8, 9, 7, 8, 9]
    scan, off = hostside.submap_members(10, [4, 0, 9], 0)
    assert scan.tolist() == [4, 0, 9] and off.tolist() == [0, 1, 2, 3]
    scan, off = hostside.submap_members(3, [1], 50)
    assert scan.tolist() == [0, 1, 2] and off.tolist() == [0, 3]
    scan, off = hostside.submap_members(10, [], 3)
    assert len(scan) == 0 and off.tolist() == [0]
    with pytest.raises(ValueError):
        hostside.submap_members(10, [10], 1)
    with pytest.raises(ValueError):
        hostside.submap_members(10, [3], -1)


def test_the_crafted_bag_is_what_the_tests_need():
    scans, _ = R.bag()
    assert [len(s) for s in scans] == R.LENGTHS and {0, 1, 63, 64, 65, 255, 256, 257, 1081} <= set(R.LENGTHS)
    assert not np.isfinite(scans[R.NONFINITE]).all() and all(np.isfinite(s).all() for i, s in enumerate(scans) if i != R.NONFINITE)
    member_scan, aff, moff = R.members()
    counts = np.diff(moff).tolist()
    assert counts[0] == 0 and counts[1] == 1 and 2 in counts and 11 in counts
    assert np.array_equal(aff[moff[1]], np.float32([1, 0, 0, 0]))
    assert member_scan[moff[4]] == member_scan[moff[4] + 1], "the same scan twice"
    assert 0 in member_scan[moff[5]:moff[6]] and R.LENGTHS[0] == 0, "a member of 0 points"
    mxy, off = R.merged()
    assert off[0] == 0 and off[-1] == len(mxy) == sum(R.LENGTHS[i] for i in member_scan)
    # merged lengths cross multiples of a gather workgroup and of a gather chunk: inside a target, and the whole cloud
    # spans several chunks with a ragged end
    inside = lambda k: any(off[t] < q * k < off[t + 1] for t in range(len(off) - 1) for q in range(1, off[-1] // k + 1))
    assert inside(R.GATHER_THREADS) and inside(R.GATHER_CHUNK)
    assert off[-1] > 3 * R.GATHER_CHUNK and off[-1] % R.GATHER_CHUNK and off[-1] % R.GATHER_THREADS
    # the seam of two MEMBERS inside a chunk and off a workgroup boundary (the bisection of the member table)
    starts = off[3] + np.cumsum([R.LENGTHS[i] for i in R.TARGET_MEMBERS[3]])[:-1]
    assert np.any(starts % R.GATHER_THREADS != 0)
    # the scan that leaves the grid: most of its merged points are outside, some of the target's are inside
    leave = mxy[off[7]:off[7] + R.LENGTHS[R.LEAVING]]
    assert (np.abs(leave).max(axis=1) >= R.RANGE_M).mean() > 0.5
    assert (np.abs(mxy[off[7]:off[8]]).max(axis=1) < R.RANGE_M).any()
    # non-finite points stay, where they were
    bad = mxy[off[6]:off[6] + R.LENGTHS[R.NONFINITE]]
    assert np.array_equal(np.isfinite(bad).all(axis=1), np.isfinite(scans[R.NONFINITE]).all(axis=1))


def test_submap_clouds_agree_with_double_precision():
    xy, off = R.packed()
    member_scan, aff, moff = R.members()
    mxy, _ = R.merged()
    assert mxy.dtype == np.float32
    o64 = off.astype(np.int64)
    row = 0
    for m, i in enumerate(member_scan):
        p = xy[o64[i]:o64[i + 1]].astype(np.float64)
        c, s, tx, ty = aff[m].astype(np.float64)
        want = np.stack([c * p[:, 0] - s * p[:, 1] + tx, s * p[:, 0] + c * p[:, 1] + ty], axis=1)
        got = mxy[row:row + len(p)].astype(np.float64)
        row += len(p)
        fin = np.isfinite(want).all(axis=1)
        assert np.array_equal(np.isfinite(got).all(axis=1), fin)
        # three roundings per coordinate, each half an ulp of a magnitude below |c x| + |s y| + |t|
        bound = 3 * 2.0 ** -24 * (np.abs(c * p[fin, 0]) + np.abs(s * p[fin, 1]) + abs(tx) + abs(ty) + np.abs(want[fin]).max(axis=1))
        assert np.all(np.abs(got[fin] - want[fin]).max(axis=1) <= bound)
    assert row == len(mxy)
    # the identity member is a copy, bit for bit
    _, moff_pts = R.merged()
    assert np.array_equal(mxy[moff_pts[1]:moff_pts[2]].view(np.uint32), R.bag()[0][8].view(np.uint32))


def test_a_bad_member_id_is_an_empty_member_in_the_restatement():
    xy, off = R.packed()
    scan = np.array([3, -1, len(off) - 1, 4], dtype=np.int32)
    aff = np.tile(np.float32([1, 0, 0, 0]), (4, 1))
    mxy, moff = hostside.submap_clouds(xy, off, scan, aff, np.array([0, 2, 4], dtype=np.int32))
    assert moff.tolist() == [0, R.LENGTHS[3], R.LENGTHS[3] + R.LENGTHS[4]]
    assert np.array_equal(mxy, np.concatenate([R.bag()[0][3], R.bag()[0][4]]))


def test_a_fused_evaluation_differs_in_bits_on_the_crafted_bag():
    """The GPU test compares bits: a kernel whose products were contracted into the sums (one rounding per coordinate) must
    not pass it.  Here: that evaluation differs from the spec on this bag, in many points."""
    xy, off = R.packed()
    member_scan, aff, _ = R.members()
    mxy, _ = R.merged()
    fused = R.fused_clouds(xy, off, member_scan, aff, None)
    assert fused.shape == mxy.shape
    fin = np.isfinite(mxy).all(axis=1)
    differ = (fused.view(np.uint32) != mxy.view(np.uint32)).any(axis=1) & fin
    assert differ.sum() >= 100, "points whose fused evaluation differs: %d" % differ.sum()
    assert not R.same_cloud(fused, mxy) and R.same_cloud(mxy.copy(), mxy)


def test_the_loop_fallback_matches_on_the_merged_clouds():
    """A backend whose match() has no submap_radius (the oracle's) gets the merged clouds as extra scans
    (hostside.submap_extra_scans): its records are oracle.csm_match on each pair's merged cloud."""
    from nautilus_amd import synth
    backend = OracleBackend()
    assert "submap_radius" not in inspect.signature(backend.match).parameters
    bag = synth.SynthBag(60)
    xy, off = csm.pack_scans(bag.scans)
    src = np.array([40, 41, 55, 47], dtype=np.int32)
    tgt = np.array([3, 3, 20, 0], dtype=np.int32)
    a = bag.odom[src, 2] - bag.odom[tgt, 2]
    theta0 = a - 2 * math.pi * np.rint(a / (2 * math.pi))
    xy_m, off_m, tgt_m = hostside.submap_extra_scans(xy, off, bag.odom, tgt, 2)
    assert len(off_m) == len(off) + 3 and tgt_m.tolist() == [61, 61, 62, 60]
    assert np.array_equal(xy_m[:len(xy)], xy) and np.array_equal(off_m[:len(off)], off)
    # target 0's submap is clipped to scans 0 .. 2, target 20's is 18 .. 22
    assert off_m[61] - off_m[60] == sum(len(bag.scans[i]) for i in (0, 1, 2))
    assert off_m[63] - off_m[62] == sum(len(bag.scans[i]) for i in (18, 19, 20, 21, 22))
    m, spec, search = backend.match(xy_m, off_m, src, tgt_m, theta0, 16)
    gs, ss = O.grid_spec(30.0, 0.05, 2.0, 1e-10, 16), O.search_spec(61, 81, 81, math.radians(1.0))
    for i in range(len(src)):
        cloud = xy_m[off_m[tgt_m[i]]:off_m[tgt_m[i] + 1]]
        want = O.csm_match(bag.scans[src[i]], O.grid_build(cloud, gs), gs, theta0[i], ss)
        assert (m["itheta"][i], m["ix"][i], m["iy"][i]) == (want.itheta, want.ix, want.iy), i
        assert m["score"][i] == np.float32(want.score), i


def test_the_loop_refuses_a_radius_that_reaches_the_source():
    import examples.slam_loop as loop
    assert loop.LC_MIN_SEPARATION == 20
    for k in (20, 25, -1):
        with pytest.raises(ValueError):
            loop.run(n_scans=40, lc_submap=k, backend=OracleBackend())
