"""Shared inputs of the submap tests (tests/test_submap_cpu.py, tests/test_submap_gpu.py): ONE crafted bag, its targets and
the merged clouds by the numpy restatement of the spec (hostside.submap_clouds; DESIGN.md section 3, "Submaps"), computed once.

The bag: scans of a 4 m x 3 m room seen from poses a few decimetres apart, of 0, 1, 63, 64, 65, 255, 256, 257 and 1081 points
and a few random lengths; one scan with NaN / inf points; one whose points leave the grid of the GPU tests (range 3.2 m) once
its member affine is applied.  The targets: no member; one member under the identity; two; eleven; the same scan twice; a
member without points; the non-finite scan; the scan that leaves the grid.  Merged lengths cross multiples of 256 (a gather
workgroup) and of 2048 (a gather chunk), inside targets and at their seams."""
import functools
import math

import numpy as np

from nautilus_amd import hostside

GATHER_THREADS, GATHER_CHUNK = 256, 2048  # nhip_submap.hip: SUB_T, SUB_CHUNK
RANGE_M, RES, SIGMA, MAX_SHIFT = 3.2, 0.05, 2.0, 12  # S = 128: four 64 x 64 tiles; a 25 x 25 lattice fits the border
LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, 1081, 300, 517, 999, 40, 200, 777, 130]
NONFINITE, LEAVING = 12, 13  # the scan with NaN / inf points, the scan whose member affine moves it out of the grid


def _room(rng, n):
    """n points on the walls of the room, world frame."""
    side = rng.integers(0, 4, n)
    u = rng.uniform(-1.0, 1.0, n)
    x = np.where(side == 0, 2.0, np.where(side == 1, -2.0, 2.0 * u))
    y = np.where(side == 2, 1.5, np.where(side == 3, -1.5, 1.5 * u))
    return np.stack([x, y], axis=1)


def _into_frame(points, pose):
    c, s = math.cos(pose[2]), math.sin(pose[2])
    d = points - pose[:2]
    return np.stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1]], axis=1)


@functools.lru_cache(maxsize=None)
def bag():
    """(scans: list of (n, 2) float32, poses (n_scans, 3) float64)."""
    rng = np.random.default_rng(20240611)
    poses = np.concatenate([rng.uniform(-0.3, 0.3, (len(LENGTHS), 2)), rng.uniform(-0.1, 0.1, (len(LENGTHS), 1))], axis=1)
    scans = [_into_frame(_room(rng, n), poses[i]).astype(np.float32) for i, n in enumerate(LENGTHS)]
    bad = scans[NONFINITE]
    bad[3] = (np.nan, 0.5)
    bad[7] = (1.0, np.inf)
    bad[11] = (-np.inf, np.nan)
    bad[39] = (np.nan, np.nan)
    for s in scans:
        s.setflags(write=False)
    poses.setflags(write=False)
    return scans, poses


# members of every target, by scan index; the affines come from the poses except where given
TARGET_MEMBERS = [
    [],                                      # 0: no member
    [8],                                     # 1: one member, identity affine (= the plain build of scan 8)
    [9, 10],                                 # 2
    [8, 7, 6, 5, 11, 4, 3, 2, 14, 1, 15],    # 3: eleven members: across two chunk seams
    [10, 10],                                # 4: the same scan twice
    [0, 9, 0, 2, 0],                         # 5: members without points first, between and last
    [NONFINITE, 5],                          # 6
    [LEAVING, 4],                            # 7: the first member moved by (2.5, -2.0): most of it leaves the grid
    [11],                                    # 8: under its own pose relative to scan 3
]
TARGET_ANCHOR = [0, 8, 9, 8, 10, 9, 5, 4, 3]


@functools.lru_cache(maxsize=None)
def members():
    """(member_scan int32, member_affine (n, 4) float32, member_offsets int32) of TARGET_MEMBERS."""
    _, poses = bag()
    member_scan = np.array([m for t in TARGET_MEMBERS for m in t], dtype=np.int32)
    member_offsets = np.concatenate([[0], np.cumsum([len(t) for t in TARGET_MEMBERS])]).astype(np.int32)
    anchors = np.repeat(TARGET_ANCHOR, np.diff(member_offsets))
    aff = hostside.submap_member_affines(poses, anchors, member_scan)
    aff[member_offsets[1]] = (1.0, 0.0, 0.0, 0.0)
    aff[member_offsets[7], 2:] += np.float32([2.5, -2.0])
    for a in (member_scan, aff, member_offsets):
        a.setflags(write=False)
    return member_scan, aff, member_offsets


@functools.lru_cache(maxsize=None)
def packed():
    """(xy, offsets) of the bag."""
    from nautilus_amd import csm
    xy, off = csm.pack_scans(bag()[0])
    xy.setflags(write=False)
    off.setflags(write=False)
    return xy, off


@functools.lru_cache(maxsize=None)
def merged():
    """(xy, offsets) of the targets' merged clouds: the restatement of the spec."""
    xy, off = packed()
    mxy, moff = hostside.submap_clouds(xy, off, *members())
    mxy.setflags(write=False)
    moff.setflags(write=False)
    return mxy, moff


@functools.lru_cache(maxsize=None)
def second_members():
    """A second set of submaps with the same number of targets (the rebuild test): other members, other lengths."""
    _, poses = bag()
    lists = [[5, 6], [9], [], [3, 4, 5], [8, 11], [14], [2, 1, 0], [10, 15], [7, 7, 7]]
    assert len(lists) == len(TARGET_MEMBERS)
    member_scan = np.array([m for t in lists for m in t], dtype=np.int32)
    member_offsets = np.concatenate([[0], np.cumsum([len(t) for t in lists])]).astype(np.int32)
    anchors = np.repeat([t[0] if t else 0 for t in lists], np.diff(member_offsets))
    return member_scan, hostside.submap_member_affines(poses, anchors, member_scan), member_offsets


def fused_clouds(xy, offsets, member_scan, member_affine, member_offsets):
    """What a CONTRACTED kernel would give: each coordinate's sum taken in double and rounded to float once."""
    off = np.asarray(offsets, dtype=np.int64)
    parts = []
    aff = np.asarray(member_affine, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for m, i in enumerate(member_scan):
            p = np.asarray(xy[off[i]:off[i + 1]], dtype=np.float64)
            c, s, tx, ty = aff[m]
            parts.append(np.stack([c * p[:, 0] + (-s) * p[:, 1] + tx, s * p[:, 0] + c * p[:, 1] + ty], axis=1).astype(np.float32))
    return np.concatenate(parts)


def same_cloud(got, want):
    """The issue's comparison of two float32 clouds: equal bits wherever `want` is finite, non-finite at the same places."""
    got, want = np.asarray(got, dtype=np.float32).reshape(-1), np.asarray(want, dtype=np.float32).reshape(-1)
    if got.shape != want.shape:
        return False
    fin = np.isfinite(want)
    return bool(np.array_equal(np.isfinite(got), fin) and np.array_equal(got.view(np.uint32)[fin], want.view(np.uint32)[fin]))
