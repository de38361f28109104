"""Shared inputs of the STEP-SEAM tests of the two other copies of the one-workgroup exclusive scan that carries between
steps of 1024 items (tests/test_step_seams_cpu.py holds their preconditions, tests/test_step_seams_gpu.py runs them), computed
once and read-only.  (The copy in nhip_corr.hip: tests/corr_seams.py, family f; the one in nhip_submap.hip:
tests/submap_edges.py.)

HITL -- hitl_offsets_kernel (nhip_hitl.hip): four scans at once (a-nodes, b-nodes and their points) with four carries, then
the second pass that turns a b-node's `-2 - rank` into `n_a + rank` and adds the a-points to its offset once n_a is known.
hitl_list(name): 1023 .. 2500 scans of 0 .. 12 points, each DESIGNED as a member of line a, of line b, of both (it goes to a)
or of neither: points meant to lie on a line are generated in the world within 2 cm of it (width 5 cm) and taken into the
scan frame in double, points meant to miss are metres away; the threshold is 3 points.  Every list has runs of 80 non-members
across each step seam; "no a" has no a-node at all (n_a = 0: every block id comes from the second pass), "no b" no b-node
(the second pass changes nothing), "late a" its first a-node after the first seam (b-nodes of the first step are renumbered
by a count that only the later steps produce).  hitl_expected(name): hostside.hitl_relevant_poses with the reference's
double width comparison, as tests/hitl_reference.py.

FEATURES -- feat_offsets_kernel and feat_pack_kernel (nhip_feat.hip): features_case(n, cap): n scans of 1 .. 9 points with a
synthesised idx table (n, cap) and counts 0 .. cap, runs of zero counts across each step seam; the scan counts leave the last
workgroup of the pack kernel (four scans, one wave each) with 1, 2 or 3 scans; cap 64 makes lane 63 live.  The expectation
is feature_reference.clouds."""
import functools
from types import SimpleNamespace as NS

import numpy as np

from nautilus_amd import hostside
from tests import feature_reference as FR
from tests import hitl_reference as HR

STEP = 1024                       # scans per step of hitl_offsets_kernel and of feat_offsets_kernel
SCANS_PER_WORKGROUP = 4           # feat_pack_kernel: FT / 64, one wave per scan
LINE_A, LINE_B = HR.LINE_A, HR.LINE_B
WIDTH, THRESHOLD = 0.05, 3
MAX_POINTS = 12
NEITHER, ON_A, ON_B, BOTH = 0, 1, 2, 3
SEAM_RUN = 40                     # non-members on either side of every step seam
HITL_LISTS = {"mixed 1023": 1023, "mixed 1024": 1024, "mixed 1025": 1025, "mixed 2049": 2049, "mixed 2500": 2500,
              "no a 2049": 2049, "no b 2049": 2049, "late a 2500": 2500}
LATE_A_FROM = 1100                # "late a": no a-node before this scan


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def seam_runs(n):
    """[from, to) runs of designed non-members: SEAM_RUN scans on either side of every multiple of 1024 (cut at n; a list of
    1023 ends in such a run)."""
    return [(s - SEAM_RUN, min(s + SEAM_RUN, n)) for s in range(STEP, n + SEAM_RUN, STEP)]


def hitl_kinds(name):
    """The designed membership of every scan of list `name`."""
    n = HITL_LISTS[name]
    rng = np.random.default_rng(sorted(HITL_LISTS).index(name) + 500)
    kind = rng.choice([NEITHER, ON_A, ON_B, BOTH], n, p=[0.4, 0.25, 0.25, 0.1])
    if name.startswith("no a"):
        kind[(kind == ON_A) | (kind == BOTH)] = ON_B
    if name.startswith("no b"):
        kind[kind == ON_B] = ON_A
    if name.startswith("late a"):
        early = np.arange(n) < LATE_A_FROM
        kind[early & ((kind == ON_A) | (kind == BOTH))] = ON_B
    for lo, hi in seam_runs(n):
        kind[lo:hi] = NEITHER
    return kind


@functools.lru_cache(maxsize=None)
def hitl_list(name):
    """-> NS(kind, scans, poses, xy, offsets, on_a, on_b): on_a / on_b the designed numbers of points on each line."""
    kind = hitl_kinds(name)
    rng = np.random.default_rng(len(kind) + 7 * len(name))
    away = [(0.05, 0.35), (0.65, 0.95)]  # parameters at least 0.7 m from the crossing of the two lines
    few, many = (lambda: int(rng.integers(0, THRESHOLD))), (lambda: int(rng.integers(THRESHOLD, 6)))
    scans, poses, on_a, on_b = [], [], [], []
    for k in kind:
        na, nb = (many() if k in (ON_A, BOTH) else few()), (many() if k in (ON_B, BOTH) else few())
        miss = int(rng.integers(0, MAX_POINTS - na - nb + 1))
        if k == NEITHER and rng.random() < 0.2:
            na = nb = miss = 0  # (scans of no point at all among the non-members)
        pose = np.array([rng.uniform(-5, 5), rng.uniform(-5, 5), rng.uniform(-np.pi, np.pi)])
        w = np.concatenate([HR._on(rng, LINE_A, na, away), HR._on(rng, LINE_B, nb, away), rng.uniform([10, -10], [20, 10], (miss, 2))])
        w = w[rng.permutation(len(w))]
        c, s = np.cos(pose[2]), np.sin(pose[2])
        d = w - pose[:2]
        scans.append(np.stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1]], axis=1).astype(np.float32).reshape(-1, 2))
        poses.append(pose)
        on_a.append(na)
        on_b.append(nb)
    xy = np.concatenate(scans).astype(np.float32)
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int32)
    poses = np.array(poses)
    _frozen(xy, offsets, poses, kind)
    return NS(kind=kind, scans=scans, poses=poses, xy=xy, offsets=offsets, on_a=_frozen(np.array(on_a)), on_b=_frozen(np.array(on_b)))


@functools.lru_cache(maxsize=None)
def hitl_expected(name):
    """hostside's selection with the reference's width comparison, in the layout the device packs:
    NS(a_poses, b_poses, n_a, n_b, block_pose, block_offsets, points, scan_block, scan_offset)."""
    s = hitl_list(name)
    a, b = hostside.hitl_relevant_poses(s.poses, s.scans, np.float32(LINE_A), np.float32(LINE_B), line_width=np.float64(WIDTH),
                                        point_threshold=THRESHOLD)
    blocks = list(a) + list(b)
    block_pose = np.array([i for i, _ in blocks], np.int32)
    block_offsets = np.concatenate([[0], np.cumsum([len(p) for _, p in blocks])]).astype(np.int32)
    points = np.concatenate([p for _, p in blocks] + [np.zeros((0, 2), np.float32)]).astype(np.float32).reshape(-1, 2)
    scan_block, scan_offset = -np.ones(len(s.scans), np.int32), np.zeros(len(s.scans), np.int32)
    scan_block[block_pose] = np.arange(len(blocks))
    scan_offset[block_pose] = block_offsets[:-1]
    _frozen(block_pose, block_offsets, points, scan_block, scan_offset)
    return NS(a_poses=a, b_poses=b, n_a=len(a), n_b=len(b), block_pose=block_pose, block_offsets=block_offsets, points=points,
              scan_block=scan_block, scan_offset=scan_offset)


# ------------------------------------------------------------------------------------------------------------ features pack
FEATURE_SCANS = (1023, 1025, 2049, 2050, 2051)
FEATURE_CAPS = (1, 20, 64)


def feature_zero_runs(n):
    """[from, to) runs of scans without features: seam_runs(n), but the last scan (in the pack kernel's partial last
    workgroup) has `cap` of them."""
    return [(lo, min(hi, n - 1)) for lo, hi in seam_runs(n)]


@functools.lru_cache(maxsize=None)
def features_cloud():
    """(xy, normals, offsets) of 2,051 scans of 1 .. 9 points; a launch over n scans takes the first n."""
    rng = np.random.default_rng(91)
    lengths = rng.integers(1, 10, max(FEATURE_SCANS))
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    xy = rng.uniform(-20, 20, (int(offsets[-1]), 2)).astype(np.float32)
    normals = rng.normal(0, 1, xy.shape).astype(np.float32)
    return _frozen(xy, normals, offsets)


@functools.lru_cache(maxsize=None)
def features_case(n, cap):
    """-> NS(idx (n, cap) int32, -1 padded; count (n,) int32; expect: {with normals: (xy, normals or None, offsets)})."""
    xy, normals, offsets = features_cloud()
    rng = np.random.default_rng(1000 * cap + n)
    lengths = np.diff(offsets)[:n]
    count = rng.integers(0, cap + 1, n).astype(np.int32)
    count[rng.random(n) < 0.1] = cap
    for lo, hi in feature_zero_runs(n):
        count[lo:hi] = 0
    count[0], count[n - 1] = cap, cap
    idx = (rng.integers(0, 1 << 30, (n, cap)) % lengths[:, None]).astype(np.int32)
    idx[np.arange(cap)[None, :] >= count[:, None]] = -1
    sub = (xy[:offsets[n]], normals[:offsets[n]], offsets[:n + 1])
    expect = {True: _frozen(*FR.clouds(sub[0], sub[1], sub[2], idx, count)),
              False: _frozen(*[a for a in FR.clouds(sub[0], None, sub[2], idx, count) if a is not None])}
    return NS(idx=_frozen(idx), count=_frozen(count), expect=expect)
