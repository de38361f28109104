"""Inputs for the HITL kernels (nhip_hitl.hip, resid_p2l_normal_eq_kernel) and what the host says about them.

SELECTION.  scans() is one set of 27 scans with their poses; CONFIGS are the calls made on it: (line a, line b, width,
threshold).  The expectation of a call is hostside.hitl_relevant_poses with the width as np.float64 -- the reference's
comparison of a float distance with CONFIG_DOUBLE hitl_line_width (a Python-float width compares in float under numpy 2
and admits d == float32(w), which the reference rejects).  Points meant to lie on a line are generated in the world within
2 cm of it and taken into the scan frame in double, so the float round trip (1e-6) cannot move them across the 5 cm width;
points meant to miss are metres away.  tests/test_hitl_cpu.py checks with hostside alone that every category named below
occurs.

NORMAL EQUATIONS.  ne_blocks(): the blocks of resid_reference.segments() plus blocks of NE_SIZES points tiled from its first
'rotated' case, with the 28 sums of resid_reference.p2l_reference's longdouble rows and the sums of their magnitudes.

K_P2L_NE.  The bound of a sum over n rows is (K + n) 2**-53 (sum of magnitudes).  K covers what the terms themselves carry:
a product of two Jacobian entries carries both entries' errors, about twice resid_reference.K_P2L's single values.  It is
measured on the CPU, never from a kernel (tests/test_hitl_cpu.py): the oracle's Jet rows, their 28 sums formed in double in
row order, against the reference sums, block by block over resid_reference.segments(); the figure is the worst of
(ratio - n) -- what is left for K once the n of the summation is taken out -- and of the ratio of the same rows summed in
longdouble (no summation error at all); K = resid_reference.k_rule(figure).
    measured: ratio - n at most -8.98 (double sums: the ratios themselves stay below 0.09), ratio 0.031 (longdouble sums)
    ->   k_rule(0.031) = 4 (the rule's floor)   ->   K_P2L_NE = 4
"""
import functools
import math
from types import SimpleNamespace as NS

import numpy as np

from nautilus_amd import hostside
from tests import resid_reference as RR

LD = RR.LD
K_P2L_NE = 4

# ------------------------------------------------------------------------------------------------ selection
LINE_A, LINE_B = (0.0, 0.0, 4.0, 3.0), (0.0, 3.0, 4.0, 0.0)          # oblique, crossing at (2, 1.5)
FLAT, POINT_B = (0.0, 0.0, 2.0, 0.0), (1.5, 1.0, 1.5, 1.0)           # the width-boundary recipe's segment; a zero-length line b
QUIRK_H, QUIRK_V = (-1.0, 0.01, 4.0, 0.01), (0.01, -2.0, 0.01, 5.0)  # axis-aligned, 1 cm off the axis: signed distances of
#   centimetres round coarser than the ends' own coordinate, so IsBetween(projection, 0.01, 0.01) holds only when two roundings cancel
FAR_A, FAR_B = (100.0, 100.0, 101.0, 101.0), (200.0, 100.0, 201.0, 100.0)
W5, W25 = np.float32(0.05), np.float32(0.25)
SCAN_LENGTHS = (0, 1, 9, 10, 11, 63, 64, 65, 127, 128, 129, 1081, 1089, 2500)

# name -> (line a, line b, width, threshold)
CONFIGS = {
    "oblique w0.05 t10": (LINE_A, LINE_B, 0.05, 10),
    "oblique w0.25 t10": (LINE_A, LINE_B, 0.25, 10),
    "oblique w0.05 t1": (LINE_A, LINE_B, 0.05, 1),
    "flat + zero-length b w0.05 t1": (FLAT, POINT_B, 0.05, 1),
    "flat + zero-length b w0.25 t10": (FLAT, POINT_B, 0.25, 10),
    "horizontal then vertical w0.25 t10": (QUIRK_H, QUIRK_V, 0.25, 10),
    "vertical then horizontal w0.05 t10": (QUIRK_V, QUIRK_H, 0.05, 10),
    "nothing selected": (FAR_A, FAR_B, 0.05, 10),
}


def _on(rng, seg, n, ranges, spread=0.02):
    """n world points within `spread` of the segment, at parameters drawn from `ranges` (pairs of t in [0, 1])."""
    x0, y0, x1, y1 = seg
    r = np.array(ranges)[rng.integers(0, len(ranges), n)]
    t = rng.uniform(r[:, 0], r[:, 1])
    ln = math.hypot(x1 - x0, y1 - y0)
    nx, ny = -(y1 - y0) / ln, (x1 - x0) / ln
    d = rng.uniform(-spread, spread, n)
    return np.stack([x0 + t * (x1 - x0) + d * nx, y0 + t * (y1 - y0) + d * ny], axis=1)


@functools.lru_cache(maxsize=None)
def scans():
    """-> NS(scans: list of (k, 2) float32, poses (n, 3), xy, offsets, plan: per scan (on a, on b, at the crossing) under the
    first configuration, boundary: index of the heading-0 scan at the origin, quirk: index of the heading-0 scan off it)."""
    rng = np.random.default_rng(479)
    away = [(0.05, 0.35), (0.65, 0.95)]                                # parameters at least 0.7 m from the crossing
    # (length, on a, on b, at the crossing): the first fourteen have the lengths of SCAN_LENGTHS
    plan = [(0, 0, 0, 0), (1, 1, 0, 0), (9, 9, 0, 0), (10, 10, 0, 0), (11, 11, 0, 0),
            (63, 9, 10, 0),        # 9 on a, 10 on b: a b-block, the a-points dropped
            (64, 9, 9, 0),         # 9 on each: absent
            (65, 12, 15, 0),       # enough on both: an a-block with its a-points only
            (127, 0, 11, 0), (128, 0, 9, 0),
            (129, 0, 5, 20),       # 20 points near both lines: on a
            (1081, 200, 100, 0), (1089, 0, 0, 0), (2500, 300, 0, 0),
            (40, 10, 10, 0), (300, 11, 0, 0), (300, 0, 10, 0), (77, 3, 30, 0), (512, 256, 0, 0), (700, 0, 0, 12),
            (20, 0, 0, 0), (256, 64, 64, 0), (257, 0, 129, 0), (1000, 9, 0, 1)]
    assert tuple(p[0] for p in plan[:len(SCAN_LENGTHS)]) == SCAN_LENGTHS
    out, poses = [], []
    for length, na, nb, nc in plan:
        pose = np.array([rng.uniform(-5, 5), rng.uniform(-5, 5), rng.uniform(-math.pi, math.pi)])
        w = np.concatenate([_on(rng, LINE_A, na, away), _on(rng, LINE_B, nb, away),
                            np.array([2.0, 1.5]) + rng.uniform(-0.01, 0.01, (nc, 2)),
                            rng.uniform([10, -10], [20, 10], (length - na - nb - nc, 2))])
        w = w[rng.permutation(len(w))]
        c, s = math.cos(pose[2]), math.sin(pose[2])
        d = w - pose[:2]
        out.append(np.stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1]], axis=1).astype(np.float32).reshape(-1, 2))
        poses.append(pose)
    # the width boundary: pose (0, 0, 0), segment (0, 0) - (2, 0), float distances of exactly float32(w) and one step either
    # side; non-finite points; clusters on FLAT, on the zero-length line b and beside QUIRK_V
    up, dn = (lambda v: np.nextafter(v, np.float32(1))), (lambda v: np.nextafter(v, np.float32(0)))
    edge = np.array([[1, W5], [1, dn(W5)], [1, up(W5)], [1, W25], [1, dn(W25)], [1, up(W25)]], np.float32)
    bad = np.array([[np.nan, 0.5], [np.inf, 0.0], [0.5, -np.inf], [np.nan, np.nan], [-np.inf, np.inf], [1.0, np.nan]], np.float32)
    boundary = len(out)
    out.append(np.concatenate([edge, bad, _on(rng, FLAT, 12, [(0.05, 0.95)], 0.01),
                               np.array(POINT_B[:2]) + rng.uniform(-0.02, 0.02, (12, 2)),
                               rng.uniform([5, 5], [9, 9], (7, 2))]).astype(np.float32))
    poses.append(np.zeros(3))
    # heading exactly 0, off the origin: points up to 0.24 m either side of the two axis-aligned segments
    quirk = len(out)
    pose = np.array([0.1, -0.2, 0.0])
    w = np.concatenate([_on(rng, QUIRK_H, 300, [(0.05, 0.45), (0.55, 0.95)], 0.24), _on(rng, QUIRK_V, 300, [(0.05, 0.3), (0.4, 0.95)], 0.24)])
    out.append((w - pose[:2]).astype(np.float32))
    poses.append(pose)
    # ... and one more heading-0 node whose points lie beside the vertical segment only
    out.append((_on(rng, QUIRK_V, 64, [(0.5, 0.9)], 0.04) - [2.0, 1.0]).astype(np.float32))
    poses.append(np.array([2.0, 1.0, 0.0]))
    assert len(out) <= 64
    xy = np.concatenate(out).astype(np.float32)
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in out])]).astype(np.int32)
    xy.setflags(write=False)
    return NS(scans=out, poses=np.array(poses), xy=xy, offsets=offsets, plan=plan, boundary=boundary, quirk=quirk)


@functools.lru_cache(maxsize=None)
def expected(name):
    """hostside's selection of configuration `name` with the reference's width comparison, in the layout the device packs:
    NS(a_poses, b_poses, n_a, n_b, block_pose, block_offsets, points)."""
    la, lb, w, thr = CONFIGS[name]
    s = scans()
    with np.errstate(invalid="ignore", over="ignore"):
        a, b = hostside.hitl_relevant_poses(s.poses, s.scans, np.float32(la), np.float32(lb), line_width=np.float64(w), point_threshold=thr)
    blocks = list(a) + list(b)
    return NS(a_poses=a, b_poses=b, n_a=len(a), n_b=len(b), block_pose=np.array([i for i, _ in blocks], np.int32),
              block_offsets=np.concatenate([[0], np.cumsum([len(p) for _, p in blocks])]).astype(np.int32),
              points=np.concatenate([p for _, p in blocks]).astype(np.float32).reshape(-1, 2) if blocks else np.zeros((0, 2), np.float32))


def classes(name, scan):
    """(on a, on b) masks of one scan under configuration `name`, by hostside's distance with the reference's comparison."""
    la, lb, w, _ = CONFIGS[name]
    s = scans()
    pts, pose = s.scans[scan], s.poses[scan]
    f = np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        c, sn, tx, ty = f(np.cos(pose[2])), f(np.sin(pose[2])), f(pose[0]), f(pose[1])
        wpt = np.stack([c * pts[:, 0] - sn * pts[:, 1] + tx, sn * pts[:, 0] + c * pts[:, 1] + ty], axis=1).astype(f)
        on_a = hostside.distance_to_line_segment_f32(wpt, f(la)) <= np.float64(w)
        on_b = ~on_a & (hostside.distance_to_line_segment_f32(wpt, f(lb)) <= np.float64(w))
    return on_a, on_b


# ------------------------------------------------------------------------------------------------ normal equations
TRIP = 1024                                           # points of one trip of the kernel's row loop: 256 lanes x 4 loads
NE_SIZES = (0, 1, 63, 64, 65, 255, 256, 257, TRIP, TRIP + 1, 2 * TRIP)


def ne_of_rows(res, jp, jl, dtype=LD):
    """The 28 numbers of one point-to-line block from its rows: one residual per point, J = [jp | jl]."""
    if len(res) == 0:
        return np.zeros(28, dtype)
    J = np.concatenate([np.asarray(jp, dtype), np.asarray(jl, dtype)], axis=1)[:, None, :]
    return RR.normal_equations(np.asarray(res, dtype)[:, None], J)


def ne_of_rows_in_order(res, jp, jl):
    """The same sums formed in double, one row after the other (what a sequential host loop computes)."""
    acc = np.zeros(28)
    J = np.concatenate([jp, jl], axis=1)
    iu = np.triu_indices(6)
    for r, j in zip(res, J):
        acc[:21] += np.outer(j, j)[iu]
        acc[21:27] += j * r
        acc[27] += r * r
    return acc


@functools.lru_cache(maxsize=None)
def ne_blocks():
    """-> NS(segs, pts, offsets, bpose, bline, poses, lines, sizes, ne, m_ne): every case of RR.segments() as a block with its
    own pose and line pose, then one block per size of NE_SIZES on the first 'rotated' case's segment, pose and line pose,
    its points tiled; ne / m_ne (n_blocks, 28) longdouble from RR.p2l_reference's rows and magnitudes."""
    cs = RR.segments()
    rot = next(c for c in cs if c.tag == "rotated")
    blocks = [(c.seg, c.pts, c.pose, c.line, c.ref) for c in cs]
    for n in NE_SIZES:
        pts = np.resize(rot.pts, (n, 2)).astype(np.float32)
        blocks.append((rot.seg, pts, rot.pose, rot.line, RR.p2l_reference(rot.seg, pts, rot.pose, rot.line) if n else None))
    sizes = np.array([len(b[1]) for b in blocks])
    ne, m_ne = np.zeros((len(blocks), 28), LD), np.zeros((len(blocks), 28), LD)
    for k, (_, _, _, _, ref) in enumerate(blocks):
        if ref is not None and sizes[k]:
            ne[k], m_ne[k] = ne_of_rows(ref.res, ref.jp, ref.jl), ne_of_rows(ref.m_res, ref.m_jp, ref.m_jl)
    pts = np.concatenate([b[1] for b in blocks]).astype(np.float32)
    pts.setflags(write=False)
    return NS(segs=np.stack([b[0] for b in blocks]).astype(np.float32), pts=pts,
              offsets=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), bpose=np.arange(len(blocks), dtype=np.int32),
              bline=np.arange(len(blocks), dtype=np.int32), poses=np.stack([b[2] for b in blocks]), lines=np.stack([b[3] for b in blocks]),
              sizes=sizes, ne=ne, m_ne=m_ne, n_cases=len(cs))
