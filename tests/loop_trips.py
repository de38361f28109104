"""Crafted inputs that send the kernels' loops round a second time, with the smallest data that crosses each seam: the carries
of K8's hitl_offsets_kernel beyond 1024 scans, K16's and K21's grid-stride loops over scans beyond 4096 workgroups (the LDS words
of a workgroup's first scan must not show in its second), the 1024-row steps of K20's and K21's row scans, the 64-node steps of
K21's row kernels, K20's grid-stride over queries beyond 16384 and its 256-row trips of a window, the tiles of eight queries in
K21's cost kernel when a chunk is no multiple of eight -- and the sector count of K16 and K21 on every sector boundary.

Nothing here computes an expected value: those come from hostside (K8) and from the references (place_reference,
localize_reference, rangesig_reference).  tests/test_loop_trips_cpu.py asserts that each case holds what it is for."""
import functools
import math
from types import SimpleNamespace

import numpy as np

from nautilus_amd import hostside
from tests import localize_reference as LR
from tests import place_reference as PR
from tests import rangesig_reference as RR

F = np.float32

# ---------------------------------------------------------------- K8: more than 1024 scans
HITL = dict(line_a=(0.0, 0.0, 10.0, 0.0), line_b=(0.0, 5.0, 10.0, 5.0), width=0.05, threshold=3)
HITL_CASES = (("b then a", 1025), ("b then a", 2050), ("a then b", 1025), ("a then b", 2050), ("mix", 1023), ("mix", 1024), ("mix", 1025),
              ("mix", 2050))


def hitl_membership(name, k):
    """what scan k is to be: "a" (an a-node), "b" or "-" (neither).  "b then a": no a-node among scans 0 .. 1023, so the second
    pass adds an n_a and a pts_a that the first step of the loop did not know; "a then b": its mirror image."""
    if name == "mix":
        return "ab-b-aa-b"[(k * 5 + k // 1024) % 9]
    first, second = ("b", "a") if name == "b then a" else ("a", "b")
    if k < 1024:
        return first if k % 3 else "-"
    return (second, first, "-", second)[k % 4]


@functools.lru_cache(maxsize=None)
def hitl_table(name, n_scans):
    """NS(scans, xy, offsets, poses) as hitl_reference.scans(): scans of 0 .. 12 points at the identity pose; a point is on line a
    (y = 0.01), on line b (y = 5.01) or on neither (y = 2.5)."""
    rng = np.random.default_rng(1024 + n_scans + len(name))
    thr = HITL["threshold"]
    scans = []
    for k in range(n_scans):
        m = hitl_membership(name, k)
        if m == "a":
            na, nb = int(rng.integers(thr, 9)), int(rng.integers(0, 5))    # (enough on a: the b-points do not count)
        elif m == "b":
            na, nb = int(rng.integers(0, thr)), int(rng.integers(thr, 9))
        else:
            na, nb = int(rng.integers(0, thr)), int(rng.integers(0, thr))
        no = int(rng.integers(0, 13 - na - nb)) if k % 7 else 0
        if m == "-" and k % 5 == 0:
            na = nb = no = 0  # an empty scan
        y = np.concatenate([np.full(na, 0.01), np.full(nb, 5.01), np.full(no, 2.5)])
        pts = np.stack([rng.uniform(0.5, 9.5, len(y)), y], axis=1)
        scans.append(rng.permutation(pts).astype(F).reshape(-1, 2))
    off = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int32)
    return SimpleNamespace(scans=scans, xy=np.concatenate(scans).astype(F).reshape(-1, 2), offsets=off, poses=np.zeros((n_scans, 3)))


def hitl_expected(table):
    """(class bytes, counts (2 n), scan_block (n), scan_offset (n), totals (3)) as hostside classifies: the blocks are all
    a-nodes in scan order, then all b-nodes; a scan that is neither has block -1 and offset 0."""
    la, lb, w, thr = HITL["line_a"], HITL["line_b"], HITL["width"], HITL["threshold"]
    n = len(table.scans)
    a_poses, b_poses = hostside.hitl_relevant_poses(table.poses, table.scans, la, lb, w, thr)
    cls, cnt = np.zeros(len(table.xy), np.uint8), np.zeros(2 * n, np.int32)
    for k, pts in enumerate(table.scans):  # (identity poses: the world points are the scan's)
        on_a = hostside.distance_to_line_segment_f32(pts, la) <= F(w)
        on_b = ~on_a & (hostside.distance_to_line_segment_f32(pts, lb) <= F(w))
        cls[table.offsets[k]:table.offsets[k + 1]] = on_a.astype(np.uint8) + 2 * on_b.astype(np.uint8)
        cnt[2 * k:2 * k + 2] = (on_a.sum(), on_b.sum())
    blk, so = np.full(n, -1, np.int32), np.zeros(n, np.int32)
    at = 0
    for b, (k, pts) in enumerate(a_poses + b_poses):
        blk[k], so[k] = b, at
        at += len(pts)
    return cls, cnt, blk, so, np.array([len(a_poses), len(b_poses), at], np.int32)


# ---------------------------------------------------------------- K16 and K21: more than 4096 scans
N_MANY_SCANS = (4096, 4097, 4200)


@functools.lru_cache(maxsize=None)
def many_scans(n=4200, reach=28.0):
    """(xy, offsets) of n scans of 0 .. 3 points.  Scan s and scan s + 4096 -- the same workgroup's first and second trip -- differ in
    their number of points, in their sectors and in their ranges, so a word left in LDS by the first would show in the second."""
    scans = []
    for s in range(n):
        trip = s // 4096
        pts = []
        for i in range((s + trip) % 4):
            sector = (7 * s + 13 * i + 11 * trip) % 64
            a = 2.0 * math.pi * (sector + 0.5) / 64
            r = reach * (1 + (s + 3 * i + 5 * trip) % 9) / 10.0
            pts.append((r * math.cos(a), r * math.sin(a)))
        scans.append(np.array(pts, F).reshape(-1, 2))
    off = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int32)
    return np.concatenate(scans).astype(F), off


@functools.lru_cache(maxsize=None)
def many_scans_descriptors():
    xy, off = many_scans()
    return PR.describe(xy, off, *PR.make_tables(10, 30.0))


@functools.lru_cache(maxsize=None)
def many_scans_signatures():
    xy, off = many_scans()
    return RR.scan_signatures(xy, off, RR.make_spec())


# ---------------------------------------------------------------- K20: rows beyond 1024, queries beyond 16384, sides at 256
TALL_MAPS = ((5, 1023), (5, 1024), (5, 1025), (5, 2049), (5, 3073), (65, 2049))


@functools.lru_cache(maxsize=None)
def tall_map(width, height):
    """(grid int8, spec, origins): rows of 0 .. 5 occupied cells, occupied rows on both sides of 1024 and of 3072, a run of empty
    rows across 2048; origins of windows (side 8, then side 41 in a second spec) whose rows straddle 1024 and 2048"""
    rng = np.random.default_rng(width * 10000 + height)
    grid = rng.choice(np.array([0, -1, 99, 50], np.int8), (height, width))
    for r in range(height):
        k = int(rng.integers(0, 6))
        if r in (1022, 1023, 1024, 1025, 3071, 3072):
            k = max(k, 1)
        if 2044 <= r < 2053:
            k = 0
        grid[r, rng.permutation(width)[:k]] = 100
    spec = LR.make_spec(width=width, height=height, cell_x0=-2, cell_y0=-1000, side=8)
    ys = [y for y in (1020, 1023, 1024, 1027, 2040, 2047, 2048, 2052, 3070, 0, 512) if y < height + 4]
    origins = np.array([(x - 2, y - 1000) for y in ys for x in (0, 2, width - 1)], np.int32)
    return grid, spec, origins


def with_side(spec, side):
    s = LR.make_spec(**{f: getattr(spec, f) for f in LR.FIELDS})
    s.side = side
    return s


N_MANY_QUERIES = (16384, 16385, 16700)


@functools.lru_cache(maxsize=None)
def many_queries():
    """(grid, spec, origins (16700, 2)): side 3 on the 17 x 130 map.  Query q and query q - 16384 -- one workgroup's trips -- lie at
    different places; about one in five lies off the map (an empty window)."""
    _, grid, spec, _ = LR.many_queries_case()
    spec = with_side(spec, 3)
    q = np.arange(16700)
    x = spec.cell_x0 + (q * 5 + q // 16384 * 3) % 21 - 2
    y = spec.cell_y0 + (q * 11 + q // 16384 * 17) % 134 - 2
    return grid, spec, np.stack([x, y], axis=1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def many_queries_windows():
    grid, spec, origins = many_queries()
    return LR.map_windows(grid, spec, origins)


@functools.lru_cache(maxsize=None)
def wide_window_map():
    """(grid 130 x 65, spec, origins): for sides 255, 256 and 257 -- one trip of 256 window rows, exactly one, and one row more"""
    grid = LR.value_map(65, 130, 256)
    spec = LR.make_spec(width=65, height=130, cell_x0=-30, cell_y0=-60, side=256)
    origins = np.array([(0, 0), (0, 67), (0, 68), (0, 69), (2, -58), (-20, -187), (-20, -188), (-20, -189), (40, 300), (1, 197), (1, 198)], np.int32)
    return grid, spec, origins


# ---------------------------------------------------------------- K21: lattice rows beyond 1024, rows of 64 nodes and more
def lattice_map(ni, nj, stride, seed):
    """(grid, spec) with ni x nj lattice nodes of the stride: rows of 0 .. 3 anchors (free node cells), the rest of the nodes and
    of the cells walls, unknown or neither; anchors in the rows on both sides of every multiple of 1024"""
    rng = np.random.default_rng(seed)
    width, height, h = ni * stride, nj * stride, stride // 2
    grid = rng.choice(np.array([100, -1, 50, 0], np.int8), (height, width))
    nodes = rng.choice(np.array([100, -1, 50], np.int8), (nj, ni))
    for j in range(nj):
        k = int(rng.integers(0, 4)) if ni < 64 else int(rng.integers(0, ni + 1))
        if j % 1024 in (1023, 0, 1):
            k = max(k, 1)
        nodes[j, rng.permutation(ni)[:k]] = 0
    if ni >= 64:  # a full row, an empty one, and one with the last node of a 64-node step, the first of the next and the row's last
        nodes[0], nodes[1], nodes[2] = 0, 100, 100
        nodes[2, [63, min(64, ni - 1), ni - 1]] = 0
    grid[h::stride, h::stride][:nj, :ni] = nodes
    spec = RR.make_spec(width=width, height=height, stride=stride, rays_per_sector=1, max_ray_cells=1, cell_x0=-3, cell_y0=7)
    return grid, spec


@functools.lru_cache(maxsize=None)
def lattice_cases():
    """[(name, grid, spec)]: nj at and around 1024 and 2048 with strides 1 and 3 (3 .. 8 nodes a row), ni at and around 64 and 128
    in a map 5 rows high"""
    out = []
    for t, nj in enumerate((1023, 1024, 1025, 2049)):
        for stride in (1, 3):
            ni = 3 + (2 * t + stride) % 6
            out.append(("nj %d stride %d" % (nj, stride), *lattice_map(ni, nj, stride, 100 * nj + stride)))
    for ni in (64, 65, 128, 129):
        out.append(("ni %d" % ni, *lattice_map(ni, 5, 1, ni)))
    return out


@functools.lru_cache(maxsize=None)
def lattice_results():
    return {name: RR.anchors_and_signatures(grid, spec) for name, grid, spec in lattice_cases()}


# ---------------------------------------------------------------- K21: chunks of query rows that are no multiple of eight
MATCH_A, MATCH_QUERIES, MATCH_CHUNK_ROWS = 65, (7, 8, 9, 16, 25), (3, 8, 9, 12)


def key_row_bytes(n_anchors):
    """a row of the key workspace: four bytes an anchor, the anchors rounded up to 64 (nhip_host_rangesig.hip)"""
    return 4 * ((max(n_anchors, 1) + 63) // 64 * 64)


def chunk_rows(workspace_bytes, n_anchors):
    """the rows of queries one launch of the cost kernel takes: what the workspace holds (nhip_host_rangesig.hip)"""
    return min(workspace_bytes // key_row_bytes(n_anchors), 1 << 18)


@functools.lru_cache(maxsize=None)
def match_case():
    """(query_sig (25, 64), map_sig (65, 64), anchors, spec, records (25, K, 4)): the records of the first Q queries are those of a
    call with Q queries (a query's records depend on no other query)"""
    rng = np.random.default_rng(65)
    qs = rng.integers(0, 256, (max(MATCH_QUERIES), 64)).astype(np.uint8)
    qs[rng.random(qs.shape) < 0.3] = 255
    qs[5] = 255          # no sector: no record
    qs[13, 6:] = 255     # six sectors, below min_sectors
    ms = rng.integers(0, 256, (MATCH_A, 64)).astype(np.uint8)
    an = RR.lattice_anchors(MATCH_A)
    spec = RR.make_spec(width=10, height=7, stride=1, min_sep=1)
    return qs, ms, an, spec, RR.match(qs, ms, an, spec)[0]


# ---------------------------------------------------------------- the sector count on its boundaries
def boundary_points():
    """[(x, y, j, kind)]: for every boundary direction j = 1 .. 31 and e in {-3, 0, 5} the point p = 2^e DIRS[j] -- both products
    of the sector test are then equal and their difference is exactly 0 -- its negation, and both with y one float up and
    one float down.  kind 0: on the boundary; +1 / -1: y moved up / down."""
    out = []
    for j in range(1, 32):
        for e in (-3, 0, 5):
            x, y = F(RR.DIRS[j][0] * F(2.0 ** e)), F(RR.DIRS[j][1] * F(2.0 ** e))
            for s in (1, -1):
                px, py = F(s * x), F(s * y)
                out += [(px, py, j, 0), (px, np.nextafter(py, F(np.inf)), j, 1), (px, np.nextafter(py, F(-np.inf)), j, -1)]
    return out


def boundary_scans():
    """(xy, offsets): a scan per point of boundary_points(), so every point's sector shows in its scan's signature / descriptor"""
    pts = boundary_points()
    return np.array([(p[0], p[1]) for p in pts], F), np.arange(len(pts) + 1, dtype=np.int32)
