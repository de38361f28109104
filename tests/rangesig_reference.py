"""The slow, obviously-right statement of the range signatures ("Range signatures"; the device form is K21,
nautilus_amd/csrc/nhip_rangesig.hip), and the crafted inputs its tests share.  Written from the spec's text and differently
from the kernels and from hostside on purpose: the tables from math.cos / math.sin / math.sqrt and python's round(), a loop per
anchor, per ray and per step with rdiv as (2 a + n) // (2 n) on python integers, a scan's point at a time in numpy float32
scalars, a cost per (query, anchor, shift), the selection as the greedy walk of a sorted list.  No code is shared with the
product.

A spec is anything with the fields of nhip_rangesig_spec_t as attributes (a ctypes struct, or make_spec() below).
"""
import functools
import math
from types import SimpleNamespace

import numpy as np

FIELDS = ("res", "unit", "cell_x0", "cell_y0", "width", "height", "occ_min", "free_max", "stride", "max_ray_cells", "rays_per_sector",
          "top_k", "min_sep", "min_sectors", "flags", "reserved")
F = np.float32


def make_spec(**kw):
    s = SimpleNamespace(res=0.05, unit=0.125, cell_x0=0, cell_y0=0, width=1, height=1, occ_min=100, free_max=0, stride=10,
                        max_ray_cells=600, rays_per_sector=4, top_k=5, min_sep=2, min_sectors=8, flags=0, reserved=0)
    for k, v in kw.items():
        assert k in FIELDS, k
        setattr(s, k, v)
    return s


# ---------------------------------------------------------------- item 2: tables
def ray_table(spec):
    """[(dx, dy, n, scale)] for t = 0 .. 64 m - 1."""
    m, L = int(spec.rays_per_sector), int(spec.max_ray_cells)
    w = 2.0 * math.pi / 64
    out = []
    for t in range(64 * m):
        phi = (t + 0.5) * w / m
        dx, dy = round(L * math.cos(phi)), round(L * math.sin(phi))  # (round(): half to even, as lrint)
        n = max(abs(dx), abs(dy))
        scale = round(65536.0 * math.sqrt(float(dx * dx + dy * dy)) * float(spec.res) / (float(n) * float(spec.unit)))
        out.append((dx, dy, n, scale))
    return out


def edge_table(spec):
    """edge2[0 .. 254] as float32 scalars, [0] = 0."""
    out = [F(0)]
    for k in range(1, 255):
        e = F(float(spec.unit) * k)
        out.append(F(e * e))
    return out


DIRS = [(F(math.cos(2.0 * math.pi * j / 64)), F(math.sin(2.0 * math.pi * j / 64))) for j in range(32)]


# ---------------------------------------------------------------- items 1 and 3: anchors and map signatures
def anchors(grid, spec):
    """[(cx, cy, i, j)] in row-major order (j, then i)."""
    g = np.asarray(grid, dtype=np.int8).reshape(spec.height, spec.width).tolist()
    st, h = int(spec.stride), int(spec.stride) // 2
    out, nodes = [], 0
    j = 0
    while j * st + h < spec.height:
        i = 0
        while i * st + h < spec.width:
            nodes += 1
            if 0 <= g[j * st + h][i * st + h] <= spec.free_max:
                out.append((i * st + h, j * st + h, i, j))
            i += 1
        j += 1
    return out, nodes


def map_signatures(grid, spec, anchor_list, rays=None):
    """(sig uint8 (A, 64), [rays ended on a wall, in unknown, outside or at n])."""
    g = np.asarray(grid, dtype=np.int8).reshape(spec.height, spec.width).tolist()
    rays = ray_table(spec) if rays is None else [tuple(int(v) for v in r) for r in rays]
    m = int(spec.rays_per_sector)
    sig = np.full((len(anchor_list), 64), 255, np.uint8)
    ends = [0, 0, 0]
    for a, (cx, cy, _, _) in enumerate(anchor_list):
        for t, (dx, dy, n, scale) in enumerate(rays):
            val, end = 255, 2
            for k in range(1, n + 1):
                x, y = cx + (2 * k * dx + n) // (2 * n), cy + (2 * k * dy + n) // (2 * n)
                if not (0 <= x < spec.width and 0 <= y < spec.height):
                    break
                v = g[y][x]
                if v < 0:
                    end = 1
                    if spec.flags & 1:  # (NHIP_RANGESIG_UNKNOWN_STOPS)
                        val = min(254, (k * scale) >> 16)
                    break
                if v >= spec.occ_min:
                    val, end = min(254, (k * scale) >> 16), 0
                    break
            ends[end] += 1
            sig[a, t // m] = min(int(sig[a, t // m]), val)
    return sig, ends


def anchors_and_signatures(grid, spec, rays=None, max_anchors=None):
    """(anchors int32 (A, 4), sig uint8 (A, 64), stats int64 (8,): words 0 - 5) -- of the first max_anchors anchors."""
    found, nodes = anchors(grid, spec)
    kept = found if max_anchors is None else found[:max_anchors]
    sig, ends = map_signatures(grid, spec, kept, rays)
    stats = np.array([nodes, len(found), len(found) - len(kept)] + ends + [0, 0], np.int64)
    return np.array(kept, np.int32).reshape(-1, 4), sig, stats


# ---------------------------------------------------------------- item 4: scan signatures
def point_sector(x, y):
    neg = y < 0 or (y == 0 and x < 0)
    u, v = (F(-x), F(-y)) if neg else (x, y)
    sector = 32 if neg else 0
    for j in range(1, 32):
        sector += bool(F(F(DIRS[j][0] * v) - F(DIRS[j][1] * u)) >= 0)
    return sector


def scan_signatures(xy, offsets, spec):
    p = np.asarray(xy, dtype=F).reshape(-1, 2)
    edge2 = edge_table(spec)
    sig = np.full((len(offsets) - 1, 64), 255, np.uint8)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(len(offsets) - 1):
            b, e = int(offsets[s]), int(offsets[s + 1])
            if b < 0 or e < b:
                continue  # (offsets that are not a scan: all 255)
            for x, y in p[b:e]:
                r2 = F(F(x * x) + F(y * y))
                if not np.isfinite(r2):
                    continue
                q = sum(1 for k in range(1, 255) if r2 >= edge2[k])
                j = point_sector(x, y)
                sig[s, j] = min(int(sig[s, j]), q)
    return sig


# ---------------------------------------------------------------- items 5 and 6: cost and selection
def match(query_sig, map_sig, anchor_list, spec):
    """(records int32 (Q, K, 4), [queries without a record, records written])."""
    Qs = np.asarray(query_sig, dtype=np.int64).reshape(-1, 64)
    As = np.asarray(map_sig, dtype=np.int64).reshape(-1, 64)
    an = [tuple(int(v) for v in a) for a in np.asarray(anchor_list).reshape(-1, 4)]
    K = int(spec.top_k)
    rec = np.full((len(Qs), K, 4), -1, np.int32)
    none, written = 0, 0
    for q, Q in enumerate(Qs):
        js = [j for j in range(64) if Q[j] != 255]
        walk = []
        if len(js) >= spec.min_sectors:
            for a, A in enumerate(As):
                if not (0 <= an[a][0] < spec.width and 0 <= an[a][1] < spec.height):
                    continue  # (no anchor)
                best = None
                for s in range(64):
                    c = int(np.abs(Q[js] - A[[(j + s) % 64 for j in js]]).sum())
                    if best is None or c < best[0]:
                        best = (c, s)
                walk.append((best[0] * 64 + best[1], a))
        walk.sort()
        accepted = []
        for key, a in walk:
            if len(accepted) == K:
                break
            if all(max(abs(an[a][2] - an[b][2]), abs(an[a][3] - an[b][3])) > spec.min_sep for _, b in accepted):
                accepted.append((key, a))
        for k, (key, a) in enumerate(accepted):
            rec[q, k] = (a, key % 64, key // 64, len(js))
        written += len(accepted)
        none += not accepted
    return rec, [none, written]


# ---------------------------------------------------------------- crafted inputs
def _rooms(h, w, seed):
    """free space with walls, unknown patches and values that are neither (1 .. 99: passed by a ray, no anchor)"""
    rng = np.random.default_rng(seed)
    g = np.zeros((h, w), np.int8)
    g[rng.random((h, w)) < 0.06] = 100
    g[rng.random((h, w)) < 0.04] = -1
    g[rng.random((h, w)) < 0.05] = 50
    g[rng.random((h, w)) < 0.02] = 127
    g[rng.random((h, w)) < 0.02] = 99
    if h > 8 and w > 12:
        g[h // 2, 3:w - 3] = 100     # a long wall
        g[h // 2 - 2, 8:12] = -1     # unknown in front of it: rays from below cross it first
        g[2:h - 2, w - 4] = 100
    return g


@functools.lru_cache(maxsize=None)
def map_cases():
    """[(name, grid, spec, rays or None)]: every grid small enough for the per-step loops above."""
    out = []
    g = _rooms(29, 37, 1)
    for st, m, L in ((3, 4, 600), (1, 1, 7), (3, 2, 7), (5, 8, 40), (64, 4, 600)):
        out.append(("rooms 37x29 stride %d m %d L %d" % (st, m, L), g,
                    make_spec(width=37, height=29, stride=st, rays_per_sector=m, max_ray_cells=L, cell_x0=-7, cell_y0=11), None))
    for st, m, L in ((3, 4, 600), (1, 2, 7)):
        out.append(("rooms 37x29 unknown stops stride %d m %d L %d" % (st, m, L), g,
                    make_spec(width=37, height=29, stride=st, rays_per_sector=m, max_ray_cells=L, flags=1), None))
    g = _rooms(3, 5, 2)
    g[1, 2] = 0
    for st, m, L in ((1, 8, 600), (3, 2, 1), (1, 1, 1)):
        out.append(("5x3 stride %d m %d L %d" % (st, m, L), g, make_spec(width=5, height=3, stride=st, rays_per_sector=m, max_ray_cells=L), None))
    out.append(("no free cell", np.where(_rooms(9, 11, 3) == 0, 100, _rooms(9, 11, 3)).astype(np.int8),
                make_spec(width=11, height=9, stride=1, rays_per_sector=1, max_ray_cells=3), None))
    out.append(("free_max 60", _rooms(9, 11, 3), make_spec(width=11, height=9, stride=2, rays_per_sector=1, max_ray_cells=5, free_max=60,
                                                           occ_min=99), None))
    for n in (63, 64, 65, 255, 256, 257):  # exactly n anchors, rows of 70 nodes: more than a wave's 64 per step
        g = np.full(5 * 70, 50, np.int8)
        g[:n] = 0
        out.append(("%d anchors" % n, g.reshape(5, 70), make_spec(width=70, height=5, stride=1, rays_per_sector=1, max_ray_cells=3), None))
    # one wall cell in an open row: every anchor left of it meets it at another k, k = 1 and k = n = 7 among them
    g = np.zeros((3, 12), np.int8)
    g[1, 9] = 100
    out.append(("wall at k = 1 .. n", g, make_spec(width=12, height=3, stride=1, rays_per_sector=1, max_ray_cells=7), None))
    out.append(("saturating unit", g, make_spec(width=12, height=3, stride=1, rays_per_sector=1, max_ray_cells=7, unit=0.001), None))
    # rdiv's halves on both signs: ends (4, 2) and (-4, -2) put the minor step on k * 2 / 4 = 0.5, 1.5: up on both signs of a
    g = np.zeros((9, 13), np.int8)
    g[5, 8] = g[3, 4] = g[4, 7] = 100
    rays = [(4, 2, 4, 30000), (-4, -2, 4, 30000)] * 32
    out.append(("rdiv halves", g, make_spec(width=13, height=9, stride=2, rays_per_sector=1, max_ray_cells=4), rays))
    return out


def _near_edge(T):
    """points whose r2 lies at and around the float32 T: (x, 0) for the floats x around sqrt(T), and (x, y) with a small y"""
    pts = []
    x0 = F(math.sqrt(float(T)))
    xs = [x0]
    for _ in range(6):
        xs = [np.nextafter(xs[0], F(0))] + xs + [np.nextafter(xs[-1], F(np.inf))]
    ulps = (float(np.nextafter(T, F(np.inf))) - float(T), float(T) - float(np.nextafter(T, F(0))))  # (they differ at a power of two)
    for x in xs:
        pts.append((x, F(0)))
        for ulp in ulps:
            for j in (1, 2, 3):
                pts.append((x, F(math.sqrt(j * ulp))))
    return pts


@functools.lru_cache(maxsize=None)
def scan_case():
    """(xy float32, offsets int32, spec): scans of 0, 1, 63, 64, 65, 1081 and 3000 points and the crafted ones"""
    spec = make_spec()
    rng = np.random.default_rng(7)
    edge2 = edge_table(spec)
    scans = [np.zeros((0, 2), F)]
    for n in (1, 63, 64, 65, 1081, 3000):
        r, a = rng.uniform(0.0, 35.0, n), rng.uniform(-math.pi, math.pi, n)
        scans.append(np.stack([r * np.cos(a), r * np.sin(a)], axis=1).astype(F))
    scans.append(np.array([(0, 0), (-1, 0.0), (-1, -0.0), (1, 0), (0, 1), (0, -1), (-0.0, 0.0)], F))  # the sector counts' boundaries
    scans.append(np.array(_near_edge(edge2[1]) + _near_edge(edge2[254]), F))
    scans.append(np.array([(np.nan, 1), (1, np.nan), (np.inf, 0), (-np.inf, 1), (3e19, 3e19), (1e-30, 1e-30), (2, 2)], F))
    a = rng.uniform(-math.pi, math.pi, 40)  # several points per sector, few sectors: the minimum decides
    r = rng.uniform(0.1, 31.0, 40)
    scans.append(np.stack([r * np.cos(np.round(a)), r * np.sin(np.round(a))], axis=1).astype(F))
    xy = np.concatenate(scans).astype(F)
    off = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int32)
    return xy, off, spec


def lattice_anchors(n, per_row=10):
    """n anchors on a lattice of stride 1 in a window of per_row x ceil(n / per_row): {cx, cy, i, j} = {i, j, i, j}"""
    b = np.arange(n)
    return np.stack([b % per_row, b // per_row, b % per_row, b // per_row], axis=1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def match_cases():
    """[(name, query_sig, map_sig, anchors, spec)] on crafted bytes"""
    rng = np.random.default_rng(11)
    out = []

    def spec_for(n, **kw):
        return make_spec(width=10, height=max((n + 9) // 10, 1), stride=1, **kw)
    for A in (1, 63, 64, 65, 257):
        for Q in (0, 1, 17):
            qs = rng.integers(0, 256, (Q, 64)).astype(np.uint8)
            qs[rng.random((Q, 64)) < 0.3] = 255
            ms = rng.integers(0, 256, (A, 64)).astype(np.uint8)
            out.append(("random A %d Q %d" % (A, Q), qs, ms, lattice_anchors(A), spec_for(A, min_sep=int(A % 3))))
    # ties: every shift costs the same (the smallest wins), two anchors cost the same (the lower index wins)
    ms = np.full((30, 64), 10, np.uint8)
    qs = np.full((2, 64), 12, np.uint8)
    qs[1, ::3] = 255
    out.append(("ties among shifts and anchors", qs, ms, lattice_anchors(30), spec_for(30, min_sep=0)))
    # all-255 query, valid = min_sectors - 1 against valid = min_sectors
    qs = np.full((3, 64), 255, np.uint8)
    qs[1, :7] = 20
    qs[2, :8] = 20
    ms = rng.integers(0, 255, (40, 64)).astype(np.uint8)
    out.append(("valid around min_sectors", qs, ms, lattice_anchors(40), spec_for(40)))
    # the largest cost: 64 sectors of |0 - 255| = 16,320; 254 beside it
    qs = np.zeros((2, 64), np.uint8)
    qs[1] = 254
    ms = np.stack([np.full(64, 255, np.uint8), np.full(64, 254, np.uint8), np.zeros(64, np.uint8)])
    out.append(("bytes 0 254 255", qs, ms, lattice_anchors(3), spec_for(3, min_sep=0, top_k=3)))
    # suppression: equal signatures everywhere, so the walk is the list's order: anchors at exactly min_sep and min_sep + 1 steps,
    # and the lattice row wrap (the end of one row and the start of the next are 9 steps apart in i)
    ms = np.full((40, 64), 7, np.uint8)
    qs = np.full((1, 64), 9, np.uint8)
    for sep in (0, 1, 2, 3):
        out.append(("suppression min_sep %d" % sep, qs, ms, lattice_anchors(40), spec_for(40, min_sep=sep, top_k=16)))
    # fewer admissible anchors than K: -1 fill; two entries of the list are no anchors (cells outside the window)
    an = lattice_anchors(6)
    an[1] = (-1, -1, -1, -1)
    an[4, 0] = 10
    out.append(("fewer anchors than K", qs, ms[:6], an, spec_for(6, min_sep=0, top_k=8)))
    # a scan turned by 5 sectors: Q[j] = A[(j + 5) mod 64] recovers shift 5 at cost 0
    ms = rng.integers(0, 255, (12, 64)).astype(np.uint8)
    qs = np.stack([np.roll(ms[7], -5), np.roll(ms[3], -63)])
    qs[0, 10:30] = 255
    out.append(("turned by 5 and by 63 sectors", qs, ms, lattice_anchors(12), spec_for(12)))
    return out


@functools.lru_cache(maxsize=None)
def map_results():
    """{name: (anchors, sig, stats)} of map_cases(), computed once"""
    return {name: anchors_and_signatures(g, s, rays) for name, g, s, rays in map_cases()}


@functools.lru_cache(maxsize=None)
def scan_result():
    xy, off, spec = scan_case()
    return scan_signatures(xy, off, spec)


@functools.lru_cache(maxsize=None)
def match_results():
    """{name: (records, [queries without a record, records written])} of match_cases(), computed once"""
    return {name: match(qs, ms, an, s) for name, qs, ms, an, s in match_cases()}
