"""Shared inputs of the correspondence-search SEAM tests (tests/test_corr_seams_cpu.py holds their preconditions,
tests/test_corr_seams_gpu.py runs them): blocks that put every input-dependent seam of corr_search_kernel, corr_scan_kernel
and corr_compact_kernel (nhip_corr.hip, K5) on an index by design, and the rows the CPU oracle gives for them (plain:
oracle.corr_search_batch; gated at cos 20 deg: oracle.corr_search_gated_batch), computed once and read-only.

Every pose is exactly zero: inverse(T_t) * T_s is the identity in the kernel's float arithmetic, a query equals its source
point bit for bit, and the kernel's path conditions are restated here exactly in float32 numpy (inv_cell, cells, hashed,
scan_everything_passes, bucket).  Point i of EVERY scan carries the normal (1, (i + 1) / 8192): a row names the target index
it matched (matched_index), so a tie between coincident targets that goes to the wrong one changes the row's bytes; against
a source normal the gate's dot product is at least 1 and passes, except where a family replaces a target's normal by
(0, (i + 1) / 8192), which fails it.

  family_a()        source ladder x keep masks on one hashed target of 600 points: sources of 0 .. 4097 points put the ends
                    of a wave (63 | 64), of a round (255 | 256) and of a source pass (2047 | 2048, 4095 | 4096) on designed
                    kept rows -- the ballot's popcount below lane 63, the (round, wave) table, `pos += round_total` and the
                    `written` carried into the next pass, with every row kept, none, every other, a random half, and ONE
  family_b()        target ladder: targets of 0 .. 4097 points -- a ragged last staging round (255 | 256 | 257), the full stage
                    (2047 | 2048: hashed, uint16 indices up to 2047) and the exhaustive scan's second and third stage
                    (2049, 4096 | 4097: `t0 + i`); the nearest neighbour is the last point, point 0, or the lower of two
                    coincident points on either side of a stage seam or at the two ends of the cloud
  family_c(thr)     the two-run bucket visit: query cells cx = -5 .. 4 (every residue of cx & 3 on both sides of zero, the
                    arithmetic shift of negative cells, `lo >> 2 != hi2 >> 2`, `b0 | 3`, `b0 + 2`, the second run), the only
                    target in reach in each of the nine cells around the query
  family_d()        bucket extremes: 2,048 targets in ONE cell (one bucket holds the stage, every lane walks all of it) and
                    2,048 targets in 2,048 cells
  family_e()        path switches: a hashed 2,048-point target 25 m inside the 4096-cell limit and a source of two passes
                    with a query beyond the limit in neither, the first, the second or both -- the hashed target scanned in
                    bucket order (`s_sorted[i]`, the unsigned tie-break), walk and scan in one block with `written` carried
                    between them; the same with a query at 3e7; a target with one point beyond the limit (never hashed)
  family_g()        the gate inside the walk: the nearest target fails it, the second nearest is the match
  family_f(n)       1023 .. 2500 blocks of scans of 0 .. 5 points: corr_scan_kernel's steps of 1024 and their carry, runs of
                    blocks without rows at both ends and across each seam, corr_compact_kernel's `n == 0`

A case is a Case: scans, block lists, threshold and what its family designed."""
import functools
import math

import numpy as np

from oracle import oracle as O

F = np.float32
LANES = 256                  # nhip_corr_shared.h (CT, NB, CELL_LIMIT) and nhip_corr.hip: CT, threads of a workgroup
ROUNDS = 8                   # MAX_PER_LANE: source points a lane owns per pass
PASS = LANES * ROUNDS        # source points per pass
STAGE = 2048                 # TGT_CHUNK: target points staged in LDS, the most a hashed block holds (uint16_t s_sorted)
BUCKETS = 1024               # NB: hash buckets, in groups of four
CELL_LIMIT = 4096.0          # CELL_LIMIT: cell coordinates from here on take the exhaustive scan
SCAN_STEP = 1024             # blocks per step of corr_scan_kernel
WAVE = 64
THR = 0.25
MIN_COS = math.cos(math.radians(20.0))
NORMAL_STEP = 1.0 / 8192.0   # a point's normal is (1, (index + 1) / 8192): exact in float for every index used here


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def normals_of(n, failing=()):
    """The normals of a scan of n points; the points listed in `failing` get (0, .): no source normal passes the gate."""
    nrm = np.stack([np.ones(n), (np.arange(n) + 1) * NORMAL_STEP], axis=1).astype(F)
    nrm[list(failing), 0] = 0.0
    return nrm


def matched_index(rows):
    """The target index every row names through its target normal."""
    return np.rint(np.asarray(rows)[:, 7].astype(np.float64) / NORMAL_STEP).astype(np.int64) - 1


class Case:
    """scans / normals: lists of (n, 2) float32; xy, nrm, off: the packed table; bs, bt: the blocks; aff: zero poses as
    (cos, sin, x, y) rows; thr; design: what the family's preconditions refer to."""

    def __init__(self, name, thr, scans, bs, bt, normals=None, **design):
        self.name, self.thr = name, float(thr)
        self.scans = [np.ascontiguousarray(s, dtype=F).reshape(-1, 2) for s in scans]
        self.normals = [normals_of(len(s)) for s in self.scans]
        for k, v in (normals or {}).items():
            self.normals[k] = np.ascontiguousarray(v, dtype=F).reshape(-1, 2)
        self.xy = np.concatenate(self.scans + [np.zeros((0, 2), F)]).astype(F)
        self.nrm = np.concatenate(self.normals + [np.zeros((0, 2), F)]).astype(F)
        self.off = np.concatenate([[0], np.cumsum([len(s) for s in self.scans])]).astype(np.int32)
        self.bs, self.bt = np.asarray(bs, dtype=np.int32), np.asarray(bt, dtype=np.int32)
        self.aff = np.tile(F([1, 0, 0, 0]), (len(self.scans), 1))
        self.design = design
        for a in self.scans + self.normals + [self.xy, self.nrm, self.off, self.bs, self.bt, self.aff]:
            a.setflags(write=False)

    @property
    def n_blocks(self):
        return len(self.bs)

    def block(self, b):
        """(source xy, source normals, target xy, target normals) of block b."""
        s, t = int(self.bs[b]), int(self.bt[b])
        return self.scans[s], self.normals[s], self.scans[t], self.normals[t]


# ------------------------------------------------------------------------------------- the kernel's path conditions, restated
def inv_cell(thr):
    """`__fdiv_rn(1.0f, __fmul_rn(thr, 1.001f))`"""
    return F(1.0) / (F(thr) * F(1.001))


def scaled(v, thr):
    """`__fmul_rn(v, inv_cell)`: the float cell coordinate."""
    return (np.asarray(v, dtype=F) * inv_cell(thr)).astype(F)


def cells(pts, thr):
    """`(int32_t)floorf(fx), (int32_t)floorf(fy)` of every point (the points are within the limit)."""
    return np.floor(scaled(pts, thr)).astype(np.int64).reshape(-1, 2)


def hashed(tgt, thr):
    """The block buckets its target: it fits the stage and no coordinate reaches the limit."""
    return len(tgt) <= STAGE and bool(np.all(np.abs(scaled(tgt, thr)) < CELL_LIMIT))


def scan_everything_passes(src, tgt, thr):
    """Per source pass of 2048 points: True where the pass takes the exhaustive scan (`scan_all`)."""
    h = hashed(tgt, thr)
    return [bool(not h or np.any(np.abs(scaled(src[p:p + PASS], thr)) >= CELL_LIMIT)) for p in range(0, len(src), PASS)]


def paths(case, b):
    """(hashed, [scan_all of every pass]) of block b."""
    src, _, tgt, _ = case.block(b)
    return hashed(tgt, case.thr), scan_everything_passes(src, tgt, case.thr)


def _u32(v):
    return np.asarray(v, dtype=np.int64) & 0xFFFFFFFF


def group_hash(gx, cy):
    return ((((_u32(gx) * 73856093) & 0xFFFFFFFF) ^ ((_u32(cy) * 19349663) & 0xFFFFFFFF)) & (BUCKETS // 4 - 1)) << 2


def bucket(cx, cy):
    """`cell_hash`: the group of (cx >> 2, cy) is hashed, the cell's place in it is cx & 3."""
    cx = np.asarray(cx, dtype=np.int64)
    return group_hash(cx >> 2, cy) | (cx & 3)


def two_runs(cx):
    """The three cells cx - 1 .. cx + 1 straddle a group of four."""
    cx = np.asarray(cx, dtype=np.int64)
    return ((cx - 1) >> 2) != ((cx + 1) >> 2)


# ------------------------------------------------------------------------------------------------------------ the oracle's rows
@functools.lru_cache(maxsize=None)
def expected(name, gated):
    """(rows (capacity, 8), counts, cap_offsets) of case `name` by the CPU oracle."""
    c = case(name)
    if gated:
        return _frozen(*O.corr_search_gated_batch(c.xy, c.nrm, c.off, c.bs, c.bt, c.aff, c.thr, MIN_COS))
    return _frozen(*O.corr_search_batch(c.xy, c.nrm, c.off, c.bs, c.bt, c.aff, c.thr))


def block_rows(name, gated, b):
    rows, counts, cap = expected(name, gated)
    return rows[cap[b]:cap[b] + counts[b]]


def compacted(name, gated):
    """(block_offsets, rows, corr_block): the contiguous layout nhip_corr_compact_dev leaves."""
    rows, counts, cap = expected(name, gated)
    keep = (np.arange(len(rows)) - np.repeat(cap[:-1], np.diff(cap))) < np.repeat(counts, np.diff(cap))
    boff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return boff, rows[keep], np.repeat(np.arange(len(counts), dtype=np.int32), counts)


# ------------------------------------------------------------------------------------- a. source ladder x keep masks
A_LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049, 4096, 4097)
A_LONE = (0, 63, 64, 255, 256, 2047, 2048)  # ends of a wave, of a round, of a pass
A_TARGET = 600


def a_masks(ns):
    """name -> keep mask of a source of ns points (masks that coincide at this length are listed once)."""
    rng = np.random.default_rng(1000 + ns)
    out = {"all": np.ones(ns, bool), "none": np.zeros(ns, bool), "alternating": np.arange(ns) % 2 == 0,
           "half": rng.permutation(ns) < ns // 2}
    for k in A_LONE + (ns - 1,):
        if 0 <= k < ns:
            m = np.zeros(ns, bool)
            m[k] = True
            out["lone@%d" % k] = m
    seen, unique = set(), {}
    for name, m in out.items():
        if m.tobytes() not in seen:
            seen.add(m.tobytes())
            unique[name] = m
    return unique


@functools.lru_cache(maxsize=None)
def family_a():
    """Scan 0: the target, 25 x 24 points 0.7 m apart (jittered by 5 cm).  One source scan and one block per (length, mask):
    point i sits within 4 mm of target (7 i + 3) % 600 where the mask keeps it, and 37 m from there where it does not.
    design: blocks = [(ns, mask name, mask, designed target index of every point)]."""
    rng = np.random.default_rng(101)
    k = np.arange(A_TARGET)
    tgt = (np.stack([(k % 25 - 12) * 0.7, (k // 25 - 12) * 0.7], axis=1) + rng.uniform(-0.05, 0.05, (A_TARGET, 2))).astype(F)
    scans, blocks = [tgt], []
    for ns in A_LENGTHS:
        for name, mask in a_masks(ns).items():
            j = (7 * np.arange(ns) + 3) % A_TARGET
            p = tgt[j].astype(np.float64) + rng.uniform(-0.004, 0.004, (ns, 2))
            p[~mask] += [37.0, -23.0]
            scans.append(p.astype(F))
            blocks.append((ns, name, _frozen(mask), _frozen(j)))
    n = len(blocks)
    return Case("a", THR, scans, np.arange(1, n + 1), np.zeros(n), blocks=blocks)


# ------------------------------------------------------------------------------------------------------ b. target ladder
B_LENGTHS = (0, 1, 2, 255, 256, 257, 2047, 2048, 2049, 4096, 4097)
B_SOURCES = 300
B_SEAMS = ((2047, 2048), (4095, 4096))  # the last point of a stage and the first of the next
B_VARIANTS = ("ends", "seam", "wrap")


def b_sets(nt, variant):
    """The coincident sets (lower index, higher index) of a target, or None where the variant does not exist at this length.
    ends: points 0 and nt - 1 are unique nearest neighbours; stage seams strictly inside the cloud carry a coincident pair.
    seam: every stage seam the cloud has carries a pair, the last point included.  wrap: points 0 and nt - 1 coincide."""
    if variant == "ends":
        return [s for s in B_SEAMS if s[1] < nt - 1] if nt >= 1 else None
    if variant == "seam":
        return [s for s in B_SEAMS if s[1] < nt] if nt > STAGE else None
    if variant == "wrap":
        return [(0, nt - 1)] + [s for s in B_SEAMS if s[1] < nt - 1] if nt >= 2 else None
    raise KeyError(variant)


def b_target(nt, variant):
    k = np.arange(nt)
    rng = np.random.default_rng(200 + nt)
    tgt = (np.stack([(k % 72 - 36) * 0.7, (k // 72 - 30) * 0.7], axis=1) + rng.uniform(-0.05, 0.05, (nt, 2))).astype(F)
    for lo, hi in b_sets(nt, variant):
        tgt[hi] = tgt[lo]
    return tgt


@functools.lru_cache(maxsize=None)
def family_b():
    """One target and one source scan per (length, variant), and the empty target.  Source points 0 .. 3 sit next to target 0,
    target nt - 1 and the higher point of each stage-seam pair; the others next to random targets, every fifth 37 m away.
    design: blocks = [(nt, variant, sets, designed: (n_sources,) index of the target each source sits next to or -1)]."""
    scans, bs, bt, blocks = [], [], [], []
    for nt in B_LENGTHS:
        for variant in B_VARIANTS if nt else ("empty",):
            sets = [] if nt == 0 else b_sets(nt, variant)
            if sets is None:
                continue
            rng = np.random.default_rng(300 + 7 * nt + len(variant))
            tgt = b_target(nt, variant) if nt else np.zeros((0, 2), F)
            j = rng.integers(0, max(nt, 1), B_SOURCES)
            j[4::5] = -1
            j[:4] = [0, nt - 1, min(B_SEAMS[0][1], nt - 1), min(B_SEAMS[1][1], nt - 1)]
            if nt == 0:
                j[:] = -1
            src = np.array([37.0, -23.0]) + rng.uniform(0.0, 5.0, (B_SOURCES, 2))
            src[j >= 0] = tgt[j[j >= 0]]
            src = (src + rng.uniform(-0.004, 0.004, (B_SOURCES, 2))).astype(F)
            bt.append(len(scans))
            scans.append(tgt)
            bs.append(len(scans))
            scans.append(src)
            blocks.append((nt, variant, tuple(sets), _frozen(j)))
    return Case("b", THR, scans, bs, bt, blocks=blocks)


def lowest_coincident(tgt):
    """For every target point the lowest index with the same coordinates."""
    first = {}
    return np.array([first.setdefault(p.tobytes(), i) for i, p in enumerate(np.ascontiguousarray(tgt))], dtype=np.int64)


# ------------------------------------------------------------------------------------- c. neighbour cells of the two-run visit
C_CX = tuple(range(-5, 5))
C_OFFSETS = tuple((ox, oy) for oy in (-1, 0, 1) for ox in (-1, 0, 1))
C_THRESHOLDS = (0.25, 0.03)


@functools.lru_cache(maxsize=None)
def family_c(thr):
    """One block of 90 queries and 90 targets.  Case n = (cx, (ox, oy)): the query at the centre of cell (cx, cy_n), cy_n =
    12 (n - 45) + n % 3 (at least ten cells between cases, both signs), its target at the centre + 0.6 cell (ox, oy): 0.85 cell
    away at most, in cell (cx + ox, cy_n + oy); the targets are stored in a seeded order.
    design: cx, cy, ox, oy (90,), target_of (90,): index of query n's target."""
    cell = np.float64(F(thr) * F(1.001))
    cx = np.repeat(C_CX, len(C_OFFSETS))
    ox, oy = np.tile([o[0] for o in C_OFFSETS], len(C_CX)), np.tile([o[1] for o in C_OFFSETS], len(C_CX))
    n = np.arange(len(cx))
    cy = 12 * (n - 45) + n % 3
    q = np.stack([(cx + 0.5) * cell, (cy + 0.5) * cell], axis=1).astype(F)
    t = np.stack([(cx + 0.5 + 0.6 * ox) * cell, (cy + 0.5 + 0.6 * oy) * cell], axis=1).astype(F)
    order = np.random.default_rng(41).permutation(len(n))  # target index i holds case order[i]'s target
    target_of = np.argsort(order)
    return Case("c%g" % thr, thr, [q, t[order]], [0], [1], cx=_frozen(cx), cy=_frozen(cy), ox=_frozen(ox), oy=_frozen(oy),
                target_of=_frozen(target_of))


# ------------------------------------------------------------------------------------------------------ d. bucket extremes
D_CELL = (7, -3)
D_COINCIDENT = ((5, 6, 2047), (100, 1900))
D_PER_CELL = 20


@functools.lru_cache(maxsize=None)
def family_d():
    """Block 0: 2,048 targets inside cell (7, -3), distinct but for the sets D_COINCIDENT; queries: one ON each coincident set
    (distance 0 to all of its points), then 20 in that cell and in each of its eight neighbours.  Block 1: target k in cell
    (k % 64 - 32, k // 64 - 16); 300 queries within 4 mm of random targets, every seventh 37 m away.
    design: on_sets: [(query, lowest index of its set)], all_cells_designed (300,)."""
    rng = np.random.default_rng(51)
    cell = np.float64(F(THR) * F(1.001))
    one = ((np.array(D_CELL) + rng.uniform(0.02, 0.98, (STAGE, 2))) * cell).astype(F)
    for s in D_COINCIDENT:
        one[list(s[1:])] = one[s[0]]
    q = [one[[s[0] for s in D_COINCIDENT]]]
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            q.append(((np.array(D_CELL) + [dx, dy] + rng.uniform(0.02, 0.98, (D_PER_CELL, 2))) * cell).astype(F))
    k = np.arange(STAGE)
    spread = ((np.stack([k % 64 - 32, k // 64 - 16], axis=1) + rng.uniform(0.05, 0.95, (STAGE, 2))) * cell).astype(F)
    j = rng.integers(0, STAGE, 300)
    j[6::7] = -1
    src = spread[np.maximum(j, 0)].astype(np.float64) + rng.uniform(-0.004, 0.004, (300, 2))
    src[j < 0] += [37.0, -23.0]
    return Case("d", THR, [np.concatenate(q), one, src.astype(F), spread], [0, 2], [1, 3],
                on_sets=[(i, s[0]) for i, s in enumerate(D_COINCIDENT)], all_cells_designed=_frozen(j))


# --------------------------------------------------------------------------------------------------------- e. path switches
E_SETS = ((17, 700, 1301, 2040), (3, 512, 1024, 2047))     # four coincident targets each, at x = 1024.95
E_SET_XY = ((1024.95, 1.0), (1024.95, 3.0))
E_FAR_XY = ((1025.1, 1.0), (1025.1, 3.0))                  # beyond the limit of 1025.02 m, 0.15 m from a set
E_HUGE_XY = ((3.0e7, 1.0), (3.0e7, 3.0))
E_SOURCES = PASS + 300
E_AT = (1000, PASS + 100)                                  # the far query's place in pass 0 and in pass 1
E_BEYOND = 77                                              # the target point moved beyond the limit in the last block
E_VARIANTS = ("none", "pass0", "pass1", "both", "huge pass0", "huge pass1", "huge both", "target beyond")


@functools.lru_cache(maxsize=None)
def family_e():
    """Scan 0: 2,048 targets, 128 x 16 between x = 1000 and 1024.7 with the two coincident sets at x = 1024.95 (hashed: 4095.7
    cells); scan 1: the same with point 77 at x = 1025.3 (never hashed).  Sources of 2,348 points within 4 mm of targets; the
    variants replace the points E_AT by queries beyond the limit.
    design: variants; far: per block [(source index, lowest index of its set or -1 for a query that matches nothing)]."""
    rng = np.random.default_rng(61)
    k = np.arange(STAGE)
    tgt = np.stack([1000.0 + 24.7 * (k % 128) / 127.0, 0.3 * (k // 128)], axis=1)
    for s, p in zip(E_SETS, E_SET_XY):
        tgt[list(s)] = p
    tgt = tgt.astype(F)
    beyond = tgt.copy()
    beyond[E_BEYOND] = (1025.3, 2.0)
    j = (5 * np.arange(E_SOURCES) + 1) % STAGE
    base = (tgt[j].astype(np.float64) + rng.uniform(-0.004, 0.004, (E_SOURCES, 2))).astype(F)
    scans, bs, bt, far = [tgt, beyond], [], [], []
    for v in E_VARIANTS:
        src, marks = base.copy(), []
        where = {"pass0": [0], "pass1": [1], "both": [0, 1]}.get(v.replace("huge ", ""), [])
        for n, p in enumerate(where):  # (the first far query goes to set 0, the second to set 1)
            src[E_AT[p]] = (E_HUGE_XY if v.startswith("huge") else E_FAR_XY)[n]
            marks.append((E_AT[p], -1 if v.startswith("huge") else E_SETS[n][0]))
        bs.append(len(scans))
        bt.append(1 if v == "target beyond" else 0)
        scans.append(src)
        far.append(marks)
    return Case("e", THR, scans, bs, bt, variants=E_VARIANTS, far=far, base=_frozen(base))


# ------------------------------------------------------------------------------------------ g. the gate decides inside the walk
G_SOURCES = 300


@functools.lru_cache(maxsize=None)
def family_g():
    """300 queries a metre apart; each has a target 5 cm away whose normal FAILS the gate and one 12 cm away that passes.
    design: near, second (300,): the two target indices of every query."""
    rng = np.random.default_rng(71)
    k = np.arange(G_SOURCES)
    q = np.stack([(k % 20) * 1.0, (k // 20) * 1.0], axis=1) + rng.uniform(-0.2, 0.2, (G_SOURCES, 2))
    order = rng.permutation(2 * G_SOURCES)
    pts = np.concatenate([q + [0.05, 0.0], q + [0.0, -0.12]])  # (first half: the near ones)
    where = np.argsort(order)                                  # pts[m] is stored at index where[m]
    near, second = where[:G_SOURCES], where[G_SOURCES:]
    return Case("g", THR, [q, pts[order]], [0], [1], normals={1: normals_of(2 * G_SOURCES, failing=near)}, near=_frozen(near),
                second=_frozen(second))


# ------------------------------------------------------------------------------------------------ f. block-count ladder
F_BLOCKS = (1023, 1024, 1025, 2048, 2049, 2500)
F_EDGE_RUN, F_SEAM_RUN = 7, 12  # blocks without rows at each end; on either side of every seam


def f_empty_runs(n):
    """[from, to) runs of blocks designed to keep no row."""
    runs = [(0, F_EDGE_RUN), (n - F_EDGE_RUN, n)]
    return runs + [(s - F_SEAM_RUN, min(s + F_SEAM_RUN, n)) for s in range(SCAN_STEP, n + 1, SCAN_STEP)]


@functools.lru_cache(maxsize=None)
def family_f(n):
    """Scans 0 .. 5: the first k of five anchor points a metre apart (targets); 6 .. 11: the same within 4 mm (sources that
    match); 12 .. 17: the same 50 m away (sources that match nothing).  n blocks of random pairs; inside f_empty_runs(n) the
    source is the 0-point scan, a far one, or the target is the 0-point scan, in turn."""
    rng = np.random.default_rng(81)
    anchor = np.stack([np.arange(5) * 1.0, np.zeros(5)], axis=1)
    scans = [anchor[:k] for k in range(6)] + [anchor[:k] + rng.uniform(-0.004, 0.004, (k, 2)) for k in range(6)] + \
            [anchor[:k] + 50.0 for k in range(6)]
    rng = np.random.default_rng(82 + n)
    bs, bt = rng.integers(6, 18, n), rng.integers(0, 6, n)
    empty = np.zeros(n, bool)
    for lo, hi in f_empty_runs(n):
        for b in range(max(lo, 0), hi):
            empty[b] = True
            bs[b], bt[b] = [(6, bt[b]), (12 + b % 6, bt[b]), (6 + b % 6, 0)][b % 3]
    return Case("f%d" % n, THR, scans, bs, bt, empty=_frozen(empty))


# ----------------------------------------------------------------------------------------------------------------- registry
CASES = ["a", "b"] + ["c%g" % t for t in C_THRESHOLDS] + ["d", "e", "g"] + ["f%d" % n for n in F_BLOCKS]


def case(name):
    if name.startswith("c"):
        return family_c(float(name[1:]))
    if name.startswith("f"):
        return family_f(int(name[1:]))
    return {"a": family_a, "b": family_b, "d": family_d, "e": family_e, "g": family_g}[name]()
