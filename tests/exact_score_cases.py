"""Designed inputs for the exact-score pass (NHIP_SEARCH_EXACT_SCORE: csm_exact_score_kernel, nhip_csm_score.hip) and its
definition in numpy.  No device; of the library only host calls (the spec's taps).

THE DEFINITION.  V = blur_sums(hit_raster(target), taps) are exact integers; a cell's likelihood
is v = max(float64(V) / float64(K * K), floor_p), its log is taken in longdouble, and a pair's score is the longdouble mean
over ALL points of the source scan: a point that fails the sanity rule (a rotated coordinate that is not finite or not below
1e9 in magnitude) or lands outside the grid contributes log(floor_p), an empty scan scores log(floor_p).  A point's cell
follows the kernels' chain: (cos, sin) of theta0 and of the lattice's delta composed in double, each operation rounded on
its own, narrowed to float; xr, yr in float, each operation rounded on its own; cell = S // 2 + floor(double(xr) / res) +
origin + lattice index - half width.  oracle.pose_score_exact is the second, independent statement;
tests/test_exact_score_cases_cpu.py holds the two together on every case below.

THE BOUND.  Every log-likelihood is <= 0: the mean has no cancellation, and a double evaluation in any order differs from
the definition by at most (K + n) * 2**-53 relative -- n for the order of the n-term sum, K for log, the division and the
rotation.  K by the project's rule (tests/resid_reference.py k_rule), measured on the CPU, never from a kernel: the oracle's
in-order double sum against the longdouble definition over all 4,450 cases below gives a worst one-point ratio of 0.995 and a
worst (ratio - n) of -36.2 on the longer scans (their ratios stay below 27.3 at n up to 1300), so K_EXACT = max(4, 4 * 0.995
rounded up to a power of two) = 4.
The record is a float: interval() gives lo, hi = float32(ref -+ |ref| (K + n) 2**-53), and a score must lie in the closed
float interval [lo, hi] -- one float unless the definition sits on a rounding boundary (under 1 % of the cases, checked).

THE GEOMETRY is small: range 3.0 m, res 0.05 (S = 120), max_shift 8, floor_p 1e-10.  One target per blur radius, placed by
CELL (target_cells): random hits in bands along the rim and in all four corners (windows hang into the zero border), a
scatter field (windows of many bit patterns), a band along one row and one column (whole-row probes), a filled block of
(2 R + 2)^2 cells (961 of its 1024 points are what V = K^2 needs at R = 15) and a region without hits (an empty window).

THE LISTS (lists(sigma)): every one is a list of pairs against that target.
  probes     one-point scans, 1 x 1 x 1 lattice, theta0 = 0: the record's score is log(max(V / K^2, floor)) of ONE chosen cell
             -- 32 consecutive columns on three rows (every value of the window shift (col - R + 32) & 31), rows and
             columns 0 and S - 1 with the corners, the block's all-hit cells (score exactly 0), empty windows; the cell is
             reached through pair_origin, which takes every value of -8 .. 8
  floor      probes under a floor_p strictly between two attainable V / K^2 of the probed cells: clamp | log
  counts0/1  scans of 0, 1, 63, 64, 65, 255, 256, 257, 1081, 1300 points (strides of 256 threads, 64 lanes, four waves),
             theta0 = 0 | oblique, 3 x 3 x 3 lattice searched for real; `counts*_short` without the 1300-point scan, for
             slots without an image (NHIP_GRID_NO_IMAGE serves scans of at most 1088 points)
  pairs<n>   n = 1, 7, 8, 9, 15, 17 pairs with pairwise different scores (pair = (block & 7) * pairs_per_xcd + (block >> 3))
  edges      one-point scans at NaN / +-inf, at and below 1e9, at +-range and one float inside / outside (with origins that
             move the cell across the rim), at every float multiple of res on both axes; and all of them in one scan
  shift_ok / shift_beyond    1 x 3 x 3 lattices with |origin| + 1 == max_shift | max_shift + 1
"""
import functools
import math
from types import SimpleNamespace as NS

import numpy as np

from nautilus_amd import csm
from oracle import oracle as O
from tests import grid_reference as G

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "numpy.longdouble is not the 80-bit extended format here"
U = 2.0 ** -53
RANGE, RES, SIDE, MAX_SHIFT, FLOOR_P = 3.0, 0.05, 120, 8, 1e-10
HIT_PAD = 32
SIGMAS = (0.5, 1.0, 2.0, 2.4, 5.0)  # R = 2 (generic), 3 (<7>), 6 (<13>), 8 (generic, 17 bits), 15 (generic, 31 bits)
COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 1081, 1300)
PAIR_LISTS = (1, 7, 8, 9, 15, 17)
OBLIQUE = 0.3
DEG = math.radians(1.0)
K_EXACT = 4
SEED = 7


def radius(sigma):
    return int(math.ceil(3.0 * sigma))


def spec(sigma, cell_bits=16, no_image=False, floor_p=FLOOR_P):
    return csm.grid_spec(RANGE, RES, sigma, floor_p, MAX_SHIFT, cell_bits, no_image=no_image)


def ospec(sigma, floor_p=FLOOR_P):
    return O.grid_spec(RANGE, RES, sigma, floor_p, 16)


@functools.lru_cache(maxsize=None)
def taps(sigma):
    t, _ = G.grid_tables(spec(sigma))
    assert len(t) == 2 * radius(sigma) + 1
    t = t.astype(np.int64)
    t.setflags(write=False)
    return t


# ------------------------------------------------------------------------------------------------ the target
def points_in_cells(cells):
    """float32 points in the middle of the cells (column, row) -- cells outside the grid too -- checked to lie in them."""
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 2)
    pts = ((cells - SIDE // 2 + 0.5) * RES).astype(np.float32)
    assert np.array_equal(G.cells_of(pts, SIDE, RES), cells), "a cell centre fell into another cell"
    return pts


BAND_ROW, BAND_COL = 52, 102         # the whole-row and whole-column bands (5 cells wide, from here)
SCATTER = (8, 56, 66, 94)            # columns [8, 56), rows [66, 94)
BLOCK_AT = (70, 62)                  # first column, first row of the filled block
EMPTY_AT = (60, 25)                  # no hit within 15 cells of it


@functools.lru_cache(maxsize=None)
def target_cells(R):
    rng = np.random.default_rng(SEED)
    S = SIDE
    hit = np.zeros((S, S), bool)  # [row][column]
    ends = np.r_[0:40, S - 40:S]
    for lo in (0, S - 5):
        hit[lo:lo + 5, ends] |= rng.random((5, len(ends))) < 0.15
        hit[ends, lo:lo + 5] |= rng.random((len(ends), 5)) < 0.15
    hit[[0, 0, S - 1, S - 1], [0, S - 1, 0, S - 1]] = True
    c0, c1, r0, r1 = SCATTER
    hit[r0:r1, c0:c1] |= rng.random((r1 - r0, c1 - c0)) < 0.2
    hit[BAND_ROW:BAND_ROW + 5, :] |= rng.random((5, S)) < 0.2
    hit[:, BAND_COL:BAND_COL + 5] |= rng.random((S, 5)) < 0.2
    bc, br = BLOCK_AT
    hit[br:br + 2 * R + 2, bc:bc + 2 * R + 2] = True
    ec, er = EMPTY_AT
    assert not hit[er - 15:er + 16, ec - 15:ec + 16].any()
    rr, cc = np.nonzero(hit)
    cells = np.stack([cc, rr], axis=1)
    cells = cells[rng.permutation(len(cells))]
    cells.setflags(write=False)
    return cells


@functools.lru_cache(maxsize=None)
def target(sigma):
    pts = points_in_cells(target_cells(radius(sigma)))
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def blur(sigma):
    """The target's exact blur sums, (S, S) int64 [row][column]."""
    V = G.blur_sums(G.hit_raster(target(sigma), SIDE, RES), taps(sigma))
    V.setflags(write=False)
    return V


# ------------------------------------------------------------------------------------------------ the definition
def rotation(theta0, k, n_theta, theta_step):
    """(cos, sin) of rotation k as float32: R(theta0) R(delta_k) composed in double, every operation rounded on its own."""
    c0, s0 = math.cos(theta0), math.sin(theta0)
    d = (k - (n_theta - 1) // 2) * theta_step
    cd, sd = math.cos(d), math.sin(d)
    a, b, e, f = c0 * cd, s0 * sd, s0 * cd, c0 * sd
    return np.float32(a - b), np.float32(e + f)


def lookup_cells(points, cf, sf, shift):
    """(column, row, looked_up) per point under rotation (cf, sf) and a shift in cells: looked_up is False for a point that
    fails the sanity rule or whose cell is outside the grid (its column and row are then meaningless)."""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 2)
    x, y = p[:, 0], p[:, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        xr = (cf * x).astype(np.float32) - (sf * y).astype(np.float32)
        yr = (sf * x).astype(np.float32) + (cf * y).astype(np.float32)
        sane = (np.abs(xr) < np.float32(1e9)) & (np.abs(yr) < np.float32(1e9))
    assert xr.dtype == yr.dtype == np.float32
    col = SIDE // 2 + np.floor(np.where(sane, xr, 0).astype(np.float64) / RES).astype(np.int64) + int(shift[0])
    row = SIDE // 2 + np.floor(np.where(sane, yr, 0).astype(np.float64) / RES).astype(np.int64) + int(shift[1])
    return col, row, sane & (col >= 0) & (col < SIDE) & (row >= 0) & (row < SIDE)


def pose_shift(L, i, pose):
    """The shift in cells of pair i of list L at lattice pose (k, ix, iy)."""
    _, nx, ny, _ = L.lattice
    o = L.origin[i] if L.origin is not None else (0, 0)
    return int(o[0]) + int(pose[1]) - (nx - 1) // 2, int(o[1]) + int(pose[2]) - (ny - 1) // 2


def log_table(V, K, floor_p):
    v = np.maximum(np.asarray(V, np.float64) / (float(K) * float(K)), floor_p)
    return np.log(v.astype(LD))


@functools.lru_cache(maxsize=None)
def _log_table_of(sigma, floor_p):
    return log_table(blur(sigma), int(taps(sigma).sum()), floor_p)


def score(points, logs, floor_p, cf, sf, shift):
    """The definition: longdouble mean of the points' log-likelihoods, `logs` the table of log(max(V / K^2, floor_p))."""
    n = len(points)
    Lf = np.log(LD(floor_p))
    if n == 0:
        return Lf
    col, row, ok = lookup_cells(points, cf, sf, shift)
    L = np.full(n, Lf, dtype=LD)
    L[ok] = logs[row[ok], col[ok]]
    return L.sum(dtype=LD) / LD(n)


def reference(L, i, pose=(0, 0, 0), logs=None):
    """The definition's score of pair i of list L at lattice pose (k, ix, iy); logs: another table (a perturbed one)."""
    n_theta, _, _, step = L.lattice
    cf, sf = rotation(float(L.theta0[i]), int(pose[0]), n_theta, step)
    logs = _log_table_of(L.sigma, L.floor_p) if logs is None else logs
    return score(L.scans[L.src[i]], logs, L.floor_p, cf, sf, pose_shift(L, i, pose))


def oracle_score(L, i, pose=(0, 0, 0)):
    n_theta, nx, ny, step = L.lattice
    o = L.origin[i] if L.origin is not None else (0, 0)
    return O.pose_score_exact(L.scans[L.src[i]], target(L.sigma), ospec(L.sigma, L.floor_p), float(L.theta0[i]),
                              O.search_spec(n_theta, nx, ny, step), pose[0], pose[1], pose[2], origin=(int(o[0]), int(o[1])))


def oracle_pose(L, i, cell_bits=16):
    """The pose the search on quantised cells returns for pair i (the oracle's exhaustive match)."""
    n_theta, nx, ny, step = L.lattice
    gs = O.grid_spec(RANGE, RES, L.sigma, L.floor_p, cell_bits)
    o = L.origin[i] if L.origin is not None else (0, 0)
    m = O.csm_match(L.scans[L.src[i]], _ogrid(L.sigma, L.floor_p, cell_bits), gs, float(L.theta0[i]), O.search_spec(n_theta, nx, ny, step),
                    origin=(int(o[0]), int(o[1])))
    return (m.itheta, m.ix, m.iy), m.sum


@functools.lru_cache(maxsize=None)
def _ogrid(sigma, floor_p, cell_bits):
    return O.grid_build(target(sigma), O.grid_spec(RANGE, RES, sigma, floor_p, cell_bits))


def interval(ref, n, K=K_EXACT):
    """(lo, hi) float32: the closed interval a float record of a score with definition `ref` over n points must lie in."""
    ref = LD(ref)
    w = np.abs(ref) * LD((K + n) * U)
    return np.float32(ref - w), np.float32(ref + w)


# ------------------------------------------------------------------------------------------------ the lists
def _list(name, sigma, scans, src, theta0, origin, lattice, forced, floor_p=FLOOR_P, tags=None):
    src = np.asarray(src, np.int32)
    L = NS(name=name, sigma=sigma, scans=[np.ascontiguousarray(s, np.float32).reshape(-1, 2) for s in scans], src=src,
           theta0=np.broadcast_to(np.asarray(theta0, np.float64), src.shape).copy(),
           origin=None if origin is None else np.asarray(origin, np.int32).reshape(len(src), 2), lattice=lattice, forced=forced,
           floor_p=floor_p, tags=tags or [""] * len(src))
    L.n_points = np.array([len(L.scans[s]) for s in src])
    L.short = bool(L.n_points.max(initial=0) <= 1088)
    return L


def _probe_origin(cells):
    c, r = cells[:, 0], cells[:, 1]
    return np.stack([(3 * c + 5 * r) % 17 - 8, (7 * c + r) % 17 - 8], axis=1)


def probe_cells(R):
    """[(tag, column, row)] of the probed cells."""
    S = SIDE
    out = []
    for row in (70, 83, BAND_ROW + 2):
        first = 16 if row != BAND_ROW + 2 else 40
        out += [("shift", c, row) for c in range(first, first + 32)]
    ends = list(range(0, 36)) + list(range(S - 36, S))
    for e in (0, S - 1):
        out += [("rim", c, e) for c in ends] + [("rim", e, r) for r in ends if r not in (0, S - 1)]
    bc, br = BLOCK_AT
    out += [("block", bc + R + dc, br + R + dr) for dc in (-1, 0, 1, 2) for dr in (-1, 0, 1, 2)]
    ec, er = EMPTY_AT
    out += [("empty", ec, er), ("empty", ec + 1, er - 1)]
    return out


def _probes(sigma, name="probes", floor_p=FLOOR_P, only=None):
    cells = [t for t in probe_cells(radius(sigma)) if only is None or t[0] in only]
    tags = [t[0] for t in cells]
    rc = np.array([(c, r) for _, c, r in cells], np.int64)
    org = _probe_origin(rc)
    scans = list(points_in_cells(rc - org)[:, None, :])
    L = _list(name, sigma, scans, np.arange(len(scans)), 0.0, org, (1, 1, 1, DEG), True, floor_p, tags)
    L.cells = rc
    return L


def _floor_between(sigma):
    """A floor_p strictly between two attainable V / K^2 of the probed cells, and those two sums."""
    P = _probes(sigma, only=("shift",))
    V = np.unique(blur(sigma)[P.cells[:, 1], P.cells[:, 0]])
    V = V[V > 0]
    assert len(V) >= 4
    a, b = int(V[len(V) // 2 - 1]), int(V[len(V) // 2])
    K2 = float(taps(sigma).sum()) ** 2
    f = (a + b) / (2.0 * K2)
    assert a / K2 < f < b / K2 and 0.0 < f < 1.0
    return f, a, b


def _sources(sigma, theta0, sizes, seed):
    """Scans of the given sizes that see the target from poses one lattice step around theta0: points of the target with a
    third of a cell of jitter, moved by the inverse of (theta0 + dk degrees, (dx, dy) cells)."""
    rng = np.random.default_rng(seed)
    tgt = target(sigma).astype(np.float64)
    out = []
    for j, n in enumerate(sizes):
        dk, dx, dy = (j % 3) - 1, ((j // 3) % 3) - 1, ((j + 1) % 3) - 1
        p = tgt[rng.integers(0, len(tgt), n)] + rng.uniform(-0.3, 0.3, (n, 2)) * RES - np.array([dx, dy]) * RES
        a = -(theta0 + dk * DEG)
        c, s = math.cos(a), math.sin(a)
        out.append(np.stack([c * p[:, 0] - s * p[:, 1], s * p[:, 0] + c * p[:, 1]], axis=1).astype(np.float32))
    return out


def _edge_points(sigma):
    """[(tag, point, origin)] of the in-grid and sanity edges (theta0 = 0: the rotated point is the point)."""
    f = np.float32
    below = lambda v: np.nextafter(f(v), f(0))
    beyond = lambda v: np.nextafter(f(v), f(np.copysign(np.inf, v)))
    row_y, col_x = f((BAND_ROW + 2 - SIDE // 2 + 0.5) * RES), f((BAND_COL + 2 - SIDE // 2 + 0.5) * RES)
    out = []
    for bad in (np.nan, np.inf, -np.inf):
        out += [("not_finite", (f(bad), row_y), (0, 0)), ("not_finite", (col_x, f(bad)), (0, 0))]
    out.append(("not_finite", (f(np.nan), f(np.nan)), (0, 0)))
    for sgn in (1.0, -1.0):
        out += [("at_1e9", (f(sgn * 1e9), row_y), (0, 0)), ("below_1e9", (below(sgn * 1e9), row_y), (0, 0)),
                ("at_1e9", (col_x, f(sgn * 1e9)), (0, 0)), ("below_1e9", (col_x, below(sgn * 1e9)), (0, 0))]
    for v in (f(-RANGE), beyond(-RANGE), below(-RANGE), f(RANGE), beyond(RANGE), below(RANGE)):
        for o in (0, 1, -1):
            out += [("rim", (v, row_y), (o, 0)), ("rim", (col_x, v), (0, o))]
    for k in range(-(SIDE // 2), SIDE // 2 + 1):
        v = f(k * RES)
        out += [("multiple", (v, row_y), (0, 0)), ("multiple", (col_x, v), (0, 0))]
    return out


@functools.lru_cache(maxsize=None)
def lists(sigma):
    """name -> list, all against target(sigma)."""
    out = {}
    out["probes"] = _probes(sigma)
    fp, a, b = _floor_between(sigma)
    out["floor"] = _probes(sigma, "floor", fp, only=("shift",))
    out["floor"].between = (a, b)
    for j, th0 in enumerate((0.0, OBLIQUE)):
        scans = _sources(sigma, th0, COUNTS, 100 + j)
        out["counts%d" % j] = _list("counts%d" % j, sigma, scans, np.arange(len(scans)), th0, None, (3, 3, 3, DEG), False)
        out["counts%d_short" % j] = _list("counts%d_short" % j, sigma, scans[:-1], np.arange(len(scans) - 1), th0, None, (3, 3, 3, DEG), False)
    # pairs with pairwise different scores: 17 scans of different sizes at different headings and centres, the pose forced
    sizes = [40 + 3 * i for i in range(max(PAIR_LISTS))]
    scans = [s for i, n in enumerate(sizes) for s in _sources(sigma, 0.05 * i, [n], 200 + i)]
    for n in PAIR_LISTS:
        i = np.arange(n)
        out["pairs%d" % n] = _list("pairs%d" % n, sigma, scans[:n], i, 0.05 * i, np.stack([i % 5 - 2, i % 3 - 1], axis=1), (1, 1, 1, DEG), True)
    E = _edge_points(sigma)
    pts = [np.array([p], np.float32) for _, p, _ in E]
    pts.append(np.array([p for _, p, o in E if o == (0, 0)], np.float32))
    out["edges"] = _list("edges", sigma, pts, np.arange(len(pts)), 0.0, [o for _, _, o in E] + [(0, 0)], (1, 1, 1, DEG), True,
                         tags=[t for t, _, _ in E] + ["all"])
    near = _sources(sigma, 0.0, [65, 257, 64, 63], 300)
    out["shift_ok"] = _list("shift_ok", sigma, near, np.arange(4), 0.0, [(7, 0), (-7, 7), (0, -7), (7, 7)], (1, 3, 3, DEG), False)
    out["shift_beyond"] = _list("shift_beyond", sigma, near[:3], np.arange(3), 0.0, [(8, 0), (0, -8), (-8, 8)], (1, 3, 3, DEG), False)
    return out


def window_shifts(L):
    """(col - R + HIT_PAD) & 31 of the probed cells tagged "shift": the bit offset of the row windows' 64-bit loads."""
    sel = np.array([t == "shift" for t in L.tags])
    return (L.cells[sel, 0] - radius(L.sigma) + HIT_PAD) & 31
