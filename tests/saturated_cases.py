"""Saturated tables and the longest admitted scans: inputs at which every packed 16-bit field of the matcher's kernels holds
the largest value its limit admits, and the closed forms of what the matcher must report on them.  No GPU, no library.

Every matcher kernel adds 8-bit cell values in 16-bit fields and unpacks before a field can wrap; each limit is derived for
cells of 255 throughout (nhip_csm.hip SWAR_START_MAX: 255 points per alignment class; nhip_bnb_bounds.h LANE_WEIGHT: 4 x 64 x
255; nhip_bnb_exact.h SEG_CHUNKS: 8 x 32 x 255; nhip_bnb_origin.h cache_origins: 257 points per group of 8 lanes = 65,535).
A table built from a range scan reaches the top level almost nowhere, so these inputs are built the other way round:

THE GEOMETRY is small: range 6.0 m, res 0.05 (S = 240), sigma 2 (R = 6), max_shift 12 (pad 40), floor_p 1e-10.  Lattice L
(7 x 25 x 25, 1 degree; the strip kernels when every add is asked for), lattice S (5 x 13 x 13: 169 translations, the kernel
whose lanes are poses), lattice T (1 x 3 x 3, the longest 8-bit scan's).

THE TARGETS have one point per hit cell, at cell centres.  A cell is at the top level where its whole 13 x 13 blur window is hit
(V = K^2, log 1 = 0) -- and, the quantiser rounding to nearest, where the window lacks so little that the level still rounds
up: reach(bits) columns on each axis (0 at 16 bits, 2 at 8 bits; derived below from the definition, checked against the
oracle in tests/test_saturated_cases_cpu.py).
  plateau     a centred square of 132 x 132 hit cells: the centred 120 x 120 cells are at the top level, and every lookup of
              every source at every pose of L and S falls inside them
  corner      the block x >= x0, y >= y0: of the cells a cluster in the centre cell reaches on L, (132, 132) alone -- the LAST
              translation -- is at the top level; its neighbours lie on the near-saturated rim (the ramp is 2 R cells wide,
              further out the table is at the floor)
  corner_lo   its mirror image x <= x1, y <= y1: (108, 108) alone, the FIRST translation
  half        the half plane x >= 114: top level from column 120 on, the ramp beside it

THE SOURCES are clusters of COINCIDENT points: one float32 point n times, 0.3 cells inside cell (CENTRE + dx, CENTRE) with
dx = -2 .. 1.  The lattices rotate by at most 3 degrees, which moves such a point by under 0.1 cells: every rotation leaves
it in its cell, and the sum of a pose is n times ONE cell of the image.  dx selects the alignment class (window start
column) & 3 of the strip kernels: (148 + dx) & 3 on L, (154 + dx) & 3 on S -- all four on either lattice.
  co<n>@<j>     n points in the cell of class j on L (dx = (j + 2) % 4 - 2), n in COUNTS
  four          four clusters of 300 points, one per class, dealt in chunks of 64 points: all four register sets fill together
  stagger191    63 points of one class and 1 of another in the first chunk of 64, then three chunks of the first class: 191 points
                of it are added when the fourth chunk starts, the most at which the strip kernel still starts one
                (SWAR_START_MAX), and its fields end at 255 points, the most they ever hold (FLUSH_POINTS)
  stagger194    2 + 62, then four chunks: 194 points when the fifth chunk would start -- it must wait for an unpack, or a field
                would hold 258 points
  lanes258      4096 points in the centre cell, one point 8 cells away, one in the centre cell again: 64 runs of 64 points
                and two of one.  The bounds kernel gathers 64 runs per pass, one per lane; a second pass without a reduction
                in between would put 65 + 65 + 64 + 64 = 258 points into the fields lanes 0 .. 3 share (LANE_WEIGHT)
  spread1081    1081 distinct points on a circle of 1.5 m (not coincident; on `plateau` every lookup is at the top level)
  corner_first  1088 points in the centre cell, for `corner_lo`;  corner_last  2049 points, for `corner`.  On S the pair's
                search centre (pair_origin -6 | +6) puts the same cell at the first | last translation.
  long16        32,768 points (0x7fffffff // 65535), long8  8,421,504 points (0x7fffffff // 255): the longest scans whose
                largest possible sum the int32 records hold
"""
import functools
import math
from types import SimpleNamespace as NS

import numpy as np

from tests import grid_reference as G

RANGE, RES, SIGMA, FLOOR_P, MAX_SHIFT = 6.0, 0.05, 2.0, 1e-10, 12
SIDE, R, PAD, CENTRE = 240, 6, 40, 120
DEG = math.radians(1.0)
LATTICES = {"L": (7, 25, 25, DEG), "S": (5, 13, 13, DEG), "T": (1, 3, 3, DEG)}
COUNTS = (1, 63, 64, 65, 255, 256, 257, 258, 319, 320, 321, 1087, 1088, 1089, 1152, 2047, 2048, 2049, 4096, 4097)
SHORT = 1088  # the longest scan of the by-rotation forms (NHIP_SHORT_SCAN_POINTS)
BLOCK, TOP = 132, 120
TARGETS = ("plateau", "corner", "corner_lo", "half")
HALF_X0 = CENTRE - R
CORNER_POSE = {"corner_first": "first", "corner_last": "last"}


def levels(bits):
    return 65535 if bits == 16 else 255


def max_pts(bits):
    return 0x7fffffff // levels(bits)


# ---- the table's definition, as far as these targets need it -----------------------------------------------------------
def taps():
    """Integer blur taps round(16384 g_i / sum g) and their sum K."""
    g = [math.exp(-(i * i) / (2.0 * SIGMA * SIGMA)) for i in range(-R, R + 1)]
    t = [int(math.floor(16384.0 * v / sum(g) + 0.5)) for v in g]
    return t, sum(t)


def level_of(mx, my, bits):
    """The cell value where the blur window lacks its outer mx columns and my rows, everything else hit."""
    t, K = taps()
    V = (K - sum(t[:mx])) * (K - sum(t[:my]))
    Lf = math.log(FLOOR_P)
    step = -Lf / levels(bits)
    q = math.floor((math.log(max(V / (K * K), FLOOR_P)) - Lf) / step + 0.5)
    return int(min(max(q, 0), levels(bits)))


@functools.lru_cache(maxsize=None)
def reach(bits):
    """The largest m at which a window that lacks m columns AND m rows still rounds to the top level, while one more column
    does not: the cell (x0 + R - m, y0 + R - m) of a block x >= x0, y >= y0 is then the only top-level cell of the
    rectangle up to it."""
    m = max(k for k in range(R) if level_of(k, k, bits) == levels(bits))
    assert level_of(m + 1, m, bits) < levels(bits) and level_of(m, m + 1, bits) < levels(bits)
    return m


def _cells(xs, ys):
    return np.stack(np.meshgrid(xs, ys, indexing="xy"), axis=-1).reshape(-1, 2)


def target_cells(name, bits):
    """Hit cells (column, row) of a target."""
    if name == "plateau":
        return G._block(CENTRE - BLOCK // 2, CENTRE + BLOCK // 2, SIDE)
    if name == "corner":  # the first top-level cell of the diagonal is (CENTRE + 12, CENTRE + 12)
        return G._block(CENTRE + MAX_SHIFT - R + reach(bits), SIDE, SIDE)
    if name == "corner_lo":
        return G._block(0, CENTRE - MAX_SHIFT + R - reach(bits) + 1, SIDE)
    if name == "half":
        return _cells(np.arange(HALF_X0, SIDE), np.arange(SIDE))
    raise KeyError(name)


def target(name, bits):
    return G.cell_centres(target_cells(name, bits), SIDE, RES)


def plateau_square():
    """(lo, hi): rows and columns lo .. hi - 1 of `plateau` are at the top level."""
    return CENTRE - TOP // 2, CENTRE + TOP // 2


# ---- the sources --------------------------------------------------------------------------------------------------------
def cluster_point(cell):
    """The float32 point 0.3 cells inside cell (column, row)."""
    return np.array([(cell[0] - CENTRE + 0.3) * RES, (cell[1] - CENTRE + 0.3) * RES], np.float32)


def cluster(cell, n):
    return np.tile(cluster_point(cell), (n, 1))


def class_cell(j):
    """The cell whose window start column has class j on lattice L."""
    return (CENTRE + (j + 2) % 4 - 2, CENTRE)


def class_of(cell, lattice):
    hx = (LATTICES[lattice][1] - 1) // 2
    return (cell[0] - hx + PAD) & 3


def _four():
    left, parts = [300] * 4, []
    while any(left):
        for j in range(4):
            k = min(64, left[j])
            parts.append(cluster(class_cell(j), k))
            left[j] -= k
    return np.concatenate(parts)


def _stagger(k, chunks):
    a, b = class_cell(0), class_cell(1)
    return np.concatenate([cluster(a, k), cluster(b, 64 - k), cluster(a, 64 * (chunks - 1))])


def _lanes258():
    c = (CENTRE, CENTRE)
    return np.concatenate([cluster(c, 4096), cluster((CENTRE + 8, CENTRE), 1), cluster(c, 1)])


def _spread():
    a = 2.0 * math.pi * np.arange(1081) / 1081.0
    return np.stack([1.5 * np.cos(a), 1.5 * np.sin(a)], axis=1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def sources():
    """name -> NS(name, points, n, cell: the one cell of a coincident source or None, cls: its class on L)."""
    out = {}
    for n in COUNTS:
        for j in range(4):
            name = "co%d@%d" % (n, j)
            out[name] = NS(name=name, points=cluster(class_cell(j), n), n=n, cell=class_cell(j), cls=j)
    out["four"] = NS(name="four", points=_four(), n=1200, cell=None, cls=None)
    for name, pts in (("stagger191", _stagger(63, 4)), ("stagger194", _stagger(2, 5)), ("lanes258", _lanes258())):
        out[name] = NS(name=name, points=pts, n=len(pts), cell=None, cls=None)
    out["spread1081"] = NS(name="spread1081", points=_spread(), n=1081, cell=None, cls=None)
    for name, n in (("corner_first", 1088), ("corner_last", 2049)):
        out[name] = NS(name=name, points=cluster((CENTRE, CENTRE), n), n=n, cell=(CENTRE, CENTRE), cls=class_of((CENTRE, CENTRE), "L"))
    for s in out.values():
        s.points.setflags(write=False)
    return out


def long_source(bits):
    """The longest admitted scan of a cell width (`long16` | `long8`), and the scan of one point more."""
    n = max_pts(bits)
    name = "long%d" % bits
    return NS(name=name, points=cluster((CENTRE, CENTRE), n), n=n, cell=(CENTRE, CENTRE), cls=class_of((CENTRE, CENTRE), "L"))


def groups():
    """The lists the GPU test matches: scans of at most 1088 points (the by-rotation forms take such a list) and longer ones."""
    S = sources()
    return {"short": [k for k, s in S.items() if s.n <= SHORT], "long": [k for k, s in S.items() if s.n > SHORT]}


def pairs(names, lattice):
    """(source name, target name, (origin x, origin y)) of a list: every source on every target at the lattice's centre, and
    on S the corner sources once more with the search centre that puts their cell at the first | last translation."""
    out = [(s, t, (0, 0)) for s in names for t in TARGETS]
    if lattice == "S":
        o = MAX_SHIFT - (LATTICES["S"][1] - 1) // 2
        out += [(s, t, org) for s, t, org in (("corner_first", "corner_lo", (-o, -o)), ("corner_last", "corner", (o, o))) if s in names]
    return out


def corner_pose(name, lattice):
    """(target, origin, (itheta, ix, iy)) of the record a corner source must give: the unique top-level translation, and of
    its equal rotations the first."""
    _, nx, ny, _ = LATTICES[lattice]
    o = MAX_SHIFT - (nx - 1) // 2
    if CORNER_POSE[name] == "first":
        return "corner_lo", (-o, -o), (0, 0, 0)
    return "corner", (o, o), (0, nx - 1, ny - 1)


# ---- where the kernels see a source -------------------------------------------------------------------------------------
def rotation(th0, k, n_theta, theta_step):
    """(cos, sin) of rotation k as the kernels compose it: R(theta0) R(delta_k) in double, rounded to float once."""
    c0, s0 = math.cos(th0), math.sin(th0)
    d = (k - (n_theta - 1) // 2) * theta_step
    cd, sd = math.cos(d), math.sin(d)
    return np.float32(c0 * cd - s0 * sd), np.float32(s0 * cd + c0 * sd)


def origins(pts, cf, sf, hx, hy, cx=0, cy=0):
    """Stored-grid (row, col) of the top-left lookup cell of every point (tests/level2_runs.py origins, on this geometry)."""
    x, y = pts[:, 0].astype(np.float32), pts[:, 1].astype(np.float32)
    xr = (cf * x).astype(np.float32) - (sf * y).astype(np.float32)
    yr = (sf * x).astype(np.float32) + (cf * y).astype(np.float32)
    ix = np.floor(xr.astype(np.float64) / RES).astype(np.int64)
    iy = np.floor(yr.astype(np.float64) / RES).astype(np.int64)
    col = np.clip(SIDE // 2 + ix + cx, -hx - 1, SIDE + hx)
    row = np.clip(SIDE // 2 + iy + cy, -hy - 1, SIDE + hy)
    return row - hy + PAD, col - hx + PAD


def rotations(pts, lattice, origin=(0, 0)):
    n_theta, nx, ny, step = LATTICES[lattice]
    for k in range(n_theta):
        cf, sf = rotation(0.0, k, n_theta, step)
        yield origins(pts, cf, sf, (nx - 1) // 2, (ny - 1) // 2, origin[0], origin[1])


# ---- the closed forms ---------------------------------------------------------------------------------------------------
def closed_volume(image, n, cell, lattice, origin=(0, 0)):
    """volume[k, ix, iy] = n * image[cell + origin + (ix - hx, iy - hy)] for every k: the sums of n coincident points in `cell`
    on the (S x S, [row][column]) image of a target."""
    n_theta, nx, ny, _ = LATTICES[lattice]
    xs = cell[0] + origin[0] + np.arange(nx) - (nx - 1) // 2
    ys = cell[1] + origin[1] + np.arange(ny) - (ny - 1) // 2
    assert min(xs.min(), ys.min()) >= 0 and max(xs.max(), ys.max()) < SIDE
    plane = np.asarray(image)[np.ix_(ys, xs)].T.astype(np.int64) * int(n)
    return np.broadcast_to(plane, (n_theta, nx, ny))


def first_maximum(volume):
    """((itheta, ix, iy), sum) of the record: the largest sum at the smallest linear index."""
    lin = int(np.argmax(volume.reshape(-1)))  # (numpy returns the first of equal maxima)
    return tuple(int(v) for v in np.unravel_index(lin, volume.shape)), int(volume.reshape(-1)[lin])


def score_of(sums, n, bits):
    """The record's score float32(Lf + step * sum / n), formed in double."""
    Lf = math.log(FLOOR_P)
    step = -Lf / float(levels(bits))
    return (Lf + step * np.asarray(sums, np.float64) / float(n)).astype(np.float32)
