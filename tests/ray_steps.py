"""Beams whose steps need the ray's correction (nhip_ray.h: rdiv and rdiv_straight), and the crafted inputs that bring those
steps in front of the four kernels that walk the ray: K14's occ_trace_kernel, K15's fs_trace_kernel and fs_check_kernel, K21's
rs_map_kernel.

Step k of a beam is floor((2 k d + n) / (2 n)).  The device takes floorf(float(2 k d + n) * (1.0f / float(2 n))) and corrects it
by the remainder.  estimate_rdiv() below is a float32 model of that uncorrected estimate.  It is used for two things only: to
choose the beams (LOW: the estimate is one too low at the listed steps, HIGH: one too high), and as the mutant of the CPU
tests, which put it in the place of the references' `//` to prove that the compared outputs would differ if a correction were
missing.  No expected value comes from it: those are the references' (occupancy_reference, freespace_reference,
rangesig_reference), all of which divide python integers.

The device may round its reciprocal differently from numpy, so no test rests on one step: LOW names 153 steps of 8 different
n, HIGH 41 too-high steps (and one too-low) of 7 different n.  At n = 4096 the estimate is exact (1 / 8192 is a power of two), so
no beam of that length is listed.  n = 3001 has no beam with two off steps; two beams of one each are listed.

An entry is ((dx, dy), ((k, right cell, cell of the uncorrected estimate), ...)): cells as offsets from the beam's origin, the
two differ by one on the minor axis.
"""
import functools

import numpy as np

from tests import freespace_reference as FR
from tests import occupancy_reference as OR
from tests import rangesig_reference as RR

LOW = (
    ((14, -7), ((7, (7, -3), (7, -4)), (13, (13, -6), (13, -7)),)),
    ((-14, -13), ((7, (-7, -6), (-7, -7)),)),
    ((-7, 14), ((7, (-3, 7), (-4, 7)), (13, (-6, 13), (-7, 13)),)),
    ((-13, -14), ((7, (-6, -7), (-7, -7)),)),
    ((28, -14), ((7, (7, -3), (7, -4)), (13, (13, -6), (13, -7)), (15, (15, -7), (15, -8)), (23, (23, -11), (23, -12)), (25,
        (25, -12), (25, -13)), (27, (27, -13), (27, -14)),)),
    ((-21, 28), ((10, (-7, 10), (-8, 10)), (18, (-13, 18), (-14, 18)),)),
    ((-52, -39), ((10, (-10, -7), (-10, -8)), (18, (-18, -13), (-18, -14)), (38, (-38, -28), (-38, -29)), (42, (-42, -31),
        (-42, -32)),)),
    ((-26, -52), ((15, (-7, -15), (-8, -15)), (27, (-13, -27), (-14, -27)), (29, (-14, -29), (-15, -29)), (31, (-15, -31),
        (-16, -31)),)),
    ((-82, 41), ((1, (-1, 1), (-1, 0)), (3, (-3, 2), (-3, 1)), (7, (-7, 4), (-7, 3)), (13, (-13, 7), (-13, 6)), (15, (-15, 8), (-15,
        7)), (25, (-25, 13), (-25, 12)), (27, (-27, 14), (-27, 13)), (29, (-29, 15), (-29, 14)), (31, (-31, 16), (-31, 15)), (51,
        (-51, 26), (-51, 25)), (53, (-53, 27), (-53, 26)), (55, (-55, 28), (-55, 27)), (57, (-57, 29), (-57, 28)), (59, (-59, 30),
        (-59, 29)), (61, (-61, 31), (-61, 30)), (63, (-63, 32), (-63, 31)),)),
    ((1, 82), ((41, (1, 41), (0, 41)),)),
    ((41, -82), ((1, (1, -1), (0, -1)), (3, (2, -3), (1, -3)), (7, (4, -7), (3, -7)), (13, (7, -13), (6, -13)), (15, (8,
        -15), (7, -15)), (25, (13, -25), (12, -25)), (27, (14, -27), (13, -27)), (29, (15, -29), (14, -29)), (31, (16, -31),
        (15, -31)), (51, (26, -51), (25, -51)), (53, (27, -53), (26, -53)), (55, (28, -55), (27, -55)), (57, (29, -57), (28,
        -57)), (59, (30, -59), (29, -59)), (61, (31, -61), (30, -61)), (63, (32, -63), (31, -63)),)),
    ((-112, -56), ((7, (-7, -3), (-7, -4)), (13, (-13, -6), (-13, -7)), (15, (-15, -7), (-15, -8)), (23, (-23, -11), (-23,
        -12)), (25, (-25, -12), (-25, -13)), (27, (-27, -13), (-27, -14)), (29, (-29, -14), (-29, -15)), (31, (-31, -15),
        (-31, -16)), (45, (-45, -22), (-45, -23)), (47, (-47, -23), (-47, -24)), (49, (-49, -24), (-49, -25)), (51, (-51,
        -25), (-51, -26)), (53, (-53, -26), (-53, -27)), (55, (-55, -27), (-55, -28)), (57, (-57, -28), (-57, -29)), (59,
        (-59, -29), (-59, -30)), (61, (-61, -30), (-61, -31)), (63, (-63, -31), (-63, -32)), (87, (-87, -43), (-87, -44)),
        (89, (-89, -44), (-89, -45)), (91, (-91, -45), (-91, -46)), (93, (-93, -46), (-93, -47)), (95, (-95, -47), (-95,
        -48)), (97, (-97, -48), (-97, -49)), (99, (-99, -49), (-99, -50)), (101, (-101, -50), (-101, -51)), (103, (-103,
        -51), (-103, -52)), (105, (-105, -52), (-105, -53)), (107, (-107, -53), (-107, -54)), (109, (-109, -54), (-109,
        -55)), (111, (-111, -55), (-111, -56)),)),
    ((606, -303), ((63, (63, -31), (63, -32)), (125, (125, -62), (125, -63)), (127, (127, -63), (127, -64)), (247, (247,
        -123), (247, -124)), (249, (249, -124), (249, -125)), (251, (251, -125), (251, -126)), (253, (253, -126), (253,
        -127)), (255, (255, -127), (255, -128)), (491, (491, -245), (491, -246)), (493, (493, -246), (493, -247)), (495,
        (495, -247), (495, -248)), (497, (497, -248), (497, -249)), (499, (499, -249), (499, -250)), (501, (501, -250),
        (501, -251)), (503, (503, -251), (503, -252)), (505, (505, -252), (505, -253)), (507, (507, -253), (507, -254)),
        (509, (509, -254), (509, -255)), (511, (511, -255), (511, -256)),)),
    ((-289, 578), ((63, (-31, 63), (-32, 63)), (123, (-61, 123), (-62, 123)), (125, (-62, 125), (-63, 125)), (127, (-63,
        127), (-64, 127)), (245, (-122, 245), (-123, 245)), (247, (-123, 247), (-124, 247)), (249, (-124, 249), (-125,
        249)), (251, (-125, 251), (-126, 251)), (253, (-126, 253), (-127, 253)), (255, (-127, 255), (-128, 255)), (487,
        (-243, 487), (-244, 487)), (489, (-244, 489), (-245, 489)), (491, (-245, 491), (-246, 491)), (493, (-246, 493),
        (-247, 493)), (495, (-247, 495), (-248, 495)), (497, (-248, 497), (-249, 497)), (499, (-249, 499), (-250, 499)),
        (501, (-250, 501), (-251, 501)), (503, (-251, 503), (-252, 503)), (505, (-252, 505), (-253, 505)), (507, (-253,
        507), (-254, 507)), (509, (-254, 509), (-255, 509)), (511, (-255, 511), (-256, 511)),)),
    ((586, 293), ((1, (1, 1), (1, 0)), (3, (3, 2), (3, 1)), (7, (7, 4), (7, 3)), (15, (15, 8), (15, 7)), (31, (31, 16), (31,
        15)), (61, (61, 31), (61, 30)), (63, (63, 32), (63, 31)), (123, (123, 62), (123, 61)), (125, (125, 63), (125, 62)),
        (127, (127, 64), (127, 63)), (247, (247, 124), (247, 123)), (249, (249, 125), (249, 124)), (251, (251, 126), (251,
        125)), (253, (253, 127), (253, 126)), (255, (255, 128), (255, 127)), (493, (493, 247), (493, 246)), (495, (495,
        248), (495, 247)), (497, (497, 249), (497, 248)), (499, (499, 250), (499, 249)), (501, (501, 251), (501, 250)),
        (503, (503, 252), (503, 251)), (505, (505, 253), (505, 252)), (507, (507, 254), (507, 253)), (509, (509, 255), (509,
        254)), (511, (511, 256), (511, 255)),)),
)
HIGH = (
    ((2457, 2374), ((2383, (2383, 2302), (2383, 2303)),)),
    ((2383, 2457), ((2374, (2302, 2374), (2303, 2374)),)),
    ((-2457, 2390), ((2402, (-2402, 2336), (-2402, 2337)),)),
    ((4093, 2197), ((2706, (2706, 1452), (2706, 1453)), (4025, (4025, 2160), (4025, 2161)),)),
    ((2839, 4093), ((2368, (1642, 2368), (1643, 2368)), (3011, (2088, 3011), (2089, 3011)),)),
    ((-4093, 2849), ((2466, (-2466, 1716), (-2466, 1717)), (3305, (-3305, 2300), (-3305, 2301)),)),
    ((4093, -3053), ((2749, (2749, -2051), (2749, -2050)),)),
    ((4093, -2170), ((3977, (3977, -2108), (3977, -2109)),)),  # (the one too-low step of this list)
    ((2409, -4093), ((2580, (1518, -2580), (1519, -2580)), (3647, (2146, -3647), (2147, -3647)),)),
    ((4093, 2615), ((4039, (4039, 2580), (4039, 2581)), (4075, (4075, 2603), (4075, 2604)),)),
    ((4091, 2770), ((2445, (2445, 1655), (2445, 1656)), (3244, (3244, 2196), (3244, 2197)),)),
    ((2216, -4091), ((4055, (2196, -4055), (2197, -4055)), (4079, (2209, -4079), (2210, -4079)),)),
    ((4091, -4010), ((2096, (2096, -2055), (2096, -2054)),)),
    ((-3539, 4091), ((2442, (-2113, 2442), (-2112, 2442)),)),
    ((-4091, 2362), ((2611, (-2611, 1507), (-2611, 1508)), (3742, (-3742, 2160), (-3742, 2161)),)),
    ((4001, 3347), ((3845, (3845, 3216), (3845, 3217)), (3949, (3949, 3303), (3949, 3304)),)),
    ((3501, 4001), ((3989, (3490, 3989), (3491, 3989)), (3997, (3497, 3997), (3498, 3997)),)),
    ((-4001, -3967), ((2177, (-2177, -2159), (-2177, -2158)),)),
    ((-3963, -4001), ((2369, (-2347, -2369), (-2346, -2369)),)),
    ((3001, 2550), ((2472, (2472, 2100), (2472, 2101)),)),
    ((2569, -3001), ((2414, (2066, -2414), (2067, -2414)),)),
    ((4095, 2302), ((2671, (2671, 1501), (2671, 1502)), (3918, (3918, 2202), (3918, 2203)),)),
    ((2713, -4095), ((2449, (1622, -2449), (1623, -2449)), (3252, (2154, -3252), (2155, -3252)),)),
    ((3499, 2969), ((2446, (2446, 2075), (2446, 2076)),)),
    ((-3451, 3499), ((2442, (-2409, 2442), (-2408, 2442)),)),
    # (off steps within a hundred cells of the end: the only ones K15's check can hold in a 120-cell grid with the end cell)
    ((2157, 3001), ((2985, (2145, 2985), (2146, 2985)),)),
    ((3499, 2075), ((3456, (3456, 2049), (3456, 2050)),)),
    ((-3499, 2114), ((3475, (-3475, 2099), (-3475, 2100)),)),
    ((4006, -4095), ((4026, (3938, -4026), (3939, -4026)), (4072, (3983, -4072), (3984, -4072)),)),
)


# ---------------------------------------------------------------- the float32 model of the estimate
def estimate_rdiv(a, n):
    """floorf(float(2 a + n) * (1.0f / float(2 n))) in numpy float32, every operation rounded once: the device's estimate
    before its correction.  Same signature as the references' rdiv (ints or integer arrays)."""
    num = 2 * np.asarray(a, dtype=np.int64) + np.asarray(n, dtype=np.int64)
    inv = np.float32(1.0) / (2 * np.asarray(n, dtype=np.int64)).astype(np.float32)
    return np.floor(num.astype(np.float32) * inv).astype(np.int64)


def estimate_error(n, minor):
    """(k, d): the steps k in 0 .. n - 1 of a beam with this minor offset at which the estimate is off, and by how much."""
    k = np.arange(n, dtype=np.int64)
    d = estimate_rdiv(k * int(minor), n) - (2 * k * int(minor) + n) // (2 * n)
    at = np.nonzero(d)[0]
    return at, d[at]


def parts(beam):
    """(n, x_major, major sign, minor offset) of a beam (dx, dy), as the kernels split it."""
    dx, dy = beam
    n = max(abs(dx), abs(dy))
    x_major = abs(dx) >= abs(dy)
    return n, x_major, ((1 if dx > 0 else -1) if x_major else (1 if dy > 0 else -1)), (dy if x_major else dx)


def off_steps(lst):
    """[(beam, k, right cell, estimate's cell, +1 or -1: the estimate's error)] over a list."""
    out = []
    for beam, steps in lst:
        x_major = parts(beam)[1]
        for k, right, est in steps:
            out.append((beam, k, right, est, (est[1] - right[1]) if x_major else (est[0] - right[0])))
    return out


# ---------------------------------------------------------------- K14: the occupancy grid
def _all_in_one(origin, lst, spec):
    return OR.scan_of_cells(origin, [(origin[0] + b[0], origin[1] + b[1]) for b, _ in lst], spec)


def _walked(scans_origins, lst, spec):
    """[low, high]: the listed off steps whose right cell lies in the window, over every (origin, beams) that is traced."""
    n = [0, 0]
    for origin, beams in scans_origins:
        for beam, k, right, est, d in off_steps(lst):
            if beam in beams:
                x, y = origin[0] + right[0] - spec.cell_x0, origin[1] + right[1] - spec.cell_y0
                n[d > 0] += 0 <= x < spec.width and 0 <= y < spec.height
    return n


def occupancy_low_cases():
    """[(name, (xy, offsets, poses), spec, [low, high] steps in the window)]: every LOW beam whole inside the window, a scan
    per beam and all beams in one scan; the short ones again on a lattice of origins, no two rays sharing a cell."""
    cases = []
    spec = OR.make_spec(width=1300, height=1300, cell_x0=-650, cell_y0=-650)
    beams = [b for b, _ in LOW]
    scans = [OR.scan_of_cells((0, 0), [b], spec) for b in beams] + [_all_in_one((3, -2), LOW, spec)]
    cases.append(("one origin", OR.pack(scans), spec, _walked([((0, 0), beams), ((3, -2), beams)], LOW, spec)))
    short = [b for b in beams if max(abs(b[0]), abs(b[1])) <= 112]
    spec = OR.make_spec(width=1040, height=780)
    origins = [(130 + 260 * (i % 4), 130 + 260 * (i // 4)) for i in range(len(short))]
    scans = [OR.scan_of_cells(o, [(o[0] + b[0], o[1] + b[1])], spec) for o, b in zip(origins, short)]
    cases.append(("lattice of origins", OR.pack(scans), spec, _walked([(o, [b]) for o, b in zip(origins, short)], LOW, spec)))
    return cases


def occupancy_high_cases(i):
    """The windows of HIGH beam i, one per off step: max_ray_cells 4096, 3 .. 8 rows high on the off step's row, up to 16384
    wide.  Three scans: the beam alone and every HIGH beam in one scan, both from the world's (0, 0), outside the window; and
    every HIGH beam from an origin inside the window (its rays start there: the narrowing of k at a band that holds row 0)."""
    beam, steps = HIGH[i]
    cases = []
    for j, (k, right, est) in enumerate(steps):
        h = 3 + (2 * i + 3 * j) % 6
        w = (16384, 9001, 4200)[(i + j) % 3]
        x0 = min(right[0], est[0]) - (w // 2 if w < 16384 else 8192 - 7 * i)
        spec = OR.make_spec(width=w, height=h, cell_x0=x0, cell_y0=min(right[1], est[1]) - (h - 1) // 2, max_ray_cells=4096)
        inside = (right[0] - 5, spec.cell_y0 + h // 2)
        beams = [b for b, _ in HIGH]
        scans = [OR.scan_of_cells((0, 0), [beam], spec), _all_in_one((0, 0), HIGH, spec), _all_in_one(inside, HIGH, spec)]
        walked = _walked([((0, 0), [beam]), ((0, 0), beams), (inside, beams)], HIGH, spec)
        cases.append(("beam %d step %d" % (i, k), OR.pack(scans), spec, walked))
    return cases


# ---------------------------------------------------------------- K15: the check (rdiv_straight) and the trace (rdiv)
CHECK_SIDE, CHECK_RANGE = 1200, 30.0  # the check's grid: 1200 cells (range 30 m, res 0.05), the sensor's cell (600, 600)
HITS = ((10, 10), (1189, 10), (10, 1189), (1189, 1189))  # the one end cell of target 0 .. 3


def check_grid_spec():
    from nautilus_amd import csm
    return csm.grid_spec(CHECK_RANGE, FR.RES, 2.0, 1e-10, 8, 16)


def check_case(lst, name):
    """A case in the form of freespace_reference.check_cases(), on the 1200-cell grid: scans 0 .. 3 are the targets, one hit
    each in a corner of the grid, scan 4 + j is source beam j of the list, one point.  A beam is examined only if its end cell
    lies in the grid, so an off step can be held only if it lies within the grid's side of the beam's end: those steps get two
    pairs each, against the target whose corner leaves room for the rest of the beam.  In one the pair's origin brings the
    step's RIGHT cell onto the hit (through counts the beam), in the other the cell of the uncorrected estimate (it does not:
    the right cell is the hit's neighbour).  `steps` holds (beam, k, variant, the estimate's error) per pair."""
    half = CHECK_SIDE // 2
    scans = [FR.scan_of_cells([h], CHECK_SIDE, FR.RES) for h in HITS]
    scans += [((np.asarray([b], dtype=np.float64) + 0.5) * FR.RES).astype(np.float32) for b, _ in lst]
    src, tgt, origin, steps = [], [], [], []
    for j, (beam, st) in enumerate(lst):
        for k, right, est in st:
            room = [t for t, h in enumerate(HITS)
                    if all(0 <= h[a] + beam[a] - c[a] < CHECK_SIDE for c in (right, est) for a in (0, 1))]
            for variant, c in (("right", right), ("estimate", est)) if room else ():
                h = HITS[room[0]]
                src.append(4 + j)
                tgt.append(room[0])
                origin.append((h[0] - half - c[0], h[1] - half - c[1]))
                steps.append((beam, k, variant, est[0] - right[0] + est[1] - right[1]))
    n = len(src)
    return dict(name=name, scans=scans, src=np.asarray(src, np.int32), tgt=np.asarray(tgt, np.int32), theta0=np.zeros(n),
                poses=[(0, 0, 0)] * n, origin=np.asarray(origin, np.int32).reshape(n, 2), lattice=(1, 1, 1), fs=((0, 0), (2, 3)),
                steps=steps)


def check_cases():
    return [check_case(LOW, "low"), check_case(HIGH, "high")]


def check_counts(case, fs, fn=None):
    """The counts of a case under (hit_radius, end_margin) = fs, by `fn` (default: the reference's counts)."""
    from nautilus_amd import csm
    xy, off = FR.pack(case["scans"])
    return (fn or FR.counts)(xy, off, case["src"], case["tgt"], case["theta0"], FR.records(case["poses"]), check_grid_spec(),
                             csm.search_spec(*case["lattice"]), FR.make_spec(*fs), case["origin"])


def chunk_place(n, k, end_margin):
    """(chunks in the group, index of k's chunk in it) as fs_check_kernel groups the 64-step chunks of steps 0 .. n - 1 -
    end_margin: four while three or more are left, then two, then one.  None if step k is not examined."""
    k_end = n - end_margin
    if k >= k_end:
        return None
    chunks, c0 = (k_end + 63) >> 6, 0
    while True:
        size = 4 if chunks - c0 >= 3 else chunks - c0
        if (k >> 6) < c0 + size:
            return size, (k >> 6) - c0
        c0 += size


def trace_targets():
    """[(grid side, range in metres, [target points])]: every LOW beam that fits the side as an end cell of one target, and at
    side 120 each on its own as well."""
    out = []
    for side, reach in ((120, 3.0), (1200, 30.0)):
        fit = [b for b, _ in LOW if max(abs(b[0]), abs(b[1])) < side // 2]
        one = lambda beams: FR.scan_of_cells([(side // 2 + b[0], side // 2 + b[1]) for b in beams], side, FR.RES)
        out.append((side, reach, [one(fit)] + ([one([b]) for b in fit] if side == 120 else [])))
    return out


# ---------------------------------------------------------------- K21: the map signatures' walk
STRIDE = 16


def _scale(n):
    return min(65536, (254 << 16) // n)  # (value k for n <= 254; below 255 at k = n for every n)


def ray_table(entries):
    """64 rows (dx, dy, n, scale): the entries' beams, the rest a one-step ray along x"""
    rows = [(b[0], b[1], parts(b)[0], _scale(parts(b)[0])) for b, _ in entries]
    return rows + [(1, 0, 1, 65536)] * (64 - len(rows))


def map_case(entries, side, anchor, swapped, name):
    """(name, grid int8 (side, side), spec, rays, [(beam, the off steps that got a wall)]): free cells everywhere, every lattice node but `anchor` set to 50
    (passed by a ray, no anchor), and walls.  swapped = False: a wall on the right cell of each beam's FIRST off step, so the
    walk ends there, the estimate's cell free.  swapped = True: walls on the estimate's cells of ALL its off steps, the right
    cells free, so the walk passes every one of them."""
    spec = RR.make_spec(width=side, height=side, stride=STRIDE, max_ray_cells=4096, rays_per_sector=1)
    grid = np.zeros((side, side), np.int8)
    grid[STRIDE // 2::STRIDE, STRIDE // 2::STRIDE] = 50
    grid[anchor[1], anchor[0]] = 0
    # all beams leave one anchor: a wall goes only where no OTHER beam of the table passes (k = 1 .. n, the end cell included)
    paths = [{tuple(c) for c in OR.ray_cells(*b).tolist()} | {b} for b, _ in entries]
    walls = []
    for t, (beam, steps) in enumerate(entries):
        others = set().union(*(p for u, p in enumerate(paths) if u != t)) if len(paths) > 1 else set()
        clear = [(k, est if swapped else right) for k, right, est in steps if (est if swapped else right) not in others]
        clear = clear if swapped else clear[:1]
        for k, c in clear:
            x, y = anchor[0] + c[0], anchor[1] + c[1]
            assert 0 <= x < side and 0 <= y < side, (beam, k)
            grid[y, x] = 100
        walls.append((beam, tuple(s for s in steps if s[0] in [k for k, _ in clear])))
    return name, grid, spec, ray_table(entries), walls


def _reach(beam, steps, limit):
    return [s for s in steps if max(abs(s[1][0]), abs(s[1][1]), abs(s[2][0]), abs(s[2][1])) <= limit]


N_MAP_CASES = 10


@functools.lru_cache(maxsize=None)
def map_cases():
    """(built once: the CPU and the GPU tests share the maps and leave them unchanged)  LOW: one anchor in the middle of a 1297-cell map, every beam.  HIGH: a 2504-cell map and an anchor in each corner; the
    table holds the beams of that quadrant, with the off steps that lie inside the map (k below 2496)."""
    cases = []
    for swapped in (False, True):
        cases.append(map_case(LOW, 1297, (648, 648), swapped, "low %s" % ("swapped" if swapped else "right")))
    for sx, sy in ((1, 1), (-1, 1), (1, -1), (-1, -1)):
        anchor = (8 if sx > 0 else 2488, 8 if sy > 0 else 2488)
        entries = [(b, tuple(_reach(b, st, 2480))) for b, st in HIGH if b[0] * sx > 0 and b[1] * sy > 0]
        entries = [e for e in entries if e[1]]
        for swapped in (False, True):
            cases.append(map_case(entries, 2504, anchor, swapped, "high %+d%+d %s" % (sx, sy, "swapped" if swapped else "right")))
    assert len(cases) == N_MAP_CASES
    return cases


def walk(grid, spec, anchor, rays, rdiv):
    """One anchor's 64 values and end steps by the spec's text with `rdiv` as the ray's division (rays_per_sector 1, flags 0):
    ([val], [the step the walk ended at, or n + 1])."""
    g = np.asarray(grid)
    vals, ends = [], []
    for dx, dy, n, scale in rays:
        k = np.arange(1, n + 1, dtype=np.int64)
        x, y = anchor[0] + rdiv(k * dx, n), anchor[1] + rdiv(k * dy, n)
        inside = (x >= 0) & (x < spec.width) & (y >= 0) & (y < spec.height)
        v = g[np.where(inside, y, 0), np.where(inside, x, 0)].astype(np.int64)
        stop = ~inside | (v < 0) | (v >= spec.occ_min)
        val, end = 255, n + 1
        if stop.any():
            at = int(np.argmax(stop))
            end = at + 1
            if inside[at] and v[at] >= 0:
                val = min(254, (end * scale) >> 16)
        vals.append(val)
        ends.append(end)
    return vals, ends
