"""The numpy statement of the free-space check ("Free-space check"; the device form is K15,
nautilus_amd/csrc/nhip_freespace.hip), and the helpers its tests share.  Written from the spec's text and differently from
the kernel on purpose: every step of every beam is listed, the division is python's `//` (a floor division), cells are sets
of integer keys deduplicated with np.unique and tested with np.isin; there are no bands, no bitmaps, no windows and no code
shared with the product (nautilus_amd/hostside.freespace_counts is a third statement, held to this one).  The rotations are
the library's host tables (nhip_csm_rot0 / nhip_csm_delta_table), which run without a device.
"""
import math
from types import SimpleNamespace

import numpy as np

from nautilus_amd import csm

RAY_MAX = 4096   # a beam with |dx| or |dy| beyond this is `outside`
M = 1 << 15      # key of cell (x, y), -32 <= x, y < M - 32: (y + 32) * M + (x + 32)
FIELDS = ("n_points", "dropped", "outside", "hit", "free", "unknown", "through", "reserved")


def make_spec(hit_radius=2, end_margin=3, flags=0, reserved=0):
    return SimpleNamespace(hit_radius=hit_radius, end_margin=end_margin, flags=flags, reserved=reserved)


def rdiv(a, n):
    """floor((2 a + n) / (2 n)): round to nearest, halves up, on both signs (ints or integer arrays; n > 0)."""
    return (2 * a + n) // (2 * n)


def ray(dx, dy):
    """The free-cell offsets of the beam to (dx, dy), k = 0 .. n - 1, as a list of (x, y) python ints."""
    n = max(abs(int(dx)), abs(int(dy)))
    return [(rdiv(k * int(dx), n), rdiv(k * int(dy), n)) for k in range(n)]


def grid_side(grid_spec):
    return int(math.floor(2.0 * grid_spec.range / grid_spec.res))


def key(x, y):
    return (np.asarray(y, dtype=np.int64) + 32) * M + (np.asarray(x, dtype=np.int64) + 32)


def all_steps(d, counts):
    """Every step of every beam: beam b (offset d[b]) contributes steps k = 0 .. counts[b] - 1.  Returns (beam index, x
    offset, y offset) per listed step, int64."""
    d = np.asarray(d, dtype=np.int64).reshape(-1, 2)
    counts = np.maximum(np.asarray(counts, dtype=np.int64), 0)
    n = np.abs(d).max(axis=1) if len(d) else np.zeros(0, np.int64)
    beam = np.repeat(np.arange(len(d)), counts)
    k = np.arange(len(beam), dtype=np.int64) - np.repeat(np.cumsum(counts) - counts, counts)
    nn = n[beam]
    if not len(beam):
        return beam, np.zeros(0, np.int64), np.zeros(0, np.int64)
    return beam, rdiv(k * d[beam, 0], nn), rdiv(k * d[beam, 1], nn)


def target_sets(points, side, res):
    """One target scan: (H, F) as sorted int64 keys of grid cells (item 1): H its end cells, F its beams' free cells minus H."""
    half = side // 2
    p = np.asarray(points, dtype=np.float32).reshape(-1, 2)
    with np.errstate(invalid="ignore", over="ignore"):
        fl = np.floor(p.astype(np.float64) / res)
    ok = np.isfinite(p).all(axis=1) & (fl >= -half).all(axis=1) & (fl < side - half).all(axis=1)
    d = fl[ok].astype(np.int64)
    H = np.unique(key(half + d[:, 0], half + d[:, 1]))
    _, sx, sy = all_steps(d, np.abs(d).max(axis=1) if len(d) else np.zeros(0, np.int64))
    F = np.unique(key(half + sx, half + sy))
    return H, F[~np.isin(F, H)]


def cells_of_keys(keys, side):
    """Keys of grid cells as a (side, side) uint8 picture of 0 / 1, row = y (only to compare with a device plane)."""
    out = np.zeros((side, side), np.uint8)
    out[keys // M - 32, keys % M - 32] = 1
    return out


def free_plane(points, side, res):
    return cells_of_keys(target_sets(points, side, res)[1], side)


def rotations(theta0, search):
    """(cf, sf) float32 per (pair, rotation index): item 3 of the CSM spec from the library's host tables."""
    rot0 = csm.rot0_table(np.asarray(theta0, dtype=np.float64).reshape(-1))
    delta = csm.delta_table(search)
    c = rot0[:, None, 0] * delta[None, :, 0] - rot0[:, None, 1] * delta[None, :, 1]
    s = rot0[:, None, 1] * delta[None, :, 0] + rot0[:, None, 0] * delta[None, :, 1]
    return c.astype(np.float32), s.astype(np.float32)


def pair_counts(src_points, H, F, cf, sf, shift, side, res, fs_spec):
    """One pair (items 2-5): the eight counts as python ints."""
    f = np.float32
    half = side // 2
    q = np.asarray(src_points, dtype=f).reshape(-1, 2)
    with np.errstate(invalid="ignore", over="ignore"):
        x = (f(cf) * q[:, 0]).astype(f) - (f(sf) * q[:, 1]).astype(f)
        y = (f(sf) * q[:, 0]).astype(f) + (f(cf) * q[:, 1]).astype(f)
        v = np.stack([x, y], axis=1).astype(f)
        fin = np.isfinite(v).all(axis=1)
        fl = np.floor(v.astype(np.float64) / res)
    dropped = int((~fin).sum())
    sx, sy = int(shift[0]), int(shift[1])
    r = int(fs_spec.hit_radius)
    short = fin & (np.abs(fl) <= RAY_MAX).all(axis=1)
    d = fl[short].astype(np.int64)                       # the unshifted cell offsets: what a beam is made of
    cx, cy = half + d[:, 0] + sx, half + d[:, 1] + sy
    inside = (cx >= 0) & (cx < side) & (cy >= 0) & (cy < side)
    outside = int((fin & ~short).sum()) + int((~inside).sum())
    d, cx, cy = d[inside], cx[inside], cy[inside]
    # every cell of every point's neighbourhood, listed: (points, (2 r + 1)^2) keys
    wi, wj = np.meshgrid(np.arange(-r, r + 1), np.arange(-r, r + 1))
    near = np.isin(key(cx[:, None] + wi.reshape(1, -1), cy[:, None] + wj.reshape(1, -1)), H).any(axis=1)
    in_f = np.isin(key(cx, cy), F)
    klass = np.where(near, "hit", np.where(in_f, "free", "unknown")).tolist()
    n = np.abs(d).max(axis=1) if len(d) else np.zeros(0, np.int64)
    beam, ux, uy = all_steps(d, n - int(fs_spec.end_margin))  # k = 0 .. n - 1 - end_margin
    rx, ry = half + sx + ux, half + sy + uy
    ok = (rx >= 0) & (rx < side) & (ry >= 0) & (ry < side)      # ray cells outside the grid are skipped one by one
    struck = np.zeros(len(ok), bool)
    struck[ok] = np.isin(key(rx[ok], ry[ok]), H)
    through = len(np.unique(beam[struck]))
    return [len(q), dropped, outside, klass.count("hit"), klass.count("free"), klass.count("unknown"), through, 0]


def counts(xy, offsets, pair_src, pair_tgt, theta0, matches, grid_spec, search, fs_spec=None, pair_origin=None):
    """The whole check: int32 (n, 8).  pair_tgt are scan ids."""
    fs_spec = make_spec() if fs_spec is None else fs_spec
    xy = np.asarray(xy, dtype=np.float32).reshape(-1, 2)
    off = np.asarray(offsets, dtype=np.int64)
    side, res = grid_side(grid_spec), float(grid_spec.res)
    cf, sf = rotations(theta0, search)
    sets = {}
    out = np.zeros((len(pair_src), 8), np.int32)
    for i, (s, t) in enumerate(zip(pair_src, pair_tgt)):
        m = matches[i]
        if m["itheta"] < 0:
            out[i] = -1
            continue
        if int(t) not in sets:
            sets[int(t)] = target_sets(xy[off[t]:off[t + 1]], side, res)
        H, F = sets[int(t)]
        o = (0, 0) if pair_origin is None else pair_origin[i]
        shift = (int(o[0]) + int(m["ix"]) - (search.nx - 1) // 2, int(o[1]) + int(m["iy"]) - (search.ny - 1) // 2)
        out[i] = pair_counts(xy[off[s]:off[s + 1]], H, F, cf[i, int(m["itheta"])], sf[i, int(m["itheta"])], shift, side, res, fs_spec)
    return out


def share(c):
    """(free + through) / (hit + free + unknown) of one record (0 with an empty denominator)."""
    den = int(c[3]) + int(c[4]) + int(c[5])
    return (int(c[4]) + int(c[6])) / den if den else 0.0


# ---------------------------------------------------------------- crafted inputs
def scan_of_cells(cells, side, res):
    """A scan (sensor frame = grid frame) whose returns lie at the centres of the GRID cells `cells` ((x, y), the sensor's
    own cell being (side // 2, side // 2)): float32 (n, 2)."""
    c = np.asarray(cells, dtype=np.float64).reshape(-1, 2)
    return ((c - side // 2 + 0.5) * res).astype(np.float32)


def pack(scans):
    xy = np.concatenate([np.asarray(s, np.float32).reshape(-1, 2) for s in scans]) if scans else np.zeros((0, 2), np.float32)
    off = np.concatenate([[0], np.cumsum([len(np.asarray(s).reshape(-1, 2)) for s in scans])]).astype(np.int32)
    return xy, off


def records(poses):
    """Match records {itheta, ix, iy, 0.0} from (itheta, ix, iy) triples; a negative itheta is the rejected record."""
    m = np.zeros(len(poses), dtype=csm.MATCH_DTYPE)
    for i, (k, ix, iy) in enumerate(poses):
        m[i] = (-1, -1, -1, -np.inf) if k < 0 else (k, ix, iy, 0.0)
    return m


# ---------------------------------------------------------------- crafted cases (a 120-cell grid: range 3 m, res 0.05, max_shift 8)
SIDE, RES, HALF = 120, 0.05, 60


def small_grid_spec(cell_bits=16):
    return csm.grid_spec(3.0, RES, 2.0, 1e-10, 8, cell_bits)


def rim_cells(side, every=1):
    c = [(x, 0) for x in range(0, side, every)] + [(x, side - 1) for x in range(0, side, every)] + \
        [(0, y) for y in range(0, side, every)] + [(side - 1, y) for y in range(0, side, every)]
    return c + [(0, 0), (side - 1, 0), (0, side - 1), (side - 1, side - 1)]


def random_points(n, seed, reach=2.9):
    """n points anywhere in the grid (not cell centres), seeded."""
    return np.random.default_rng(seed).uniform(-reach, reach, (n, 2)).astype(np.float32)


def plane_cases():
    """name -> target points on the 120-cell grid (the free plane alone is checked)."""
    cell = lambda cells: scan_of_cells(cells, SIDE, RES)
    bad = np.array([[np.nan, 0.1], [0.1, np.nan], [np.inf, 0.0], [0.0, -np.inf], [3.0, 0.0], [0.0, 3.0], [-3.0001, 0.0], [1e9, 1e9],
                    [3.4e38, -3.4e38], [-3.0, -3.0], [2.9999, 2.9999]], np.float32)
    cases = {
        "end_on_another_beam": cell([(70, 60), (80, 60), (60, 75), (60, 90), (75, 75), (90, 90)]),
        "rims_and_corners": cell(rim_cells(SIDE, 7)),
        "duplicate_ends": cell([(100, 83)] * 5 + [(20, 31)] * 70 + [(100, 83)]),
        "sensor_cell": cell([(60, 60), (60, 60), (61, 60), (60, 59)]),
        "sign_asymmetry": cell([(64, 62), (56, 58), (62, 64), (58, 56), (64, 58), (56, 62)]),
        "bad_points": np.concatenate([bad, cell([(10, 100), (110, 15)]), bad[::-1]]),
    }
    for n in (0, 1, 63, 64, 65, 1081, 1300):
        cases["points_%d" % n] = random_points(n, 100 + n)
    return cases


def seam_target(side=1200):
    """One target on a 1200-cell grid whose rays cross every band seam of the device form (raster rows in bands of 396: grid
    rows 363|364, 759|760, 1155|1156) at many slopes, both ways."""
    ends = rim_cells(side, 13) + [(x, y) for y in (362, 363, 364, 365, 758, 759, 760, 761, 1154, 1155, 1156, 1157) for x in range(3, side, 97)]
    return scan_of_cells(ends, side, 0.05)


def check_cases():
    """The crafted pairs: dicts of scans (list of point arrays), src / tgt (scan ids), theta0, poses ((itheta, ix, iy); itheta < 0:
    a rejected record), origin (n, 2) or None, lattice (n_theta, nx, ny) and fs: the (hit_radius, end_margin) settings to run."""
    cell = lambda cells: scan_of_cells(cells, SIDE, RES)
    rng = np.random.default_rng(7)
    cases = []

    def add(name, scans, src, tgt, poses=None, theta0=None, origin=None, lattice=(1, 1, 1), fs=((2, 3),)):
        n = len(src)
        cases.append(dict(name=name, scans=scans, src=np.asarray(src, np.int32), tgt=np.asarray(tgt, np.int32),
                          theta0=np.zeros(n) if theta0 is None else np.asarray(theta0, np.float64),
                          poses=[(0, 0, 0)] * n if poses is None else poses,
                          origin=None if origin is None else np.asarray(origin, np.int32).reshape(n, 2), lattice=lattice, fs=fs))

    # ---- classes: every bit offset of the raster's row windows, the rim, every radius
    wall = [tuple(c) for c in rng.integers(0, SIDE, (150, 2))] + rim_cells(SIDE, 11)
    rows = (0, 1, 17, 59, 60, 118, 119)
    probe = [(x, y) for y in rows for x in range(0, 64)] + [(x, y) for y in rows for x in range(56, 120)] + rim_cells(SIDE, 5)
    add("bit_offsets_and_rim", [cell(wall), cell(probe)], [1], [0], fs=((0, 3), (1, 3), (2, 3), (16, 3)))
    add("hit_wins_over_free", [cell([(70, 60), (80, 60)]), cell([(69, 60), (68, 60), (67, 60), (79, 60), (70, 60), (71, 60), (85, 60), (70, 61)])],
        [1], [0], fs=((0, 0), (1, 0), (2, 0)))
    # ---- a shift that pushes points, then the sensor, out of the grid
    shifts = [(0, 0), (8, 0), (0, -8), (50, 0), (59, 59), (60, 0), (61, 0), (-61, 0), (0, 200), (-119, -119), (100000, -100000),
              (2147483647, -2147483648)]
    add("shift_out_of_the_grid", [random_points(400, 1), random_points(300, 2)], [1] * len(shifts), [0] * len(shifts), origin=shifts)
    # ---- the rotation arithmetic: all 61 rotations of one pair, and a searched 3 x 3 x 3 lattice with an origin
    add("rotations_61", [random_points(500, 3), random_points(300, 4)], [1] * 61, [0] * 61, poses=[(k, 0, 0) for k in range(61)],
        theta0=[0.37] * 61, lattice=(61, 1, 1))
    p27 = [(k, i, j) for k in range(3) for i in range(3) for j in range(3)]
    add("lattice_3x3x3", [random_points(500, 5), random_points(300, 6)], [1] * 27, [0] * 27, poses=p27, theta0=[-2.1] * 27,
        origin=[(3, -2)] * 27, lattice=(3, 3, 3))
    # ---- through: a hit exactly at step n - 1 - end_margin and one step beyond; margins 0, 3 and >= n; rays partly outside
    tgt_hits = cell([(67, 60), (60, 66), (52, 52), (15, 60)])
    beams = cell([(70, 60), (60, 70), (62, 60), (50, 50), (55, 55), (60, 60), (90, 60)])
    add("through_margins", [tgt_hits, beams], [1], [0], fs=((0, 0), (0, 3), (0, 64), (2, 3), (2, 7)))
    add("through_rays_outside", [tgt_hits, beams], [1, 1, 1], [0, 0, 0], origin=[(-70, 0), (-45, 0), (0, 75)], fs=((0, 0), (0, 3)))
    # ---- beams of the greatest admitted length (|d| up to 4096, one beyond): each pair's origin brings ONE far point into the
    # grid, so its ray crosses the grid in its last steps only (the ray's arithmetic at its int32 bound, at many slopes)
    far = [(4096, 1000), (-4095, 4096), (3000, -2999), (2049, 2047), (-4096, -4096), (1, 4096), (4097, 0), (-2048, 1), (4096, 0)]
    far_pts = ((np.asarray(far, dtype=np.float64) + 0.5) * RES).astype(np.float32)
    sparse = [tuple(c) for c in rng.integers(0, SIDE, (100, 2))]  # (about half of the rays meet a hit inside the grid)
    ends = [(j, s) for j in range(len(far)) for s in range(5)]
    add("longest_beams", [cell(sparse), far_pts], [1] * len(ends), [0] * len(ends),
        origin=[(10 + 9 * s - far[j][0], 5 + 11 * s - far[j][1]) for j, s in ends], fs=((0, 0), (2, 3), (0, 64)))
    # ---- source scans of every size around the wave, one target
    sizes = (0, 1, 63, 64, 65, 1081, 1300)
    add("source_sizes", [random_points(700, 8)] + [random_points(n, 200 + n) for n in sizes], list(range(1, len(sizes) + 1)),
        [0] * len(sizes), theta0=[0.1 * i for i in range(len(sizes))])
    # ---- sources with points that are dropped: non-finite before or after rotation
    junk = np.array([[np.nan, 0.0], [np.inf, 1.0], [1.0, -np.inf], [3.4e38, 3.4e38], [1e9, 0.0], [250.0, 0.0], [0.0, -204.8], [0.0, -204.86]], np.float32)
    add("dropped_and_far", [random_points(300, 9), np.concatenate([junk, random_points(50, 10)])], [1, 1], [0, 0], theta0=[0.0, 0.8])
    # ---- lists of 1 .. 17 pairs, rejected records interleaved
    scans = [random_points(400, 20 + i) for i in range(4)]
    for n in range(1, 18):
        src, tgt = [(i % 3) + 1 for i in range(n)], [(i * 7) % 4 for i in range(n)]
        poses = [(-1, -1, -1) if (i % 3 == 1 and n > 2) else (i % 3, (i * 2) % 3, (i + 1) % 3) for i in range(n)]
        add("list_%d" % n, scans, src, tgt, poses=poses, theta0=[0.05 * i - 0.3 for i in range(n)], lattice=(3, 3, 3))
    return cases


def case_counts(case, fs, fn=None):
    """The counts of a crafted case under (hit_radius, end_margin) = fs, by `fn` (default: counts above)."""
    xy, off = pack(case["scans"])
    search = csm.search_spec(*case["lattice"])
    return (fn or counts)(xy, off, case["src"], case["tgt"], case["theta0"], records(case["poses"]), small_grid_spec(), search,
                          make_spec(*fs), case["origin"])
