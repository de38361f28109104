"""The numpy statement of the occupancy grid ("Occupancy grid"; the device form is K14,
nautilus_amd/csrc/nhip_occupancy.hip), and the helpers its tests share.  Written from the spec's text and differently from the
kernel on purpose: every step of every beam of a scan is listed, the division is python's `//` (a floor division), a scan's
cells are deduplicated with np.unique on their keys and H is taken out of F with np.isin; there are no bands, no bitmaps and
no code shared with the product.

A spec is anything with the fields of nhip_occupancy_spec_t as attributes (a ctypes struct, or make_spec() below).
"""
from types import SimpleNamespace

import numpy as np

from tests.vectorize_reference import pose_affines

FIELDS = ("res", "cell_x0", "cell_y0", "width", "height", "max_ray_cells", "min_obs", "occ_permille", "free_permille", "flags",
          "reserved")
ACCUMULATE = 1
LIMIT = 2.0 ** 62  # a floor of this magnitude or more does not fit


def make_spec(**kw):
    s = SimpleNamespace(res=0.05, cell_x0=0, cell_y0=0, width=1, height=1, max_ray_cells=640, min_obs=1, occ_permille=650,
                        free_permille=196, flags=0, reserved=0)
    for k, v in kw.items():
        assert k in FIELDS, k
        setattr(s, k, v)
    return s


def rdiv(a, n):
    """floor((2 a + n) / (2 n)): round to nearest, halves up, on both signs (ints or integer arrays; n > 0)."""
    return (2 * a + n) // (2 * n)


def ray_cells(dx, dy):
    """The free-cell offsets of one beam whose end cell is (dx, dy) from its origin cell: int64 (n, 2), k = 0 .. n - 1."""
    n = max(abs(int(dx)), abs(int(dy)))
    k = np.arange(n, dtype=np.int64)
    if n == 0:
        return np.zeros((0, 2), np.int64)
    return np.stack([rdiv(k * int(dx), n), rdiv(k * int(dy), n)], axis=1)


def beams(points, affine, spec):
    """One scan: (origin cell int64 (2,), d int64 (kept, 2): end cell minus origin cell of every kept beam, counts = (traced,
    long, dropped)) -- or None if the scan is dropped."""
    f = np.float32
    c, s, tx, ty = (f(v) for v in affine)
    if not (np.isfinite(tx) and np.isfinite(ty)):
        return None
    with np.errstate(over="ignore", invalid="ignore"):
        fo = np.floor(np.array([tx, ty], dtype=np.float64) / spec.res)
    if not (np.abs(fo) < LIMIT).all():
        return None
    p = np.asarray(points, dtype=f).reshape(-1, 2)
    with np.errstate(invalid="ignore", over="ignore"):
        x = ((c * p[:, 0]).astype(f) + ((-s) * p[:, 1]).astype(f)).astype(f) + tx
        y = ((s * p[:, 0]).astype(f) + (c * p[:, 1]).astype(f)).astype(f) + ty
        w = np.stack([x.astype(f), y.astype(f)], axis=1).astype(np.float64)
        fin = np.isfinite(w).all(axis=1)
        fl = np.floor(w / spec.res)
        fits = fin & (np.abs(fl) < LIMIT).all(axis=1)
        d = fl - fo[None, :]  # (in double, before any conversion to integer)
        long_ = fits & (np.abs(d) > spec.max_ray_cells).any(axis=1)
    kept = fits & ~long_
    return fo.astype(np.int64), d[kept].astype(np.int64), (int(kept.sum()), int(long_.sum()), int((~fits).sum()))


def scan_sets(points, affine, spec):
    """One scan: (H, F, counts) -- H and F int64 (m, 2) world cells (unique rows) -- or None if the scan is dropped."""
    b = beams(points, affine, spec)
    if b is None:
        return None
    o, dk, counts = b
    H = np.unique(dk, axis=0) if len(dk) else np.zeros((0, 2), np.int64)
    # every step of every distinct beam (equal (dx, dy) give equal cells)
    n = np.abs(H).max(axis=1) if len(H) else np.zeros(0, np.int64)
    rep = np.repeat(np.arange(len(H)), n)
    k = np.arange(len(rep), dtype=np.int64) - np.repeat(np.cumsum(n) - n, n)
    nn = n[rep]
    steps = np.stack([rdiv(k * H[rep, 0], nn), rdiv(k * H[rep, 1], nn)], axis=1) if len(rep) else np.zeros((0, 2), np.int64)
    B = 1 << 20  # offsets are within +-4096: a key per offset
    key = lambda a: (a[:, 1] + (B >> 1)) * B + (a[:, 0] + (B >> 1))
    fk = np.unique(key(steps))
    fk = fk[~np.isin(fk, key(H))]
    F = np.stack([fk % B - (B >> 1), fk // B - (B >> 1)], axis=1)
    return H + o[None, :], F + o[None, :], counts


def in_window(cells, spec):
    ok = ((cells[:, 0] >= spec.cell_x0) & (cells[:, 0] < spec.cell_x0 + spec.width) &
          (cells[:, 1] >= spec.cell_y0) & (cells[:, 1] < spec.cell_y0 + spec.height))
    c = cells[ok]
    return c[:, 1] - spec.cell_y0, c[:, 0] - spec.cell_x0


def classify(hits, misses, spec):
    """grid int8 from the planes (step 5)."""
    h, obs = hits.astype(np.int64), hits.astype(np.int64) + misses.astype(np.int64)
    grid = np.full(hits.shape, -1, np.int8)
    known = obs >= spec.min_obs
    occ = known & (1000 * h >= spec.occ_permille * obs)
    free = known & ~occ & (1000 * h <= spec.free_permille * obs)
    grid[occ] = 100
    grid[free] = 0
    return grid


def occupancy(xy, offsets, poses, spec, planes=None):
    """The whole step: (grid int8 (H, W), hits int32, misses int32, stats int64 (8,)).  planes=(hits, misses): what the
    accumulate flag adds onto (not modified)."""
    aff = pose_affines(poses)
    xy = np.asarray(xy, dtype=np.float32).reshape(-1, 2)
    off = np.asarray(offsets, dtype=np.int64)
    shape = (spec.height, spec.width)
    if spec.flags & ACCUMULATE:
        hits, misses = (np.array(p, dtype=np.int32).reshape(shape) for p in planes)
    else:
        hits, misses = np.zeros(shape, np.int32), np.zeros(shape, np.int32)
    stats = np.zeros(8, np.int64)
    for i in range(len(off) - 1):
        if off[i] < 0 or off[i + 1] < off[i]:
            stats[1] += 1
            continue
        sets = scan_sets(xy[off[i]:off[i + 1]], aff[i], spec)
        if sets is None:
            stats[1] += 1
            continue
        H, F, counts = sets
        stats[0] += 1
        stats[2:5] += counts
        hits[in_window(H, spec)] += 1  # (unique cells: no index repeats)
        misses[in_window(F, spec)] += 1
    grid = classify(hits, misses, spec)
    stats[5:8] = ((grid == 100).sum(), (grid == 0).sum(), (grid == -1).sum())
    return grid, hits, misses, stats


# ---------------------------------------------------------------- crafted inputs
def cell_centre(cell, spec):
    """The world point (metres) at the centre of WORLD cell (x, y)."""
    return ((cell[0] + 0.5) * spec.res, (cell[1] + 0.5) * spec.res)


def scan_of_cells(origin, ends, spec):
    """One scan whose sensor sits at the centre of world cell `origin` (heading 0) and whose returns lie at the centres of
    the world cells `ends`: (xy float32 (n, 2) in the sensor's frame, pose (x, y, 0))."""
    ox, oy = cell_centre(origin, spec)
    e = np.asarray(ends, dtype=np.float64).reshape(-1, 2)
    xy = np.stack([(e[:, 0] + 0.5) * spec.res - ox, (e[:, 1] + 0.5) * spec.res - oy], axis=1).astype(np.float32)
    return xy, (ox, oy, 0.0)


def pack(scans):
    """[(xy, pose), ...] -> (xy, offsets int32, poses (n, 3))"""
    xy = np.concatenate([s[0].reshape(-1, 2) for s in scans]).astype(np.float32) if scans else np.zeros((0, 2), np.float32)
    off = np.concatenate([[0], np.cumsum([len(s[0]) for s in scans])]).astype(np.int32)
    return xy, off, np.array([s[1] for s in scans], dtype=np.float64).reshape(-1, 3)
