"""The numpy statement of the transient-returns filter ("Transient returns"; the device form is K19,
nautilus_amd/csrc/nhip_transient.hip), and the cases its CPU and GPU tests share.  Written from the spec's text and
differently from the kernel and from hostside.transient_filter on purpose: the hit support is summed from (2 r + 1)^2 shifted
reads of a zero-padded copy of the plane (no clipped loops, no summed-area table), the kept points are taken with a boolean
mask, and no code is shared with the product.  It builds on tests/occupancy_reference.py (the cells, the crafted scans) and
tests/vectorize_reference.py (the affines) and runs on no device.

A spec is anything with the fields of nhip_transient_spec_t as attributes (a ctypes struct, or make_spec() below).
"""
from types import SimpleNamespace

import numpy as np

from tests import occupancy_reference as OR
from tests.vectorize_reference import pose_affines

FIELDS = ("res", "cell_x0", "cell_y0", "width", "height", "support_radius", "min_through", "transient_permille", "flags", "reserved")
STATIC, TRANSIENT, UNOBSERVED, INVALID = 0, 1, 2, 3
NAMES = ("out_xy", "out_offsets", "out_index", "labels", "stats")


def make_spec(**kw):
    s = SimpleNamespace(res=0.05, cell_x0=0, cell_y0=0, width=1, height=1, support_radius=1, min_through=2, transient_permille=500,
                        flags=0, reserved=0)
    for k, v in kw.items():
        assert k in FIELDS, k
        setattr(s, k, v)
    return s


def spec_from(occ_spec, **kw):
    return make_spec(**dict(dict(res=occ_spec.res, cell_x0=occ_spec.cell_x0, cell_y0=occ_spec.cell_y0, width=occ_spec.width,
                                 height=occ_spec.height), **kw))


def scan_labels(points, affine, spec, hits_padded, misses):
    """uint8 (n,): the label of every point of one scan (items 1-5).  hits_padded: int64, r zero cells on every side."""
    f = np.float32
    r = spec.support_radius
    c, s, tx, ty = (f(v) for v in affine)
    p = np.asarray(points, dtype=f).reshape(-1, 2)
    with np.errstate(invalid="ignore", over="ignore"):
        x = ((c * p[:, 0]).astype(f) + ((-s) * p[:, 1]).astype(f)).astype(f) + tx
        y = ((s * p[:, 0]).astype(f) + (c * p[:, 1]).astype(f)).astype(f) + ty
        w = np.stack([x.astype(f), y.astype(f)], axis=1).astype(np.float64)
        fl = np.floor(w / spec.res)
        ok = np.isfinite(p).all(axis=1) & np.isfinite(w).all(axis=1) & (np.abs(fl) < OR.LIMIT).all(axis=1)
    labels = np.full(len(p), INVALID, np.uint8)
    for i in np.nonzero(ok)[0]:
        cx, cy = int(fl[i, 0]) - spec.cell_x0, int(fl[i, 1]) - spec.cell_y0  # (python ints: the true values)
        if not (0 <= cx < spec.width and 0 <= cy < spec.height):
            labels[i] = UNOBSERVED
            continue
        S = int(hits_padded[cy:cy + 2 * r + 1, cx:cx + 2 * r + 1].sum())  # (padded: rows cy - r .. cy + r of the plane)
        m = int(misses[cy, cx])
        labels[i] = TRANSIENT if (m >= spec.min_through and 1000 * S <= spec.transient_permille * (S + m)) else STATIC
    return labels


def transient_filter(xy, offsets, poses, spec, hits, misses, n_points=None):
    """The whole step: (out_xy float32 (kept, 2), out_offsets int32 (n_scans + 1,), out_index int32 (kept,), labels uint8
    (n_points,), stats int64 (8,)).  The planes are not modified."""
    aff = pose_affines(poses)
    xy = np.asarray(xy, dtype=np.float32).reshape(-1, 2)
    n_points = len(xy) if n_points is None else n_points
    off = np.asarray(offsets, dtype=np.int64)
    r = spec.support_radius
    H = np.asarray(hits, dtype=np.int64).reshape(spec.height, spec.width)
    M = np.asarray(misses, dtype=np.int64).reshape(spec.height, spec.width)
    Hp = np.zeros((spec.height + 2 * r, spec.width + 2 * r), np.int64)
    Hp[r:r + spec.height, r:r + spec.width] = H
    labels = np.full(n_points, INVALID, np.uint8)
    owner = np.full(n_points, -1, np.int64)  # the scan of every point that belongs to one
    stats = np.zeros(8, np.int64)
    counts = []
    for i in range(len(off) - 1):
        stats[4] += 1
        if off[i] < 0 or off[i + 1] < off[i] or off[i + 1] > n_points:
            stats[5] += 1
            counts.append(0)
            continue
        lab = scan_labels(xy[off[i]:off[i + 1]], aff[i], spec, Hp, M)
        labels[off[i]:off[i + 1]] = lab
        owner[off[i]:off[i + 1]] = i
        for k in range(4):
            stats[k] += int((lab == k).sum())
        kept = int(((lab == STATIC) | (lab == UNOBSERVED)).sum())
        stats[6] += int(len(lab) > 0 and kept == 0)
        counts.append(kept)
    # scans in order and points in order inside each: for scans that do not overlap (every case here) that is cloud order
    keep = (owner >= 0) & ((labels == STATIC) | (labels == UNOBSERVED))
    order = np.argsort(owner[keep], kind="stable")
    out_index = np.nonzero(keep)[0][order].astype(np.int32)
    out_offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return xy[out_index], out_offsets, out_index, labels, stats


def static_scans(xy, offsets, poses, occ_spec, **kw):
    """The composition: occupancy trace, then the filter on its planes: (the filter's five, occupancy stats, hits, misses)."""
    grid, hits, misses, occ_stats = OR.occupancy(xy, offsets, poses, occ_spec)
    return transient_filter(xy, offsets, poses, spec_from(occ_spec, **kw), hits, misses) + (occ_stats, hits, misses)


def same(got, want, what=""):
    for g, w, name in zip(got, want, NAMES):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (name, what)


def packing_properties(xy, offsets, out, what=""):
    """What every result satisfies whatever the planes: indices strictly increasing inside a scan and inside the scan's range,
    out_xy the bit copies of xy[out_index], offsets consistent with the labels."""
    out_xy, out_off, out_idx, labels, stats = out
    xy = np.asarray(xy, dtype=np.float32).reshape(-1, 2)
    off = np.asarray(offsets, dtype=np.int64)
    assert out_off[0] == 0 and out_off[-1] == len(out_idx) == len(out_xy), what
    assert out_xy.tobytes() == xy[out_idx].tobytes(), what
    for i in range(len(off) - 1):
        idx = out_idx[out_off[i]:out_off[i + 1]].astype(np.int64)
        if off[i] < 0 or off[i + 1] < off[i] or off[i + 1] > len(labels):
            assert len(idx) == 0, (what, i)
            continue
        lab = labels[off[i]:off[i + 1]]
        assert (np.diff(idx) > 0).all(), (what, i)
        assert np.array_equal(idx - off[i], np.nonzero((lab == STATIC) | (lab == UNOBSERVED))[0]), (what, i)
    assert stats[0] + stats[2] == len(out_idx) and stats[7] == 0, what


# ---------------------------------------------------------------- crafted inputs
def points_of_cells(cells, spec):
    """float32 (n, 2): the centres of the WORLD cells `cells`, for a scan at pose (0, 0, 0)"""
    e = np.asarray(cells, dtype=np.float64).reshape(-1, 2)
    return ((e + 0.5) * spec.res).astype(np.float32)


def pack(scans):
    return OR.pack(scans)


ZERO_POSE = (0.0, 0.0, 0.0)


def planes_from_rule(spec, rule):
    """hits and misses int32 (H, W) filled by rule(x, y) -> (h, m) of WINDOW cell (x, y)"""
    hits, misses = np.zeros((spec.height, spec.width), np.int32), np.zeros((spec.height, spec.width), np.int32)
    for y in range(spec.height):
        for x in range(spec.width):
            hits[y, x], misses[y, x] = rule(x, y)
    return hits, misses


def case_seams():
    """scans of 0, 1, 63, 64, 65, 255, 256, 257 points in one call -- the wave and workgroup seams of the ballot compaction --
    on a 64 x 64 window whose planes make every third cell column transient (radius 0)"""
    spec = make_spec(width=64, height=64, support_radius=0)
    hits, misses = planes_from_rule(spec, lambda x, y: (0, 5) if x % 3 == 0 else (4, 1))
    rng = np.random.default_rng(5)
    scans = []
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 0, 130):
        cells = np.stack([rng.integers(0, 64, n), rng.integers(0, 64, n)], axis=1)
        scans.append((points_of_cells(cells, spec), ZERO_POSE))
    return ("seams",) + pack(scans) + (spec, hits, misses)


def case_keep_patterns():
    """a scan that keeps everything, one that keeps nothing, one that keeps only its first point, one only its last, and
    kept / dropped lanes alternating across wave and workgroup boundaries (300 points); column 0 of the window is transient"""
    spec = make_spec(width=8, height=4, support_radius=0)
    hits, misses = planes_from_rule(spec, lambda x, y: (0, 3) if x == 0 else (2, 0))
    T, K = (0, 1), (5, 2)  # a transient cell, a static one
    scans = [[K] * 70, [T] * 70, [K] + [T] * 199, [T] * 199 + [K], [T if i % 2 else K for i in range(300)],
             [K if i % 2 else T for i in range(129)], [T] * 64 + [K] * 64 + [T] * 64]
    return ("keep patterns",) + pack([(points_of_cells(c, spec), ZERO_POSE) for c in scans]) + (spec, hits, misses)


def case_window_edges(radius, width=7, height=5, x0=-3, y0=2):
    """every cell of the window and the ring of cells one outside it (label 2), planes with distinct hits everywhere: the
    corner and edge cells clip the neighbourhood; world cells are negative on x (floor is not truncation)"""
    spec = make_spec(width=width, height=height, cell_x0=x0, cell_y0=y0, support_radius=radius, min_through=1)
    hits, misses = planes_from_rule(spec, lambda x, y: (int((x * 7 + y * 3) % 5 == 0) * (1 + x % 3), 1 + (x * 3 + y) % 9))
    cells = [(x, y) for y in range(y0 - 1, y0 + height + 1) for x in range(x0 - 1, x0 + width + 1)]
    # points near the low edge of their cell too: floor(-0.02 / 0.05) = -1, not 0
    low = (np.asarray(cells, dtype=np.float64) + 0.1) * spec.res
    xy = np.concatenate([points_of_cells(cells, spec), low.astype(np.float32)])
    return ("window edges r=%d %dx%d" % (radius, width, height), xy, np.array([0, len(cells), len(xy)], np.int32),
            np.array([ZERO_POSE, ZERO_POSE]), spec, hits, misses)


def case_thresholds():
    """both threshold edges on hand-written planes, radius 0, min_through 3, permille 250: m = 2 and m = 3; 1000 S exactly
    equal to 250 (S + m) (S = 1, m = 3: transient) and one above (S = 2, m = 3 -> 2000 > 1250; S = 1, m = 2 fails on m);
    larger equalities 25 / 75 and 26 / 74"""
    spec = make_spec(width=8, height=1, support_radius=0, min_through=3, transient_permille=250)
    hits = np.array([[0, 0, 1, 2, 1, 25, 26, 25]], np.int32)
    misses = np.array([[2, 3, 3, 3, 2, 75, 74, 76]], np.int32)
    want = [0, 1, 1, 0, 0, 1, 0, 1]
    xy = points_of_cells([(x, 0) for x in range(8)], spec)
    return ("thresholds", xy, np.array([0, 8], np.int32), np.array([ZERO_POSE]), spec, hits, misses), want


def case_thresholds_one_above():
    """permille 333: S = 1, m = 2 gives 1000 S = 333 (S + m) + 1, ONE above (static); S = 333, m = 667 is equality
    (transient); S = 334, m = 666 is above; permille 334 turns the first one transient"""
    out = []
    for permille, want in ((333, [0, 1, 0]), (334, [1, 1, 1])):
        spec = make_spec(width=3, height=1, support_radius=0, min_through=2, transient_permille=permille)
        hits, misses = np.array([[1, 333, 334]], np.int32), np.array([[2, 667, 666]], np.int32)
        xy = points_of_cells([(x, 0) for x in range(3)], spec)
        out.append((("thresholds permille %d" % permille, xy, np.array([0, 3], np.int32), np.array([ZERO_POSE]), spec, hits, misses), want))
    return out


def case_permille(permille):
    """transient_permille 0 (only S = 0 is transient) and 1000 (everything seen through often enough is)"""
    spec = make_spec(width=6, height=1, support_radius=0, min_through=1, transient_permille=permille)
    hits = np.array([[0, 1, 0, 5, 7, 0]], np.int32)
    misses = np.array([[1, 1, 0, 0, 9, 100]], np.int32)
    xy = points_of_cells([(x, 0) for x in range(6)], spec)
    return ("permille %d" % permille, xy, np.array([0, 6], np.int32), np.array([ZERO_POSE]), spec, hits, misses)


def case_large_counts():
    """planes holding 2^30 and INT32_MAX: 1000 S and permille (S + m) need int64 (S of nine cells of INT32_MAX is 1.9e10);
    with 32-bit products the labels of these cells come out differently"""
    big, top = 1 << 30, 2 ** 31 - 1
    spec = make_spec(width=5, height=3, support_radius=1, min_through=1 << 30, transient_permille=500)
    hits = np.full((3, 5), top, np.int32)
    misses = np.full((3, 5), top, np.int32)
    hits[1, 0], misses[1, 0] = 0, big          # m = min_through
    misses[1, 1] = big - 1                     # m = min_through - 1
    hits[:, 3:], misses[1, 4] = 0, top         # S = 0 around (4, 1)
    hits[0, 3] = big
    xy = points_of_cells([(x, y) for y in range(3) for x in range(5)], spec)
    cases = [("large counts", xy, np.array([0, 15], np.int32), np.array([ZERO_POSE]), spec, hits, misses)]
    s0 = make_spec(width=5, height=3, support_radius=0, min_through=1, transient_permille=500)
    h0 = np.array([[top, top, big, big, 1]] * 3, np.int32)
    m0 = np.array([[top, top - 1, big, big + 1, top]] * 3, np.int32)  # 1000 S == 500 (S + m) exactly at S == m
    cases.append(("large counts r=0", xy, np.array([0, 15], np.int32), np.array([ZERO_POSE]), s0, h0, m0))
    return cases


def case_invalid():
    """NaN and +-inf points, a non-finite affine (every point of that scan invalid), a world coordinate beyond 2^62 res, and
    good points between them"""
    spec = make_spec(width=16, height=8, cell_x0=-8, cell_y0=-4, support_radius=1, min_through=1)
    hits, misses = planes_from_rule(spec, lambda x, y: (0, 2) if (x + y) % 2 else (3, 0))
    good = points_of_cells([(-8, -4), (7, 3), (0, 0), (-1, -1), (3, -2)], spec)
    dirty = np.concatenate([good[:2], [[np.nan, 0.0], [np.inf, 1.0], [0.0, -np.inf], [3.0e17, 0.0], [0.0, -3.0e38], [1e30, 1e30]],
                            good[2:]]).astype(np.float32)
    scans = [(good, ZERO_POSE), (dirty, ZERO_POSE), (good, (np.nan, 0.0, 0.0)), (good, (0.1, 0.1, np.nan)), (good, (np.inf, 0.0, 0.0)),
             (good, (0.0, 4.0e17, 0.0)), (good, (0.05, -0.05, 0.5))]
    return ("invalid",) + pack(scans) + (spec, hits, misses)


def case_negative_cells():
    """a window wholly on negative cells, points a hair either side of cell boundaries, a rotated pose"""
    spec = make_spec(width=40, height=30, cell_x0=-45, cell_y0=-35, support_radius=2, min_through=2)
    rng = np.random.default_rng(9)
    hits = (rng.integers(1, 4, (30, 40)) * (rng.random((30, 40)) < 0.06)).astype(np.int32)
    misses = rng.integers(0, 6, (30, 40)).astype(np.int32)
    k = rng.integers(-46, -4, (150, 2)).astype(np.float64)
    on = (k * 0.05).astype(np.float32)
    edge = np.concatenate([on, np.nextafter(on, np.float32(-np.inf)), np.nextafter(on, np.float32(np.inf))]).astype(np.float32)
    scans = [(edge, ZERO_POSE), (edge[:200], (-0.31, -0.22, 0.7)), (edge[100:333], (-1.0, -0.8, -2.9))]
    return ("negative cells",) + pack(scans) + (spec, hits, misses)


def case_traced():
    """planes that come from the occupancy trace of the same scans: a square room seen from six poses, and a post that stands
    in the first scan only (its cells are seen through by the five others)"""
    occ = OR.make_spec(width=64, height=64, cell_x0=-32, cell_y0=-32, max_ray_cells=64)
    wall = [(x, -25) for x in range(-25, 26)] + [(x, 25) for x in range(-25, 26)] + [(-25, y) for y in range(-24, 25)] + \
           [(25, y) for y in range(-24, 25)]
    scans = []
    for i, o in enumerate([(0, 0), (3, 1), (-2, 4), (5, -3), (-4, -4), (1, 6)]):
        ends = list(wall)
        if i == 0:
            ends += [(10, 9), (10, 10), (11, 10), (9, 10)]
        scans.append(OR.scan_of_cells(o, ends, occ))
    return ("traced",) + pack(scans) + (occ,)


def case_many_scans(n=4200):
    """more scans than the classify and pack kernels have workgroups (4,096: the rest come round again) and than one step of
    the offsets kernel takes (1,024): scans of 0 .. 5 points on a 16 x 16 window"""
    spec = make_spec(width=16, height=16, support_radius=1, min_through=1)
    rng = np.random.default_rng(21)
    hits = (rng.integers(1, 3, (16, 16)) * (rng.random((16, 16)) < 0.15)).astype(np.int32)
    misses = rng.integers(0, 4, (16, 16)).astype(np.int32)
    lens = np.array([(i * 7) % 6 for i in range(n)])
    cells = np.stack([rng.integers(-1, 17, lens.sum()), rng.integers(-1, 17, lens.sum())], axis=1)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    return ("many scans", points_of_cells(cells, spec), off, np.zeros((n, 3)), spec, hits, misses)


def shared_cases():
    """[(name, xy, offsets, poses, spec, hits, misses)]: what the CPU and the GPU tests both run"""
    cases = [case_seams(), case_keep_patterns(), case_thresholds()[0]] + [c for c, _ in case_thresholds_one_above()]
    cases += [case_permille(0), case_permille(1000), case_invalid(),
             case_negative_cells(), case_many_scans()] + case_large_counts()
    cases += [case_window_edges(r) for r in (0, 1, 2, 4)]
    cases += [case_window_edges(r, width=3, height=3, x0=-1, y0=-1) for r in (0, 1, 4)]  # a window smaller than the neighbourhood
    name, xy, off, poses, occ = case_traced()
    grid, hits, misses, stats = OR.occupancy(xy, off, poses, occ)
    cases.append((name, xy, off, poses, spec_from(occ), hits, misses))
    cases.append(("no scans", np.zeros((0, 2), np.float32), np.array([0], np.int32), np.zeros((0, 3)), make_spec(width=5, height=4),
                  np.ones((4, 5), np.int32), np.ones((4, 5), np.int32)))
    return cases


def bad_offset_cases():
    """the three kinds of bad offsets, each alone and all in one call, between good scans that do not overlap; 64 points.
    [(name, xy, offsets, poses, spec, hits, misses, the bad scans, (value, index) of the first one's record)]"""
    spec = make_spec(width=8, height=4, support_radius=0)
    hits, misses = planes_from_rule(spec, lambda x, y: (0, 3) if x % 2 == 0 else (2, 0))
    cells = [(x, y) for y in range(4) for x in range(8)]
    xy = points_of_cells(cells + cells, spec)
    lists = [("end before start", [20, 30, 4, 12], [1], (4, 2)),          # [20, 30) good, [30, 4) bad, [4, 12) good
             ("negative start", [-2, 12, 30], [0], (-2, 0)),               # [-2, 12) bad, [12, 30) good
             ("end beyond n_points", [0, 10, 70], [1], (70, 2)),           # [0, 10) good, [10, 70) bad
             # [20, 30) good, [30, 4) bad, [4, 12) good, [12, -2) bad, [-2, 40) bad, [40, 70) bad, [70, 50) bad, [50, 64) good
             ("all three", [20, 30, 4, 12, -2, 40, 70, 50, 64], [1, 3, 4, 5, 6], (4, 2))]
    return [(name, xy, np.array(off, np.int32), np.zeros((len(off) - 1, 3)), spec, hits, misses, bad, first)
            for name, off, bad, first in lists]
