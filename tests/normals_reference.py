"""numpy restatement of the scan-normal spec ("Scan normals"; include/nautilus_hip.h), written from
the text of the spec: what tests/test_normals_gpu.py holds nhip_normals_estimate_dev to, and what
tests/test_normals_cpu.py measures against the analytic normals of a synthetic world.

estimate() returns the normals, the four info words of every point, and which points are AMBIGUOUS: a point one of whose
votes has angle / step within 1e-9 of a half-integer -- the only points where a device acos that differs from numpy's in
its last bit may move a vote to another bin.
"""
import math

import numpy as np

DEFAULTS = dict(neighborhood_size=0.15, neighborhood_step_size=0.1, mean_distance=0.1, bin_number=32, max_growth_steps=32,
                seed=1)
M32 = np.uint64(0xffffffff)
F32 = np.float32


def lowbias32(x):
    """The mixer on an array of uint64 holding 32-bit values."""
    x = np.asarray(x, dtype=np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & M32
    x ^= x >> np.uint64(16)
    return x


def sample_limit(mean_distance):
    return int(1 / (2.0 * mean_distance * mean_distance))


def neighbours(pts, i, spec):
    """(scan indices of the neighbours of point i in scan order, growth steps made)."""
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy = pts[i, 0] - pts[:, 0], pts[i, 1] - pts[:, 1]  # float32, every operation rounded on its own
        d = np.sqrt(dx * dx + dy * dy)
        r, steps = float(spec["neighborhood_size"]), 0
        nb = np.nonzero(d < F32(r))[0]
        while len(nb) < 2 and steps < spec["max_growth_steps"]:
            r += float(spec["neighborhood_step_size"])
            steps += 1
            nb = np.nonzero(d < F32(r))[0]  # rebuilt
    return nb, steps


def pair_sequence(seed, i, m, count):
    """The first `count` ordered pairs of neighbour ranks point i takes: two draws per attempt, redrawn while a == b or
    the pair was taken."""
    s0 = int(lowbias32(np.uint64(seed) ^ lowbias32(np.uint64(i))))
    out, taken, k = [], set(), 0
    while len(out) < count:
        block = 4 * count + 64
        draws = lowbias32((np.uint64(s0) + np.arange(k, k + block, dtype=np.uint64)) & M32)
        ranks = ((draws * np.uint64(m)) >> np.uint64(32)).astype(np.int64)
        for a, b in zip(ranks[0::2].tolist(), ranks[1::2].tolist()):
            if a == b or (a, b) in taken:
                continue
            taken.add((a, b))
            out.append((a, b))
            if len(out) == count:
                break
        k += block
    return out


def votes_of(pa, pb, bin_number, fold=True):
    """Per pair: (votes: bool, angle, angle / step, bin)."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        dx, dy = pb[:, 0] - pa[:, 0], pb[:, 1] - pa[:, 1]
        ln = np.sqrt(dx * dx + dy * dy)
        ok = (ln > 0) & np.isfinite(ln)
        ln = np.where(ok, ln, F32(1))
        nx, ny = (-dy) / ln, dx / ln
        if fold:
            neg = (ny < 0) | ((ny == 0) & (nx < 0))
            nx, ny = np.where(neg, -nx, nx), np.where(neg, -ny, ny)
        angle = np.arccos(np.clip(nx.astype(np.float64), -1.0, 1.0))
    step = (2.0 * math.pi) / bin_number
    q = angle / step
    return ok, angle, q, np.floor(q + 0.5).astype(np.int64)


def estimate_scan(pts, spec, fold=True):
    pts = np.ascontiguousarray(pts, dtype=F32).reshape(-1, 2)
    n, B = len(pts), int(spec["bin_number"])
    normals, info, amb = np.zeros((n, 2), F32), np.zeros((n, 4), np.int32), np.zeros(n, bool)
    term, bound = sample_limit(spec["mean_distance"]), 2.0 * math.sqrt(1.0 / B)
    for i in range(n):
        nb, steps = neighbours(pts, i, spec)
        m = len(nb)
        info[i] = (m, steps, -1, 0)
        if m < 2:
            continue
        limit = min(m * (m - 1), term)
        pairs = np.asarray(pair_sequence(spec["seed"], i, m, limit), dtype=np.int64).reshape(-1, 2)
        ok, angle, q, bins = votes_of(pts[nb[pairs[:, 0]]], pts[nb[pairs[:, 1]]], B, fold)
        count, total = {}, {}
        most = second = samples = 0
        for k in range(limit):
            if ok[k]:
                b = int(bins[k])
                if abs((q[k] - math.floor(q[k])) - 0.5) < 1e-9:
                    amb[i] = True
                count[b] = count.get(b, 0) + 1
                total[b] = total.get(b, 0.0) + float(angle[k])  # (in vote order)
                if count.get(most, 0) < count[b]:
                    second, most = most, b
                elif count.get(second, 0) < count[b]:
                    second = b
                if float(count.get(most, 0) // B) - float(count.get(second, 0) // B) >= bound:
                    break
            samples += 1
        if not count:
            info[i, 3] = samples << 16
            continue
        a = total[most] / count[most]
        normals[i] = (F32(math.cos(a)), F32(math.sin(a)))
        info[i, 2], info[i, 3] = most, count[most] | (samples << 16)
    return normals, info, amb


def estimate(xy, offsets, spec=None, fold=True):
    """(normals (n, 2) float32, info (n, 4) int32, ambiguous (n,) bool) of the packed scans."""
    spec = dict(DEFAULTS, **(spec or {}))
    xy = np.ascontiguousarray(xy, dtype=F32).reshape(-1, 2)
    parts = [estimate_scan(xy[offsets[s]:offsets[s + 1]], spec, fold) for s in range(len(offsets) - 1)]
    if not parts:
        return np.zeros((0, 2), F32), np.zeros((0, 4), np.int32), np.zeros(0, bool)
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(3))


def share_within(normals, truth, degrees=10.0):
    """Share of the points whose normal lies within `degrees` of the true one, modulo sign; (0, 0) normals count as misses."""
    dot = np.abs(np.sum(normals.astype(np.float64) * truth.astype(np.float64), axis=1))
    return float(np.mean(dot >= math.cos(math.radians(degrees))))


# ---- the inputs of the GPU tests (tests/test_normals_cpu.py shows that none of their points is ambiguous) ----
CRAFTED_LENGTHS = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1088, 1089, 2500)


def wall_scan(n, rng, spacing=0.03, noise=0.004):
    """n points in scan order along four noisy wall segments: axis-parallel, 45 degrees, oblique, axis-parallel the other way."""
    dirs = [(1.0, 0.0), (math.cos(math.pi / 4), math.sin(math.pi / 4)), (math.cos(1.9), math.sin(1.9)), (0.0, -1.0)]
    pts, corner, per = [], np.array([rng.uniform(-3, 3), rng.uniform(-3, 3)]), -(-n // 4)
    for d in dirs:
        k = min(per, n - len(pts))
        t = spacing * np.arange(k)[:, None]
        pts.extend(corner + t * np.array(d) + rng.normal(0, noise, (k, 2)))
        corner = corner + spacing * per * np.array(d)
    return np.asarray(pts, dtype=np.float64).reshape(-1, 2).astype(F32)


def crafted_batch(seed=5):
    """(xy, offsets, marks): the wall scans of CRAFTED_LENGTHS, then the scans that aim at one rule each.  marks: name ->
    global point index of the points a test asserts on by name."""
    rng = np.random.default_rng(seed)
    scans = [wall_scan(n, rng) for n in CRAFTED_LENGTHS]
    marks = {}
    base = lambda: sum(len(s) for s in scans)
    # every pair has zero length: samples, no votes
    marks["coincident"] = base()
    scans.append(np.tile(np.array([[1.5, -2.25]], F32), (12, 1)))
    # isolated points: the nearest other point at 0.2 (one growth: 0.25), 0.3 (two: 0.35), 3.3 (32: 3.35), and out of reach
    wall = np.stack([0.03 * np.arange(40), np.zeros(40)], axis=1)
    iso = np.array([[-0.2, 0.0], [0.6, 0.3], [0.6, -3.3], [60.0, 60.0]])
    marks["grow1"], marks["grow2"], marks["grow32"], marks["never"] = (base() + 40 + k for k in range(4))
    scans.append(np.concatenate([wall, iso]).astype(F32))
    # a NaN and an inf point among good ones
    s = wall_scan(30, rng)
    s[7], s[19] = (np.nan, 1.0), (np.inf, 0.5)
    marks["nan"], marks["inf"] = base() + 7, base() + 19
    scans.append(s)
    # a pair at exactly float(0.15): no neighbours until the radius grows; a pair one ulp closer: neighbours at once
    edge = F32(0.15)
    marks["at_radius"], marks["ulp_inside"] = base(), base() + 2
    scans.append(np.array([[0.0, 0.0], [edge, 0.0], [0.0, 5.0], [np.nextafter(edge, F32(0)), 5.0]], F32))
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int32)
    return np.concatenate(scans).astype(F32), offsets, marks


# the specs the GPU tests compare with this file at: the defaults (the LDS form for scans of up to 1088 points), and a sample
# list longer than the LDS form holds (102 samples: every scan takes the general form) with a bin count that is no power of two
PARITY_SPECS = {"default": {}, "long_list": dict(mean_distance=0.07, bin_number=24, seed=77)}
_EXPECTED = {}


def crafted_expected(name):
    """(normals, info, ambiguous) of crafted_batch() under PARITY_SPECS[name]; computed once per process and shared."""
    if name not in _EXPECTED:
        xy, off, _ = crafted_batch()
        _EXPECTED[name] = estimate(xy, off, PARITY_SPECS[name])
        for a in _EXPECTED[name]:
            a.setflags(write=False)
    return _EXPECTED[name]
