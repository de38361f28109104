"""Numpy statement of the scan-feature spec ("Scan features"; the reference:
src/input/feature_extracter.cc:15-165).  Test infrastructure: written from the spec as a plain sorted walk, not as the
kernel's rounds of argmin.  float32 numpy operations round one by one, like the reference's baseline-x86 floats."""
import numpy as np

F32 = np.float32


class Spec:
    def __init__(self, threshold=0.008, distance_threshold=2.0, max_neighbor_distance=0.8, neighbors_per_side=10,
                 min_neighbors=10, max_planar=20, max_edge=10):
        self.threshold, self.distance_threshold, self.max_neighbor_distance = threshold, distance_threshold, max_neighbor_distance
        self.neighbors_per_side, self.min_neighbors, self.max_planar, self.max_edge = neighbors_per_side, min_neighbors, max_planar, max_edge

    def fields(self):
        return dict(self.__dict__)


def _norm(a, b):
    """(a - b).norm() of Vector2f, widened to double."""
    dx, dy = (a[..., 0] - b[..., 0]).astype(F32), (a[..., 1] - b[..., 1]).astype(F32)
    return np.sqrt((dx * dx + dy * dy).astype(F32)).astype(np.float64)


def neighbourhood(pts, i, spec):
    """Indices of point i's neighbourhood in the reference's order (left kept, right, the point), or None (too few)."""
    n, P = len(pts), spec.neighbors_per_side
    out = []
    if i >= P:  # (size_t i - P wraps for i < P and the loop never runs)
        for k in range(i - P, i):
            if _norm(pts[i], pts[k]) <= spec.max_neighbor_distance:
                out.append(k)
    out.extend(range(i + 1, min(n, i + P)))
    if len(out) < spec.min_neighbors:
        return None
    return out + [i]


def _eig_ratio(a, b, c, d):
    A, B, Cc, D = (v.astype(np.float64) for v in (a, b, c, d))
    half_tr, half_df = 0.5 * (A + D), 0.5 * (A - D)
    disc = half_df * half_df + B * Cc
    root = np.sqrt(np.where(disc < 0.0, 0.0, disc))
    e1, e2 = half_tr + root, half_tr - root
    lo, hi = np.where(e1 < e2, e1, e2), np.where(e1 < e2, e2, e1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return lo / hi


def scores(pts, spec):
    """The smoothness score of every point of one scan (float64, NaN = no score); all points at once, one neighbour
    position per step, so every float sum runs in the neighbourhood's order."""
    pts = np.ascontiguousarray(pts, dtype=F32).reshape(-1, 2)
    n, P = len(pts), spec.neighbors_per_side
    if n == 0:
        return np.zeros(0)
    idx = np.arange(n)
    steps = []  # (index of the neighbour, whether it belongs to the neighbourhood) per position
    for k in range(P):
        j = idx - P + k
        q = pts[np.clip(j, 0, n - 1)]
        steps.append((q, (idx >= P) & (_norm(pts, q) <= spec.max_neighbor_distance)))
    for k in range(1, P):
        j = idx + k
        steps.append((pts[np.clip(j, 0, n - 1)], j < n))
    cnt = sum(m.astype(np.int64) for _, m in steps)
    steps.append((pts, np.ones(n, bool)))
    sx, sy = np.zeros(n, F32), np.zeros(n, F32)
    for q, m in steps:
        sx, sy = np.where(m, (sx + q[:, 0]).astype(F32), sx), np.where(m, (sy + q[:, 1]).astype(F32), sy)
    inv = (1.0 / (cnt + 1).astype(np.float64)).astype(F32)
    mx, my = (inv * sx).astype(F32), (inv * sy).astype(F32)
    a, b, c, d = (np.zeros(n, F32) for _ in range(4))
    for q, m in steps:
        dx, dy = (q[:, 0] - mx).astype(F32), (q[:, 1] - my).astype(F32)
        a = np.where(m, (a + (dx * dx).astype(F32)).astype(F32), a)
        b = np.where(m, (b + (dx * dy).astype(F32)).astype(F32), b)
        c = np.where(m, (c + (dy * dx).astype(F32)).astype(F32), c)
        d = np.where(m, (d + (dy * dy).astype(F32)).astype(F32), d)
    out = _eig_ratio(a, b, c, d)
    out[cnt < spec.min_neighbors] = np.nan
    return out


def _walk(pts, order, sc, spec, edge):
    cap = spec.max_edge if edge else spec.max_planar
    acc = []
    for i in order:
        if (sc[i] < spec.threshold) if edge else (sc[i] > spec.threshold):
            continue
        if len(acc) >= cap:
            continue
        if acc and (_norm(pts[acc], pts[i][None, :]) < spec.distance_threshold).any():
            continue
        acc.append(i)
    return acc


def extract_scan(pts, spec):
    """(planar indices, edge indices, scores) of one scan; the indices in acceptance order."""
    pts = np.ascontiguousarray(pts, dtype=F32).reshape(-1, 2)
    sc = scores(pts, spec)
    order = sorted((i for i in range(len(pts)) if not np.isnan(sc[i])), key=lambda i: (float(sc[i]), i))
    return _walk(pts, order, sc, spec, False), _walk(pts, order[::-1], sc, spec, True), sc


def extract(xy, offsets, spec):
    """Every scan: (planar_idx (n, max_planar) -1 padded, planar_count, edge_idx, edge_count, scores (n_points,))."""
    xy = np.ascontiguousarray(xy, dtype=F32).reshape(-1, 2)
    n = len(offsets) - 1
    pidx, eidx = -np.ones((n, spec.max_planar), np.int32), -np.ones((n, spec.max_edge), np.int32)
    pcnt, ecnt = np.zeros(n, np.int32), np.zeros(n, np.int32)
    sc = np.zeros(len(xy))
    for s in range(n):
        p, e, sc[offsets[s]:offsets[s + 1]] = extract_scan(xy[offsets[s]:offsets[s + 1]], spec)
        pidx[s, :len(p)], pcnt[s] = p, len(p)
        eidx[s, :len(e)], ecnt[s] = e, len(e)
    return pidx, pcnt, eidx, ecnt, sc


def clouds(xy, normals, offsets, idx, count):
    """The packed cloud of one set: xy[off[s] + idx] / normals[...] in acceptance order, offsets = cumulative counts."""
    xy = np.ascontiguousarray(xy, dtype=F32).reshape(-1, 2)
    sel = np.concatenate([offsets[s] + idx[s, :count[s]] for s in range(len(count))] + [np.zeros(0, np.int64)]).astype(np.int64)
    off = np.zeros(len(count) + 1, np.int32)
    off[1:] = np.cumsum(count)
    nrm = None if normals is None else np.ascontiguousarray(normals, dtype=F32).reshape(-1, 2)[sel]
    return xy[sel], nrm, off


def feature_clouds(xy, normals, offsets, spec):
    """((xy_p, nrm_p, off_p), (xy_e, nrm_e, off_e)) from this reference: what HipBackend.features() returns."""
    pidx, pcnt, eidx, ecnt, _ = extract(xy, offsets, spec)
    return clouds(xy, normals, offsets, pidx, pcnt), clouds(xy, normals, offsets, eidx, ecnt)


# ---- designed inputs (shared by the CPU and the GPU tests) ----
def line(n, spacing, angle_deg=0.0):
    t = (np.arange(n, dtype=np.float64) * spacing)
    a = np.radians(angle_deg)
    return np.stack([t * np.cos(a), t * np.sin(a)], axis=1).astype(F32)


def wall_with_jump(n=120, spacing=0.05, jump=5.0):
    """A wall seen in beam order whose second half lies `jump` metres behind the first: the points before the jump have
    right neighbours 5 m away, which are not distance-tested."""
    p = line(n, spacing).astype(np.float64)
    p[n // 2:, 1] += jump
    return p.astype(F32)
