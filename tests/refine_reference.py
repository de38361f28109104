"""The slow, obviously-right statement of the match refinement ("Match refinement"; the device form is K22,
nautilus_amd/csrc/nhip_refine.hip; the vectorised host form is hostside.refine_icp), and the case list the CPU and the GPU
tests share.

Every source point is transformed on its own in numpy float32 scalars, finds its nearest target by brute force over all target
points in float32 (ties to the lowest index), and adds its terms to the sums of lane i mod 256 in Python floats (IEEE double,
one rounding per operation); the 256 lane sums are halved pair by pair, eight levels.  The three `perturb` switches state a
WRONG rule each -- a threshold one table slot off, ties to the highest index, the lane sums added one after the other -- so
that a test can show the cases tell them apart.
"""
import functools
import math

import numpy as np

from nautilus_amd.hostside import REFINED_DTYPE, RefineFields

F = np.float32
SKIPPED, TARGET_TOO_LONG, FEW, SINGULAR, RUNAWAY, NOT_CONVERGED = 1, 2, 4, 8, 16, 32
TARGET_MAX, SLOTS = 2048, 16


def _nearest(qx, qy, tgt, tgt_ok, ties):
    """Per query the index of the nearest valid target and its float32 squared distance (index -1: none)."""
    ns, nt = len(qx), len(tgt)
    idx, best = np.full(ns, -1, np.int64), np.full(ns, np.inf, F)
    if nt == 0:
        return idx, best
    with np.errstate(all="ignore"):
        for a in range(0, ns, 512):
            dx = tgt[None, :, 0] - qx[a:a + 512, None]
            dy = tgt[None, :, 1] - qy[a:a + 512, None]
            d2 = dx * dx + dy * dy
            d2[:, ~tgt_ok] = np.inf
            d2[np.isnan(d2)] = np.inf
            j = np.argmin(d2, axis=1) if ties == "lowest" else nt - 1 - np.argmin(d2[:, ::-1], axis=1)
            b = d2[np.arange(len(j)), j]
            hit = b < F(3.0e38)
            idx[a:a + 512] = np.where(hit, j, -1)
            best[a:a + 512] = b
    return idx, best


def evaluate(src, tgt, tgn, pose, thr, ties="lowest", butterfly=True):
    """One evaluation at pose = (c, s, tx, ty) (Python floats) under the float32 threshold thr: ([H00 H01 H02 H11 H12 H22 g0 g1
    g2 cost], count)."""
    c, s, tx, ty = pose
    cf, sf, txf, tyf = F(c), F(s), F(tx), F(ty)
    ns = len(src)
    limit = F(1.0e6)
    with np.errstate(all="ignore"):
        src_ok = (np.abs(src[:, 0]) < limit) & (np.abs(src[:, 1]) < limit) if ns else np.zeros(0, bool)
        tgt_ok = (np.abs(tgt[:, 0]) < limit) & (np.abs(tgt[:, 1]) < limit) if len(tgt) else np.zeros(0, bool)
        qx, qy = np.zeros(ns, F), np.zeros(ns, F)
        for i in range(ns):
            px, py = src[i, 0], src[i, 1]
            qx[i] = F(F(F(cf * px) + F(F(-sf) * py)) + txf)
            qy[i] = F(F(F(sf * px) + F(cf * py)) + tyf)
        idx, best = _nearest(qx, qy, tgt, tgt_ok, ties)
        root = np.sqrt(best)  # float32, correctly rounded
    lanes = [[0.0] * 10 for _ in range(256)]
    count = 0
    for i in range(ns):
        j = int(idx[i])
        if not src_ok[i] or j < 0 or not (root[i] < thr):
            continue
        nx, ny = float(tgn[j, 0]), float(tgn[j, 1])
        if not (math.isfinite(nx) and math.isfinite(ny)):
            continue
        dpx, dpy = float(src[i, 0]), float(src[i, 1])
        ex, ey = float(qx[i]) - float(tgt[j, 0]), float(qy[i]) - float(tgt[j, 1])
        r = nx * ex + ny * ey
        a, b = -(s * dpx) - c * dpy, c * dpx - s * dpy
        jt = nx * a + ny * b
        acc = lanes[i % 256]
        for k, term in enumerate((nx * nx, nx * ny, nx * jt, ny * ny, ny * jt, jt * jt, nx * r, ny * r, jt * r, r * r)):
            acc[k] = acc[k] + term
        count += 1
    if butterfly:
        while len(lanes) > 1:
            lanes = [[u + v for u, v in zip(lanes[2 * m], lanes[2 * m + 1])] for m in range(len(lanes) // 2)]
        return lanes[0], count
    total = [0.0] * 10
    for lane in lanes:
        total = [u + v for u, v in zip(total, lane)]
    return total, count


def _div(a, b):
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0.0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)


def solve(v, count, min_spread):
    """(dx, dy, dtheta) from the sums, or None for SINGULAR: spread test, then the square-root-free Cholesky, written out."""
    H00, H01, H02, H11, H12, H22, g0, g1, g2 = v[:9]
    hm, hd = (H00 + H11) * 0.5, (H00 - H11) * 0.5
    q = hd * hd + H01 * H01
    lam = hm - (math.sqrt(q) if q == q and q != math.inf else q)
    d0 = H00
    l10, l20 = _div(H01, d0), _div(H02, d0)
    d1 = H11 - l10 * H01
    u = H12 - l20 * H01
    l21 = _div(u, d1)
    d2 = (H22 - l20 * H02) - l21 * u
    if not (lam / float(count) >= min_spread) or not (d0 > 0.0) or not (d1 > 0.0) or not (d2 > 0.0):
        return None
    y0 = -g0
    y1 = -g1 - l10 * y0
    y2 = (-g2 - l20 * y0) - l21 * y1
    dth = y2 / d2
    dy = y1 / d1 - l21 * dth
    dx = (y0 / d0 - l10 * dy) - l20 * dth
    return dx, dy, dth


def refine_pair(src, tgt, tgn, pose0, spec, thr_shift=0, ties="lowest", butterfly=True):
    """One pair: (record fields as a dict, trace (16, 4))."""
    thr = np.asarray(list(spec.thr), dtype=F)
    max_it, min_corr = int(spec.max_iterations), int(spec.min_corr)
    c0, s0, tx0, ty0 = (float(x) for x in pose0)
    rec = dict(c=c0, s=s0, tx=tx0, ty=ty0, info=[0.0] * 6, cost=0.0, n_corr=0, iterations=0, flags=0)
    trace = np.zeros((SLOTS, 4))
    if not all(math.isfinite(x) for x in (c0, s0, tx0, ty0)):
        rec.update(c=math.nan, s=math.nan, tx=math.nan, ty=math.nan, flags=SKIPPED)
        return rec, trace
    if len(tgt) > TARGET_MAX:
        rec["flags"] = TARGET_TOO_LONG
        return rec, trace
    ev = lambda pose, k: evaluate(src, tgt, tgn, pose, thr[min(k + thr_shift, SLOTS - 1)], ties, butterfly)
    c, s, tx, ty = c0, s0, tx0, ty0
    it, flags, converged = 0, 0, False
    while it < max_it:
        v, n = ev((c, s, tx, ty), it)
        if n < min_corr:
            flags = FEW
            break
        d = solve(v, n, float(spec.min_spread))
        if d is None:
            flags = SINGULAR
            break
        dx, dy, dth = d
        tx, ty = tx + dx, ty + dy
        hu = dth * 0.5
        u2 = hu * hu
        den = 1.0 + u2
        cd, sd = (1.0 - u2) / den, (2.0 * hu) / den
        c, s = c * cd - s * sd, s * cd + c * sd
        mx, my = tx - tx0, ty - ty0
        if not (math.sqrt(mx * mx + my * my) <= float(spec.max_shift_m)) or not (abs(s * c0 - c * s0) <= float(spec.max_turn_sin)):
            flags = RUNAWAY
            break
        trace[it] = (c, s, tx, ty)
        it += 1
        if math.sqrt(dx * dx + dy * dy) < float(spec.step_tol_m) and abs(dth) < float(spec.step_tol_rad):
            converged = True
            break
    rec["iterations"] = it
    if flags == 0:
        flags = 0 if converged else NOT_CONVERGED
        v, n = ev((c, s, tx, ty), max_it - 1)
        if n < min_corr:
            flags = FEW
        else:
            rec.update(c=c, s=s, tx=tx, ty=ty, info=v[:6], cost=v[9], n_corr=n)
    rec["flags"] = flags
    return rec, trace


def refine(xy, normals, offsets, pair_src, pair_tgt, pose0, spec=None, **perturb):
    """A list of pairs: (refined REFINED_DTYPE (n,), trace float64 (n, 16, 4))."""
    spec = RefineFields() if spec is None else spec
    xy, normals = np.asarray(xy, dtype=F).reshape(-1, 2), np.asarray(normals, dtype=F).reshape(-1, 2)
    off = np.asarray(offsets, dtype=np.int64)
    n = len(pair_src)
    pose0 = np.asarray(pose0, dtype=np.float64).reshape(n, 4)
    out, trace = np.zeros(n, REFINED_DTYPE), np.zeros((n, SLOTS, 4))
    for i in range(n):
        s, t = int(pair_src[i]), int(pair_tgt[i])
        rec, trace[i] = refine_pair(xy[off[s]:off[s + 1]], xy[off[t]:off[t + 1]], normals[off[t]:off[t + 1]], pose0[i], spec, **perturb)
        for k, val in rec.items():
            out[i][k] = val
    return out, trace


# ---- the case list --------------------------------------------------------------------------------------------------
ROOM_W, ROOM_H = 6.0, 4.0
POSE_TGT, POSE_SRC = (3.0, 2.0, 0.3), (3.4, 2.2, 0.5)  # where the two scans of a pair are taken, in the room's frame
START_OFF = (0.03, -0.02, math.radians(0.5))           # the start pose's error: what a lattice leaves


def room_points(n, rng, walls=(0, 1, 2, 3)):
    """n points on the walls of the room and the walls' inward normals, both (n, 2) float64."""
    w = rng.choice(np.asarray(walls), n)
    u = rng.random(n)
    pts = np.stack([np.where(w == 0, u * ROOM_W, np.where(w == 1, ROOM_W, np.where(w == 2, u * ROOM_W, 0.0))),
                    np.where(w == 0, 0.0, np.where(w == 1, u * ROOM_H, np.where(w == 2, ROOM_H, u * ROOM_H)))], axis=1)
    nrm = np.stack([np.where(w == 1, -1.0, np.where(w == 3, 1.0, 0.0)), np.where(w == 0, 1.0, np.where(w == 2, -1.0, 0.0))], axis=1)
    return pts, nrm


def view(pts, nrm, pose, rng, noise=0.002):
    """World points and normals as a scan taken at pose sees them: float32 (n, 2) each."""
    c, s = math.cos(pose[2]), math.sin(pose[2])
    d = pts - np.asarray(pose[:2])
    p = np.stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1]], axis=1) + rng.normal(0, noise, pts.shape)
    m = np.stack([c * nrm[:, 0] + s * nrm[:, 1], -s * nrm[:, 0] + c * nrm[:, 1]], axis=1)
    return p.astype(F), m.astype(F)


def true_pose(off=(0.0, 0.0, 0.0)):
    """(c, s, tx, ty) taking the source scan's frame into the target's, displaced by off = (dx, dy, dtheta)."""
    ct, st = math.cos(POSE_TGT[2]), math.sin(POSE_TGT[2])
    dx, dy = POSE_SRC[0] - POSE_TGT[0], POSE_SRC[1] - POSE_TGT[1]
    th = POSE_SRC[2] - POSE_TGT[2] + off[2]
    return np.array([math.cos(th), math.sin(th), ct * dx + st * dy + off[0], -st * dx + ct * dy + off[1]])


class Case:
    """Packed scans, pairs, start poses and the spec's overrides."""

    def __init__(self, name, scans, normals, pair_src, pair_tgt, pose0, **spec_kw):
        self.name = name
        self.xy = np.concatenate(scans).astype(F).reshape(-1, 2)
        self.normals = np.concatenate(normals).astype(F).reshape(-1, 2)
        self.offsets = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int32)
        self.pair_src, self.pair_tgt = np.asarray(pair_src, np.int32), np.asarray(pair_tgt, np.int32)
        self.pose0 = np.asarray(pose0, np.float64).reshape(len(self.pair_src), 4)
        self.spec_kw = spec_kw

    def fields(self):
        return RefineFields(**self.spec_kw)


def pair_case(name, ns, nt, seed, same=False, walls=(0, 1, 2, 3), start=None, edit=None, **spec_kw):
    """One pair: scan 0 the source (ns points), scan 1 the target (nt points) of the room; same: the source sees the target's
    own world points.  edit(src, srcn, tgt, tgn) may change the four arrays in place."""
    rng = np.random.default_rng(seed)
    tw, tn = room_points(nt, rng, walls)
    sw, sn = (tw[:ns], tn[:ns]) if same else room_points(ns, rng, walls)
    tgt, tgn = view(tw, tn, POSE_TGT, rng)
    src, srcn = view(sw, sn, POSE_SRC, rng)
    if edit is not None:
        src, srcn, tgt, tgn = edit(src, srcn, tgt, tgn)
    return Case(name, [src, tgt], [srcn, tgn], [0], [1], true_pose(START_OFF) if start is None else start, **spec_kw)


def _poison_target(src, srcn, tgt, tgn):
    tgt[5, 0], tgt[6, 0], tgt[7, 1], tgt[8] = np.nan, np.inf, -np.inf, (1.0e7, 1.0)
    tgt[9] = (tgt[10, 0], 1.0e7)
    tgn[20:60, 0] = np.nan
    tgn[60:70, 1] = np.inf
    return src, srcn, tgt, tgn


def _poison_source(src, srcn, tgt, tgn):
    src[3, 0], src[4, 1], src[5, 0], src[300] = np.nan, np.inf, -1.0e7, (1.0e6, 0.0)
    return src, srcn, tgt, tgn


def _far_target(src, srcn, tgt, tgn):
    tgt[11] = (5000.0, 0.0)  # a valid point beyond the float cell range: the search goes exhaustive
    return src, srcn, tgt, tgn


def _equal_normals(src, srcn, tgt, tgn):
    tgn[:] = (0.0, 1.0)
    return src, srcn, tgt, tgn


def _duplicates(src, srcn, tgt, tgn):
    """The first 200 target points once more at the end with normals turned by 0.2 rad: exact ties, the lowest index wins."""
    c, s = F(math.cos(0.2)), F(math.sin(0.2))
    n2 = np.stack([c * tgn[:200, 0] - s * tgn[:200, 1], s * tgn[:200, 0] + c * tgn[:200, 1]], axis=1).astype(F)
    return src, srcn, np.concatenate([tgt, tgt[:200]]), np.concatenate([tgn, n2])


def _threshold_edge(src, srcn, tgt, tgn):
    """Lone target points far from the room and source points 0.25 m beside them, one float less and one float more: at the
    identity start pose the first evaluation keeps the distance below thr[0] = 0.25 alone."""
    base = np.array([[-20.0, -20.0 - 3.0 * j] for j in range(3)], F)
    d = [np.nextafter(F(-19.75), F(-30.0)), F(-19.75), np.nextafter(F(-19.75), F(0.0))]
    extra = np.array([[d[j], base[j, 1]] for j in range(3)], F)
    one = np.tile(np.array([[1.0, 0.0]], F), (3, 1))
    return np.concatenate([src, extra]), np.concatenate([srcn, one]), np.concatenate([tgt, base]), np.concatenate([tgn, one])


def _many_pairs():
    """300 pairs that share 30 targets: scans 0..29 the targets (150 points), 30..329 the sources (120 points)."""
    rng = np.random.default_rng(77)
    scans, nrms = [], []
    for _ in range(30):
        p, m = view(*room_points(150, rng), POSE_TGT, rng)
        scans.append(p), nrms.append(m)
    for _ in range(300):
        p, m = view(*room_points(120, rng), POSE_SRC, rng)
        scans.append(p), nrms.append(m)
    offs = rng.normal(0, 1.0, (300, 3)) * (0.03, 0.03, math.radians(0.5))
    return Case("pairs300", scans, nrms, 30 + np.arange(300), np.arange(300) % 30, [true_pose(o) for o in offs])


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for k, ns in enumerate((1, 63, 64, 255, 256, 257, 2047, 2048, 2049, 4100)):
        out.append(pair_case("src%d" % ns, ns, 600, 100 + k, min_corr=3))
    for k, nt in enumerate((0, 1)):
        out.append(pair_case("tgt%d" % nt, 50, nt, 200 + k))
    for k, nt in enumerate((29, 30)):
        out.append(pair_case("tgt%d" % nt, nt, nt, 210 + k, same=True))
    for k, nt in enumerate((2047, 2048, 2049)):
        out.append(pair_case("tgt%d" % nt, 300, nt, 220 + k))
    out.append(pair_case("iter1", 400, 500, 300, max_iterations=1))
    out.append(pair_case("iter8", 400, 500, 301, step_tol_m=0.0, step_tol_rad=0.0))
    out.append(pair_case("iter16", 400, 500, 302, max_iterations=16, step_tol_m=0.0, step_tol_rad=0.0))
    out.append(pair_case("one_update", 400, 500, 303, step_tol_m=1.0, step_tol_rad=1.0))
    out.append(pair_case("few", 400, 500, 310, start=true_pose((5.0, 0.0, 0.0))))
    out.append(pair_case("corridor", 400, 500, 311, walls=(0, 2)))
    out.append(pair_case("equal_normals", 400, 500, 312, edit=_equal_normals))
    out.append(pair_case("runaway", 400, 500, 313, max_shift_m=1e-4))
    out.append(pair_case("skipped", 400, 500, 314, start=[np.nan] * 4))
    out.append(pair_case("poison_target", 400, 600, 320, edit=_poison_target))
    out.append(pair_case("poison_source", 400, 600, 321, edit=_poison_source))
    out.append(pair_case("far_target", 400, 600, 322, edit=_far_target))
    out.append(pair_case("far_pose", 400, 600, 323, start=true_pose((2000.0, 0.0, 0.0))))
    out.append(pair_case("duplicates", 400, 600, 324, edit=_duplicates))
    rng = np.random.default_rng(330)
    tw, tn = room_points(500, rng)
    tgt, tgn = view(tw, tn, POSE_TGT, rng)
    sw, sn = room_points(400, rng)
    src, srcn = view(sw, sn, POSE_TGT, rng)  # (the same place: the identity is the true pose, and q = p exactly under it)
    src, srcn, tgt, tgn = _threshold_edge(src, srcn, tgt, tgn)
    out.append(Case("threshold_edge", [src, tgt], [srcn, tgn], [0], [1], [[1.0, 0.0, 0.0, 0.0]], max_iterations=1))
    out.append(_many_pairs())
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(refined, trace) of the named case, computed once per process."""
    cs = case(name)
    return refine(cs.xy, cs.normals, cs.offsets, cs.pair_src, cs.pair_tgt, cs.pose0, cs.fields())
