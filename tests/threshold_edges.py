"""Designed inputs for the distance gates: offsets whose float norm lands on the two roots that decide a comparison.

A gate computes d2 = fl(fl(dx * dx) + fl(dy * dy)), takes a correctly rounded float root and compares it with a threshold.
For one threshold only two roots matter: `lo`, the largest float32 that passes, and `hi`, its successor.  A root that a
device rounds one ulp the wrong way flips the decision only for the handful of d2 values whose exact root is lo or hi, and
random clouds never touch them.  This module finds those d2 values and offsets (dx, dy) that produce them, by
generate-and-filter in plain numpy (float32 numpy operations round one by one; np.sqrt on float32 is correctly rounded).

Test infrastructure: no device, no library.  tests/test_threshold_edges_cpu.py ties the cases to the CPU oracles."""
import functools
import math

import numpy as np

F32 = np.float32
NAMED = [0.25, 0.03, 0.05, 0.1, 0.2, 0.6, 3.5, 7.5]      # the project's own thresholds
DIVIDED = [0.25 / i for i in (2, 3, 4)]                   # GetPointToNormalMatching divides the outlier threshold


def thresholds(n=128, seed=20240229):
    """The named thresholds, 0.25 / i, and a seeded log-uniform sample of [0.01, 10] to fill up to n (Python floats)."""
    rng = np.random.default_rng(seed)
    fill = np.exp(rng.uniform(math.log(0.01), math.log(10.0), 128 - len(NAMED) - len(DIVIDED)))
    return (NAMED + DIVIDED + [float(v) for v in fill])[:n]


def _next(x):
    return np.nextafter(F32(x), F32(np.inf))


def _prev(x):
    return np.nextafter(F32(x), F32(-np.inf))


def chain_d2(dx, dy):
    """fl(fl(dx * dx) + fl(dy * dy)) in float32."""
    dx, dy = np.asarray(dx, F32), np.asarray(dy, F32)
    return ((dx * dx).astype(F32) + (dy * dy).astype(F32)).astype(F32)


def chain_root(dx, dy):
    return np.sqrt(chain_d2(dx, dy)).astype(F32)


def passes(root, T, op, kind):
    """The site's comparison: `kind` "f32" compares floats against float32(T), "f64" widens the root and compares with T."""
    root = np.asarray(root, F32)
    if kind == "f32":
        return root < F32(T) if op == "<" else root <= F32(T)
    return root.astype(np.float64) < float(T) if op == "<" else root.astype(np.float64) <= float(T)


def critical_roots(T, op, kind):
    """(lo, hi): the largest float32 root that passes `root op T` and its successor."""
    lo = F32(T)  # nearest float: lo is it or its predecessor
    while not passes(lo, T, op, kind):
        lo = _prev(lo)
    while passes(_next(lo), T, op, kind):
        lo = _next(lo)
    return lo, _next(lo)


class Edge:
    """The cases of one threshold.  d2: the distinct float32 values whose root is lo or hi (ascending); offsets (n, 2)
    float32 with their d2 / root; T_down / T_up: the threshold moved one float32 step across lo / hi (a lo case passes at T
    and fails at T_down, a hi case fails at T and passes at T_up) -- in the site's threshold type, as Python floats."""

    def __init__(self, T, op, kind, quantum=0.0, per_d2_quadrant=1, seed=1):
        assert op in ("<", "<=") and kind in ("f32", "f64")
        self.T, self.op, self.kind, self.quantum = float(T), op, kind, float(quantum)
        self.lo, self.hi = critical_roots(T, op, kind)
        self.T_down = float(self.lo) if op == "<" else float(_prev(self.lo))
        self.T_up = float(_next(self.hi)) if op == "<" else float(self.hi)
        # every float32 d2 near lo^2 whose correctly rounded root is lo or hi: a few ulps either side of fl(lo * lo)
        c = F32(self.lo * self.lo)
        cand = [c]
        for _ in range(12):
            cand = [_prev(cand[0])] + cand + [_next(cand[-1])]
        cand = np.array(cand, F32)
        r = np.sqrt(cand).astype(F32)
        keep = (r == self.lo) | (r == self.hi)
        assert not keep[0] and not keep[-1], "the d2 window is too narrow"
        self.d2 = cand[keep]
        self.d2_root = r[keep]
        self._generate(per_d2_quadrant, seed)

    def _generate(self, per, seed):
        rng = np.random.default_rng(seed)
        lo, hi, q = self.lo, self.hi, self.quantum
        offs = []
        if q == 0.0:  # axis-aligned: sqrt(fl(r * r)) == r for every float r
            for r in (lo, hi):
                offs += [(r, 0.0), (-r, 0.0), (0.0, r), (0.0, -r)]
        # a random dx inside the circle, the dy that completes it and its neighbours on the grid, all four sign quadrants
        n = 4096
        step = q if q > 0.0 else None
        dx = (rng.uniform(0.05, 0.999, n) * float(lo))
        dx = (np.round(dx / step) * step).astype(F32) if step else dx.astype(F32)
        dy0 = np.sqrt(np.maximum(float(lo) ** 2 - dx.astype(np.float64) ** 2, 0.0))
        ks = np.arange(-6, 7)
        if step:
            dy = ((np.round(dy0 / step)[:, None] + ks[None, :]) * step).astype(F32)
        else:
            dy = dy0.astype(F32)[:, None].repeat(len(ks), 1)
            for j, k in enumerate(ks):
                for _ in range(abs(k)):
                    dy[:, j] = np.nextafter(dy[:, j], F32(np.inf if k > 0 else -np.inf))
        dxx = dx[:, None].repeat(len(ks), 1).ravel()
        dyy = dy.ravel()
        d2 = chain_d2(dxx, dyy)
        taken = {}
        for i in np.nonzero(np.isin(d2, self.d2) & (dyy > 0) & (dxx > 0))[0]:
            key = float(d2[i])
            if taken.get(key, 0) >= 4 * per:
                continue
            sx, sy = ((1, 1), (-1, 1), (-1, -1), (1, -1))[taken.get(key, 0) % 4]
            taken[key] = taken.get(key, 0) + 1
            offs.append((sx * float(dxx[i]), sy * float(dyy[i])))
        self.offsets = np.array(offs, F32).reshape(-1, 2)
        self.off_d2 = chain_d2(self.offsets[:, 0], self.offsets[:, 1])
        self.off_root = np.sqrt(self.off_d2).astype(F32)
        assert np.all((self.off_root == lo) | (self.off_root == hi))

    @property
    def is_lo(self):
        return self.off_root == self.lo

    def check(self, min_d2=0):
        """Both roots are present among the offsets, every sign quadrant, and (native resolution) at least min_d2 distinct d2."""
        assert self.is_lo.any() and (~self.is_lo).any(), "T=%r: a root is missing" % self.T
        o = self.offsets[(self.offsets != 0).all(1)]
        quads = {(bool(x > 0), bool(y > 0)) for x, y in o}
        assert len(quads) == 4, "T=%r: quadrants %s" % (self.T, quads)
        assert len(np.unique(self.off_d2)) >= min_d2, "T=%r: %d distinct d2" % (self.T, len(np.unique(self.off_d2)))
        if self.quantum == 0.0:
            assert (self.offsets == 0).any(1).sum() == 8
        return self


def lattice_step(T):
    """(S, Q): a power of two S >= 4 T, and the quantum Q = S * 2^-20.  q + o is exact in float32 for every lattice point q
    with |coordinates| <= 8 S and every offset o that is a multiple of Q with |o| <= S / 4, and so is (q + o) - q."""
    S = 2.0 ** math.ceil(math.log2(4.0 * float(T)))
    return S, S * 2.0 ** -20


def lattice(n, S):
    """n points of the 17 x 17 lattice of spacing S around the origin, as float32 (exact)."""
    a = np.arange(-8, 9)
    g = np.stack(np.meshgrid(a, a), -1).reshape(-1, 2).astype(np.float64) * S
    assert n <= len(g)
    return g[:n].astype(F32)


# ---- the inputs of each gate at one threshold (shared by tests/test_threshold_edges_cpu.py and the GPU tests) ----------
# Every builder returns plain arrays plus, per designed case, whether it sits on lo.  A case is LIVE when the oracle's output
# for it differs between the threshold T and T moved one float32 step across the case's root (Edge.T_down / T_up).

FAR = 3.0e7  # a target this far out has a cell coordinate beyond 4096 cells at every threshold here: the exhaustive walk


def corr_inputs(T, gated):
    """Scans and blocks of one correspondence-search batch at identity poses: sources on the lattice, one designed target
    each (gated: plus a nearer decoy whose normal fails the gate).  Blocks: hashed, exhaustive (a FAR target), and the same
    two with 289 sources (more than one round of a lane)."""
    S, Q = lattice_step(T)
    e = Edge(T, "<", "f32", quantum=Q)
    scans, normals, is_lo = [], [], []
    for n_src in (len(e.offsets), 289):
        src = lattice(n_src, S)
        o = e.offsets[np.arange(n_src) % len(e.offsets)]
        tgt = (src + o).astype(F32)
        seen = (tgt - src).astype(F32)  # the offset the kernel sees
        r = chain_root(seen[:, 0], seen[:, 1])
        keep = (r == e.lo) | (r == e.hi)
        src, tgt, r, o = src[keep], tgt[keep], r[keep], o[keep]
        nt = np.tile(F32([1.0, 0.0]), (len(tgt), 1))
        if gated:
            half = (np.round(o.astype(np.float64) / 2.0 / Q) * Q)
            tgt = np.concatenate([tgt, (src + half).astype(F32)])
            nt = np.concatenate([nt, np.tile(F32([0.0, 1.0]), (len(src), 1))])
        far = F32([[FAR, FAR]])
        scans += [src, tgt, np.concatenate([tgt, far])]
        normals += [np.tile(F32([1.0, 0.0]), (len(src), 1)), nt, np.concatenate([nt, F32([[1.0, 0.0]])])]
        is_lo.append(r == e.lo)
    off = np.zeros(len(scans) + 1, np.int32)
    off[1:] = np.cumsum([len(s) for s in scans])
    return dict(edge=e, xy=np.concatenate(scans), nrm=np.concatenate(normals), off=off,
                bs=np.array([0, 0, 3, 3], np.int32), bt=np.array([1, 2, 4, 5], np.int32), src_scan=[0, 0, 3, 3],
                is_lo=[is_lo[0], is_lo[0], is_lo[1], is_lo[1]], poses=np.zeros((len(scans), 3)), min_cos=0.5)


def corr_kept(c, rows, counts, cap):
    """Per block, per source point: whether the search kept a row for it (sources are distinct lattice points)."""
    out = []
    for b, s in enumerate(c["src_scan"]):
        got = {tuple(r[:2]) for r in rows[cap[b]:cap[b] + counts[b]]}
        out.append(np.array([tuple(p) in got for p in c["xy"][c["off"][s]:c["off"][s + 1]]]))
    return out


def corr_oracle(c, gated, thr):
    from oracle import oracle as O
    aff = O.pose_affines(c["poses"])
    if gated:
        return O.corr_search_gated_batch(c["xy"], c["nrm"], c["off"], c["bs"], c["bt"], aff, thr, c["min_cos"])
    return O.corr_search_batch(c["xy"], c["nrm"], c["off"], c["bs"], c["bt"], aff, thr)


def corr_check_live(c, gated, want):
    """Both roots in every block, and every case live.  want: the oracle's output at T.  Returns the number of cases."""
    e = c["edge"]
    at_T, down, up = (corr_kept(c, *w) for w in (want, corr_oracle(c, gated, e.T_down), corr_oracle(c, gated, e.T_up)))
    n = 0
    for b, lo in enumerate(c["is_lo"]):
        assert lo.any() and (~lo).any(), (e.T, b)
        assert np.array_equal(at_T[b], lo), (e.T, b, "kept at T")
        assert not down[b][lo].any() and up[b][~lo].all(), (e.T, b, "not live")
        n += len(lo)
    return n


def pair_gate_inputs(T):
    """Poses (doubles whose float conversions are exact), candidates and min_separation of one pair-gate call.  Case k: A_k
    on the lattice at index 2 k, C_k = A_k + o_k next to it (fails on separation alone when o_k passes), B_k = A_k + o_k at
    index 2 K + k.  The candidates are every pose, and pose 0 once more (a == b off the diagonal)."""
    S, Q = lattice_step(T)
    e = Edge(T, "<", "f32", quantum=Q)
    K = len(e.offsets)
    A = lattice(K, S).astype(np.float64)
    B = A + e.offsets.astype(np.float64)
    assert np.array_equal(B.astype(F32).astype(np.float64), B)
    poses = np.zeros((3 * K, 3))
    poses[0:2 * K:2, :2], poses[1:2 * K:2, :2], poses[2 * K:, :2] = A, B, B
    poses[:, 2] = np.random.default_rng(3).uniform(-3, 3, 3 * K)
    cand = np.concatenate([np.arange(3 * K), [0]]).astype(np.int32)
    return dict(edge=e, poses=poses, cand=cand, min_sep=1, a=2 * np.arange(K), c=2 * np.arange(K) + 1, b=2 * K + np.arange(K),
                is_lo=e.is_lo)


def pair_gate_check_live(c, want):
    from oracle import oracle as O
    e, lo, a, b = c["edge"], c["is_lo"], c["a"], c["b"]
    down, up = (O.pair_gate(c["poses"], c["cand"], t, c["min_sep"]) for t in (e.T_down, e.T_up))
    assert lo.any() and (~lo).any(), e.T
    for f in (want[a, b], want[b, a]):
        assert np.array_equal(f.astype(bool), lo), (e.T, "flags at T")
    assert not down[a, b][lo].any() and up[a, b][~lo].all() and not down[b, a][lo].any() and up[b, a][~lo].all(), (e.T, "not live")
    assert not want[a, c["c"]].any() and not up[a, c["c"]].any()  # the same offsets one index apart: separation alone
    assert want[c["c"], b].all() and not want[np.arange(len(want)), np.arange(len(want))].any() and not want[0, -1] and not want[-1, 0]
    return len(lo)


def feat_phase1_inputs(T, P=3):
    """Scans in which the left neighbour i - P + k of point i lies at a designed offset from it (point i at the origin, so the
    difference is the offset bit for bit): k = 0 and k = P - 1, i = P (the first point with left neighbours) and i = P + 3.
    Returns the spec's fields, xy, offsets and per scan (i, is_lo)."""
    e = Edge(T, "<=", "f64")
    rng = np.random.default_rng(int(T * 1e6) + 7)
    _, first = np.unique(e.off_d2, return_index=True)
    pick = sorted(set(first.tolist()) | {0, 3, 5, 6})  # one offset per d2 value, and four axis-aligned ones (both roots)
    scans, meta = [], []
    for c in pick:
        for k, i in ((0, P), (P - 1, P), (0, P + 3), (P - 1, P + 3)):
            n = i + P
            ang, rad = rng.uniform(0, 2 * np.pi, n), rng.uniform(0.25, 0.6, n) * T
            pts = np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1).astype(F32)
            pts[i] = 0.0
            pts[i - P + k] = e.offsets[c]
            scans.append(pts)
            meta.append((i, bool(e.is_lo[c])))
    off = np.zeros(len(scans) + 1, np.int32)
    off[1:] = np.cumsum([len(s) for s in scans])
    fields = dict(threshold=0.008, distance_threshold=2.0, max_neighbor_distance=float(T), neighbors_per_side=P, min_neighbors=2,
                  max_planar=20, max_edge=10)
    return dict(edge=e, fields=fields, moved="max_neighbor_distance", xy=np.concatenate(scans), off=off, meta=meta)


def _same(a, b):
    return (np.isnan(a) & np.isnan(b)) | (a == b)


def feat_phase1_check_live(c, want_scores):
    """Point i's score at T differs from its score at the moved threshold, and no other point's does."""
    from tests import feature_reference as R
    e, off = c["edge"], c["off"]
    moved = {}
    for name, t in (("down", e.T_down), ("up", e.T_up)):
        spec = R.Spec(**dict(c["fields"], **{c["moved"]: t}))
        moved[name] = np.concatenate([R.scores(c["xy"][off[s]:off[s + 1]], spec) for s in range(len(off) - 1)])
    los = [lo for _, lo in c["meta"]]
    assert any(los) and not all(los), e.T
    for s, (i, lo) in enumerate(c["meta"]):
        a, b = want_scores[off[s]:off[s + 1]], moved["down" if lo else "up"][off[s]:off[s + 1]]
        same = _same(a, b)
        assert not same[i] and same.sum() == len(a) - 1 and not np.isnan(a[i]), (e.T, s, "not live")
    return len(c["meta"])


def feat_phase2_inputs(T, edge):
    """Two scans of designed pairs (w_c on the lattice, p_c = w_c + o_c, neighbours in the scan): one that LDS holds and one
    of 2049 points with the pairs at its start, middle and end.  Everything else is a pile of coincident filler points, which
    have no score.  neighbors_per_side 2 and min_neighbors 1: a point is scored from its right neighbour alone, so every
    designed point is eligible -- for the planar walk at threshold +2, for the edge walk at -2 -- and whether both points of
    a pair are accepted hangs on their distance alone.  Returns per scan the pairs' (index of w, is_lo)."""
    S, Q = lattice_step(T)
    e = Edge(T, "<", "f64", quantum=Q)
    K = len(e.offsets)
    w = lattice(K, S)
    p = (w + e.offsets).astype(F32)
    seen = (w - p).astype(F32)
    assert np.array_equal(chain_root(seen[:, 0], seen[:, 1]), e.off_root)
    pairs = np.stack([w, p], 1).reshape(-1, 2)  # w_0 p_0 w_1 p_1 ...
    fill = F32([100.0 * S, 100.0 * S])
    short = np.concatenate([pairs, np.tile(fill, (3, 1))])
    long_ = np.tile(fill, (2049, 1))
    g = [0, K // 3, 2 * K // 3, K]
    at = [0, 1000, 2049 - 1 - 2 * (K - g[2])]  # (the last point has no right neighbour: it stays a filler)
    idx_long = np.zeros(K, np.int64)
    for j in range(3):
        n = g[j + 1] - g[j]
        long_[at[j]:at[j] + 2 * n] = pairs[2 * g[j]:2 * g[j + 1]]
        idx_long[g[j]:g[j + 1]] = at[j] + 2 * np.arange(n)
    off = np.array([0, len(short), len(short) + len(long_)], np.int32)
    fields = dict(threshold=-2.0 if edge else 2.0, distance_threshold=float(T), max_neighbor_distance=0.0, neighbors_per_side=2,
                  min_neighbors=1, max_planar=64, max_edge=64)
    return dict(edge=e, fields=fields, moved="distance_threshold", xy=np.concatenate([short, long_]), off=off, is_lo=e.is_lo,
                w_index=[2 * np.arange(K), idx_long], walk=1 if edge else 0)


def feat_phase2_check_live(c, want):
    """At T a lo pair has one point accepted and a hi pair both; across the root it is the other way round.  Returns, per
    scan, the acceptance rounds of the suppressing points (the first accepted point of each lo pair)."""
    from tests import feature_reference as R
    e, lo = c["edge"], c["is_lo"]
    sel = {"T": want}
    for name, t in (("down", e.T_down), ("up", e.T_up)):
        sel[name] = R.extract(c["xy"], c["off"], R.Spec(**dict(c["fields"], **{c["moved"]: t})))
    assert lo.any() and (~lo).any(), e.T
    rounds = []
    for s, wi in enumerate(c["w_index"]):
        def taken(x):
            idx, cnt = x[2 * c["walk"]][s], x[2 * c["walk"] + 1][s]
            assert cnt < idx.shape[0], "the cap was reached"
            acc = list(idx[:cnt])
            return np.array([(i in acc) + (i + 1 in acc) for i in wi]), acc
        n_T, acc = taken(sel["T"])
        assert np.array_equal(n_T, np.where(lo, 1, 2)), (e.T, s, n_T)
        assert (taken(sel["down"])[0][lo] == 2).all() and (taken(sel["up"])[0][~lo] == 1).all(), (e.T, s, "not live")
        rounds.append([min(acc.index(i) if i in acc else 99, acc.index(i + 1) if i + 1 in acc else 99) for i in wi[lo]])
    return rounds


# ---- one reference per threshold, computed once and shared by the CPU and the GPU tests (treat as read-only) -----------
@functools.lru_cache(maxsize=None)
def corr_case(T, gated):
    """(inputs, the oracle's (rows, counts, cap) at T, number of live cases); asserts both roots and 100 % live."""
    c = corr_inputs(T, gated)
    want = corr_oracle(c, gated, T)
    return c, want, corr_check_live(c, gated, want)


@functools.lru_cache(maxsize=None)
def pair_gate_case(T):
    from oracle import oracle as O
    c = pair_gate_inputs(T)
    want = O.pair_gate(c["poses"], c["cand"], T, c["min_sep"])
    return c, want, pair_gate_check_live(c, want)


@functools.lru_cache(maxsize=None)
def feat_phase1_case(T):
    from tests import feature_reference as R
    c = feat_phase1_inputs(T)
    want = R.extract(c["xy"], c["off"], R.Spec(**c["fields"]))
    return c, want, feat_phase1_check_live(c, want[4])


@functools.lru_cache(maxsize=None)
def feat_phase2_case(T, edge):
    """(inputs, the reference's output at T, per scan the acceptance rounds of the suppressing points)."""
    from tests import feature_reference as R
    c = feat_phase2_inputs(T, edge)
    want = R.extract(c["xy"], c["off"], R.Spec(**c["fields"]))
    return c, want, feat_phase2_check_live(c, want)
