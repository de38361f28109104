"""numpy restatement of "Loop-closure consistency" (DESIGN.md section 3), written from that text: the pair test on prepared
records, the bit matrix, the degrees and the greedy set.  It shares no code with nautilus_amd.hostside; the prepared records
themselves come from consistency.prepare, the one function behind every path.  Also the fixture the spec's defaults were chosen
on (fixture(), study())."""
import math

import numpy as np


def pair_quantities(rec, lo, hi, spec):
    """(e2, tt2, chord, tr2) of the pairs (lo[k], hi[k]), lo < hi, every operation a float64 operation rounded on its own."""
    cl, sl, xl, yl, pxl, pyl, lal, lbl = (rec[lo, k] for k in range(8))
    ch, sh, xh, yh, _, _, lah, lbh = (rec[hi, k] for k in range(8))
    with np.errstate(invalid="ignore", over="ignore"):
        ihx = -(ch * xh + sh * yh)
        ihy = sh * xh - ch * yh
        cq = cl * ch + sl * sh
        sq = sl * ch - cl * sh
        qx = (cl * ihx - sl * ihy) + xl
        qy = (sl * ihx + cl * ihy) + yl
        ex = ((cq * pxl - sq * pyl) + qx) - pxl
        ey = ((sq * pxl + cq * pyl) + qy) - pyl
        e2 = ex * ex + ey * ey
        chord = 2.0 - 2.0 * cq
        ell = np.abs(lal - lah) + np.abs(lbl - lbh)
        tt = spec.t0 + spec.t_rate * ell
        tr = spec.r0 + spec.r_rate * ell
        tt = np.where(spec.t_max < tt, spec.t_max, tt)  # min(a, b) = b < a ? b : a
        tr = np.where(spec.r_max < tr, spec.r_max, tr)
        return e2, tt * tt, chord, tr * tr


def adjacency_bool(rec, spec):
    M = len(rec)
    m, n = np.meshgrid(np.arange(M), np.arange(M), indexing="ij")
    e2, tt2, chord, tr2 = pair_quantities(rec, np.minimum(m, n), np.maximum(m, n), spec)
    with np.errstate(invalid="ignore"):
        return (e2 <= tt2) & (chord <= tr2) & (m != n)


def pack(A):
    """M rows of ceil(M / 64) uint64 words: bit n of row m is bit n % 64 of word n // 64."""
    M = len(A)
    W = (M + 63) // 64
    padded = np.zeros((M, W * 64), dtype=np.uint8)
    padded[:, :M] = A
    weights = np.uint64(1) << np.arange(64, dtype=np.uint64)
    return (padded.reshape(M, W, 64).astype(np.uint64) * weights).sum(axis=2, dtype=np.uint64)


def greedy(A, deg, max_steps):
    """(members in pick order, steps, 1 if the cap ended the set with C not empty)."""
    M = len(A)
    if M == 0:
        return [], 0, 0
    C = np.ones(M, dtype=bool)
    score = np.asarray(deg, dtype=np.int64)
    members = []
    while True:
        live = np.nonzero(C)[0]
        best = score[live].max()
        u = int(live[score[live] == best].min())
        members.append(u)
        C = C & A[u]
        C[u] = False
        if not C.any():
            return members, len(members), 0
        if len(members) >= max_steps:
            return members, len(members), 1
        live = np.nonzero(C)[0]
        score = np.zeros(M, dtype=np.int64)
        score[live] = A[np.ix_(live, live)].sum(axis=1)


def consistent_set(rec, spec):
    """dict(adj uint64 (M, W), deg int32 (M,), members int32 (M,) (-1 behind the set), n_members, stats int64 (8,),
    adj_stats int64 (8,): what the adjacency call alone reports)."""
    rec = np.asarray(rec, dtype=np.float64).reshape(-1, 8)
    M = len(rec)
    A = adjacency_bool(rec, spec) if M else np.zeros((0, 0), dtype=bool)
    deg = A.sum(axis=1).astype(np.int32)
    picked, steps, cap = greedy(A, deg, int(spec.max_steps))
    members = np.full(M, -1, dtype=np.int32)
    members[:len(picked)] = picked
    stats = np.zeros(8, dtype=np.int64)
    stats[:5] = (M, int(deg.sum()) // 2, int(deg.max()) if M else 0, steps, cap)
    adj_stats = stats.copy()
    adj_stats[3:] = 0
    return dict(adj=pack(A), deg=deg, members=members, n_members=len(picked), stats=stats, adj_stats=adj_stats)


# ---- the fixture of the defaults' study -------------------------------------------------------------------------------------------

def compose(a, b):
    """a o b of poses (x, y, theta), rows."""
    c, s = np.cos(a[..., 2]), np.sin(a[..., 2])
    return np.stack([a[..., 0] + c * b[..., 0] - s * b[..., 1], a[..., 1] + s * b[..., 0] + c * b[..., 1], a[..., 2] + b[..., 2]], axis=-1)


def inverse(a):
    c, s = np.cos(a[..., 2]), np.sin(a[..., 2])
    return np.stack([-(c * a[..., 0] + s * a[..., 1]), s * a[..., 0] - c * a[..., 1], -a[..., 2]], axis=-1)


def fixture(seed=7, n_scans=2000, n_records=600, n_displaced=100, n_coherent=50):
    """A SynthBag(n_scans, poses_only=True) loop, its estimate drifted as examples/slam_loop.run drifts its own (0.02 m and 0.3
    degrees per step), n_records true records at separation > 20 and distance < 2 m with lattice noise of 2.5 cm and 0.01 rad;
    n_displaced of them displaced by 1.5 .. 3 m in a random direction, n_coherent by one and the same world-frame transform.
    Returns (poses, src, tgt, rel, kind): kind 0 untouched, 1 displaced, 2 coherent."""
    from nautilus_amd import synth
    bag = synth.SynthBag(n_scans, poses_only=True)
    est = synth.odometry_from_truth(bag.truth, sigma_t=0.02, sigma_th_deg=0.3, seed=synth.SEED)
    est = est - est[0] + bag.truth[0]
    rng = np.random.default_rng(seed)
    idx = np.arange(n_scans)
    d = np.linalg.norm(bag.truth[:, None, :2] - bag.truth[None, :, :2], axis=2)
    s, t = np.nonzero((d < 2.0) & (idx[:, None] - idx[None, :] > 20))
    pick = np.sort(rng.choice(len(s), n_records, replace=False))
    src, tgt = s[pick].astype(np.int32), t[pick].astype(np.int32)
    rel = compose(inverse(bag.truth[tgt]), bag.truth[src])
    rel[:, 2] -= 2 * math.pi * np.rint(rel[:, 2] / (2 * math.pi))
    rel[:, :2] += rng.uniform(-0.025, 0.025, (n_records, 2))
    rel[:, 2] += rng.uniform(-0.01, 0.01, n_records)
    kind = np.zeros(n_records, dtype=np.int32)
    touched = rng.permutation(n_records)[:n_displaced + n_coherent]
    disp, coh = touched[:n_displaced], touched[n_displaced:]
    r, a = rng.uniform(1.5, 3.0, n_displaced), rng.uniform(0, 2 * math.pi, n_displaced)
    rel[disp, 0] += r * np.cos(a)
    rel[disp, 1] += r * np.sin(a)
    kind[disp] = 1
    T = np.array([2.0, -1.5, 0.05])  # one world-frame transform: Z' = X_tgt^-1 o T o X_tgt o Z
    rel[coh] = compose(inverse(est[tgt[coh]]), compose(T[None, :], compose(est[tgt[coh]], rel[coh])))
    kind[coh] = 2
    rel = rel.astype(np.float32).astype(np.float64)  # (the records' floats, as the loop makes them)
    return est, src, tgt, rel, kind


def study(settings):
    """Kept records per kind of the fixture under each setting (a dict of spec overrides): rows (overrides, members, untouched
    kept, displaced kept, coherent kept)."""
    from nautilus_amd import consistency
    poses, src, tgt, rel, kind = fixture()
    rec = consistency.prepare(poses, src, tgt, rel)
    rows = []
    for kw in settings:
        got = consistent_set(rec, consistency.spec(**kw))
        mem = got["members"][:got["n_members"]]
        rows.append((kw, len(mem), int((kind[mem] == 0).sum()), int((kind[mem] == 1).sum()), int((kind[mem] == 2).sum())))
    return rows


# ---- the scenes both test files run (tests/test_consistency_cpu.py, tests/test_consistency_gpu.py) --------------------------------

def loop_records(M, seed=11, n_scans=400, shift=(0.0, 0.0), outliers=0.25):
    """M prepared records of a drifted loop: true revisits with lattice noise, a share of them displaced by 1.5 .. 3 m."""
    from nautilus_amd import consistency, synth
    bag = synth.SynthBag(n_scans, poses_only=True)
    est = synth.odometry_from_truth(bag.truth, sigma_t=0.02, sigma_th_deg=0.3, seed=synth.SEED)
    est = est - est[0] + bag.truth[0]
    est[:, :2] += np.asarray(shift, dtype=np.float64)
    rng = np.random.default_rng(seed)
    idx = np.arange(n_scans)
    d = np.linalg.norm(bag.truth[:, None, :2] - bag.truth[None, :, :2], axis=2)
    s, t = np.nonzero((d < 2.0) & (idx[:, None] - idx[None, :] > 20))
    pick = rng.choice(len(s), M, replace=M > len(s))
    src, tgt = s[pick], t[pick]
    rel = compose(inverse(bag.truth[tgt]), bag.truth[src])
    rel[:, :2] += rng.uniform(-0.025, 0.025, (M, 2))
    rel[:, 2] += rng.uniform(-0.01, 0.01, M)
    bad = rng.random(M) < outliers
    r, a = rng.uniform(1.5, 3.0, M), rng.uniform(0, 2 * math.pi, M)
    rel[bad, 0] += (r * np.cos(a))[bad]
    rel[bad, 1] += (r * np.sin(a))[bad]
    return consistency.prepare(est, src, tgt, rel.astype(np.float32).astype(np.float64))


def plane_records(xy, p=(3.0, -2.0), la=5.0, lb=40.0):
    """Records whose W is the translation xy[m], all at one place: with the rates' term 0 the matrix is the unit-disk graph of
    the points xy with radius t0."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    rec = np.zeros((len(xy), 8))
    rec[:, 0], rec[:, 2:4], rec[:, 4:6], rec[:, 6], rec[:, 7] = 1.0, xy, p, la, lb
    return rec


def edge_specs(rec, which):
    """For the 2-record scene `rec`: specs that put the pair one ulp below, exactly on (where a double's square hits it; else the
    first double whose square is not below) and one ulp above the tolerance `which` ("t0", "r0", "t_max", "r_max"), as (name,
    spec overrides, the pair is consistent)."""
    from nautilus_amd import consistency
    wide = consistency.spec(t0=1e3, t_max=1e3, r0=1e3, r_max=1e3)
    e2, _, chord, _ = (float(v[0]) for v in pair_quantities(rec, np.array([0]), np.array([1]), wide))
    target = e2 if which in ("t0", "t_max") else chord
    t = math.sqrt(target)
    while t * t >= target:
        t = math.nextafter(t, 0.0)
    while t * t < target:
        t = math.nextafter(t, math.inf)  # the smallest double whose square is not below the target
    out = []
    for name, v, ok in (("below", math.nextafter(t, 0.0), False), ("on", t, True), ("above", math.nextafter(t, math.inf), True)):
        if which == "t0":
            kw = dict(t0=v, t_rate=0.0, t_max=1e3, r0=1e3, r_max=1e3)
        elif which == "r0":
            kw = dict(r0=v, r_rate=0.0, r_max=1e3, t0=1e3, t_max=1e3)
        elif which == "t_max":  # t0 + t_rate len lies far above the cap: the cap decides
            kw = dict(t0=0.0, t_rate=1e3, t_max=v, r0=1e3, r_max=1e3)
        else:
            kw = dict(r0=0.0, r_rate=1e3, r_max=v, t0=1e3, t_max=1e3)
        out.append(("%s_%s" % (which, name), kw, ok))
    return out


def scenes():
    """name -> (records (M, 8), spec overrides)."""
    S = {}
    for M in (0, 1, 2, 63, 64, 65, 127, 128, 129, 257, 1025):
        S["loop_%d" % M] = (loop_records(M), {})
    S["edge_free_70"] = (plane_records(np.stack([100.0 * np.arange(70), np.zeros(70)], axis=1)), {})
    for M in (65, 130):
        S["identical_%d" % M] = (plane_records(np.zeros((M, 2))), {})
    # two cliques of 33, too far apart to touch; record 0 is in the second one
    far = np.zeros((66, 2))
    far[[k for k in range(66) if k == 0 or (k % 2 == 0 and k != 2) or k == 65][:33], 0] = 500.0
    S["two_cliques_66"] = (plane_records(far), {})
    # a clique of 4 at (1.45, 0), and a hub at the origin with 6 spokes at radius 0.7 whose first touches the clique: the hub
    # and that spoke have the largest degrees and are in no clique larger than 2 with each other
    spokes = [(0.7 * math.cos(k * math.pi / 3), 0.7 * math.sin(k * math.pi / 3)) for k in range(6)]
    clique = [(1.45, 0.0), (1.45, 0.01), (1.46, 0.0), (1.46, 0.01)]
    S["pendant_11"] = (plane_records(clique + [(0.0, 0.0)] + spokes), dict(t0=0.76, t_rate=0.0))
    S["far_10km_129"] = (loop_records(129, shift=(1.0e4, -1.0e4)), {})
    bad = loop_records(70)
    bad[5], bad[64] = np.nan, np.inf
    bad[17, 3], bad[40, 6] = np.nan, np.nan
    S["nan_inf_70"] = (bad, {})
    S["capped_130"] = (plane_records(np.zeros((130, 2))), dict(max_steps=70))
    S["capped_loop_257"] = (loop_records(257), dict(max_steps=9))
    pair = loop_records(2, seed=5, outliers=0.0)
    for which in ("t0", "r0", "t_max", "r_max"):
        for name, kw, _ in edge_specs(pair, which):
            S["edge_" + name] = (pair, kw)
    exact = plane_records([(0.3, 0.0), (0.0, 0.0)], p=(0.0, 0.0))  # e2 = 0.3 * 0.3 exactly as t0 = 0.3 squares
    for name, v in (("below", math.nextafter(0.3, 0.0)), ("on", 0.3), ("above", math.nextafter(0.3, 1.0))):
        S["exact_t0_" + name] = (exact, dict(t0=v, t_rate=0.0))
    return S


_CACHE = {}


def scene_results():
    """name -> (records, spec, the reference's result), computed once per process and never changed."""
    if not _CACHE:
        from nautilus_amd import consistency
        for name, (rec, kw) in scenes().items():
            sp = consistency.spec(**kw)
            _CACHE[name] = (rec, sp, consistent_set(rec, sp))
    return _CACHE
