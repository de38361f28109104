"""Relative-pose factors ("Relative-pose factors"; K23): the definition restated per factor in plain Python
floats, the case list the CPU and GPU tests share, and the bounds they assert.  Written from the definition, not from
nautilus_amd/hostside.py: tests/test_relpose_cpu.py holds the two against each other bit for bit.

Python floats are IEEE doubles and every operation below is one rounded operation, in the definition's order; cos, sin and atan2
are libm's, CAUCHY's log1p is log1p_pinned below: fdlibm's, in IEEE operations.  `wrong` swaps in one of three wrong rules (tests/test_relpose_cpu.py shows that the case list tells
each from the definition)."""
import math
import struct

import numpy as np

BAD_INFO, BAD_MEASUREMENT, SAME_POSE = 1, 2, 4
KINDS = ("none", "huber", "soft_l1", "cauchy")
SCALE_OF = {"none": 1.0, "huber": 2.0, "soft_l1": 0.37, "cauchy": 3.0}  # in standard deviations: inliers and outliers on the list
N_POSES = 40
U = 2.0 ** -53


def _hi(x):
    return struct.unpack("<q", struct.pack("<d", x))[0] >> 32


def _with_hi(x, hi):
    return struct.unpack("<d", struct.pack("<Q", ((hi & 0xffffffff) << 32) | (struct.unpack("<Q", struct.pack("<d", x))[0] & 0xffffffff)))[0]


def log1p_pinned(x):
    """log1p(x), x >= 0 and finite, as the relative-pose rows take it: fdlibm's s_log1p.c for x >= 0, every operation rounded once."""
    ln2_hi, ln2_lo = 6.93147180369123816490e-01, 1.90821492927058770002e-10
    Lp = (6.666666666666735130e-01, 3.999999999940941908e-01, 2.857142874366239149e-01, 2.222219843214978396e-01,
          1.818357216161805012e-01, 1.531383769920937332e-01, 1.479819860511658591e-01)
    hx = _hi(x)
    if hx < 0x3e200000:
        return x if hx < 0x3c900000 else x - x * x * 0.5
    k, hu, f, c = 0, 1, x, 0.0
    if hx >= 0x3FDA827A:
        if hx < 0x43400000:
            u = 1.0 + x
            hu = _hi(u)
            k = (hu >> 20) - 1023
            c = (1.0 - (u - x) if k > 0 else x - (u - 1.0)) / u
        else:
            u = x
            hu = _hi(u)
            k = (hu >> 20) - 1023
        hu &= 0x000fffff
        if hu < 0x6a09e:
            u = _with_hi(u, hu | 0x3ff00000)
        else:
            k += 1
            u = _with_hi(u, hu | 0x3fe00000)
            hu = (0x00100000 - hu) >> 2
        f = u - 1.0
    hfsq, kd = 0.5 * f * f, float(k)
    if hu == 0:
        if f == 0.0:
            return 0.0 if k == 0 else kd * ln2_hi + (c + kd * ln2_lo)
        R = hfsq * (1.0 - 0.66666666666666666 * f)
        return f - R if k == 0 else kd * ln2_hi - ((R - (kd * ln2_lo + c)) - f)
    s = f / (2.0 + f)
    z = s * s
    R = z * (Lp[0] + z * (Lp[1] + z * (Lp[2] + z * (Lp[3] + z * (Lp[4] + z * (Lp[5] + z * Lp[6]))))))
    return f - (hfsq - s * (hfsq + R)) if k == 0 else kd * ln2_hi - ((hfsq - (s * (hfsq + R) + (kd * ln2_lo + c))) - f)


def log1p_cases():
    """Arguments of log1p_pinned: its branch seams (2^-54, 2^-29, 0.41422 = the high word 0x3FDA827A, sqrt(2) - 1 and 2^k sqrt(2) - 1
    either side, 2^53), 1 + x with an empty fraction and fractions below 2^-20, and 4,000 drawn log-uniformly and uniformly."""
    rng = np.random.default_rng(17)
    seams = [0.0, 2.0 ** -1074, 2.0 ** -54, 2.0 ** -29, _with_hi(0.0, 0x3FDA827A), 2.0 ** 0.5 - 1.0, 1.0, 3.0, 2.0 ** 0.5 * 2 - 1, 2.0 ** 0.5 * 8 - 1,
             2.0 ** 53, 1.0 + 2.0 ** -30, 3.0 + 2.0 ** -25, 2.0 ** 20 - 1.0, 1e300, 1.7976931348623157e308]
    near = [v for s_ in seams for v in (math.nextafter(s_, 0.0), s_, math.nextafter(s_, math.inf)) if 0.0 <= v < math.inf]
    return np.array(near + list(10.0 ** rng.uniform(-17, 16, 2000)) + list(rng.uniform(0.0, 4.0, 2000)), dtype=np.float64)


def loss_value(kind, a, s):
    """(rho, rho') of DESIGN.md section 3, "Robust loss", in its operation order."""
    b = a * a
    if kind == "huber":
        if s <= b:
            return s, 1.0
        q = math.sqrt(s)
        return (2.0 * a) * q - b, a / q
    if kind == "soft_l1":
        x = s / b
        q = math.sqrt(1.0 + x)
        return (2.0 * s) / (q + 1.0), 1.0 / q
    if kind == "cauchy":
        x = s / b
        return (s if x < 2.0 ** -54 else b * log1p_pinned(x)), 1.0 / (1.0 + x)
    return s, 1.0


def flags_of(z, L, same_pose):
    fl = 0
    ok = all(math.isfinite(v) for v in L)
    if ok:
        L00, L01, L02, L11, L12, L22 = L
        ok = L00 > 0.0
        if ok:
            l10, l20 = L01 / L00, L02 / L00
            D1 = L11 - l10 * L01
            ok = D1 > 0.0
            if ok:
                u = L12 - l20 * L01
                l21 = u / D1
                D2 = (L22 - l20 * L02) - l21 * u
                ok = D2 > 0.0
    if not ok:
        fl |= BAD_INFO
    if not all(math.isfinite(v) for v in z):
        fl |= BAD_MEASUREMENT
    if same_pose:
        fl |= SAME_POSE
    return fl


def error(z, pa, pb):
    """(e (3), E (3 x 6), (c_a, s_a, c_b, s_b)) of one factor: the unwhitened error and its Jacobian over [a | b]."""
    ca, sa, cb, sb = math.cos(pa[2]), math.sin(pa[2]), math.cos(pb[2]), math.sin(pb[2])
    Dx, Dy = pb[0] - pa[0], pb[1] - pa[1]
    dx, dy = ca * Dx + sa * Dy, (-sa) * Dx + ca * Dy
    cr, sr = ca * cb + sa * sb, ca * sb - sa * cb
    ce, se = cr * z[2] + sr * z[3], sr * z[2] - cr * z[3]
    e = [dx - z[0], dy - z[1], math.atan2(se, ce)]
    E = [[-ca, -sa, dy, ca, sa, 0.0], [sa, -ca, -dx, -sa, ca, 0.0], [0.0, 0.0, -1.0, 0.0, 0.0, 1.0]]
    return e, E, (ca, sa, cb, sb)


def whitener(L):
    """W (3 x 3 upper triangular, zeros below) of an information that passed flags_of."""
    L00, L01, L02, L11, L12, L22 = L
    D0 = L00
    l10, l20 = L01 / D0, L02 / D0
    D1 = L11 - l10 * L01
    u = L12 - l20 * L01
    l21 = u / D1
    D2 = (L22 - l20 * L02) - l21 * u
    q0, q1, q2 = math.sqrt(D0), math.sqrt(D1), math.sqrt(D2)
    return [[q0, q0 * l10, q0 * l20], [0.0, q1, q1 * l21], [0.0, 0.0, q2]]


def factor(z, L, pa, pb, same_pose=False, kind="none", a=1.0, wrong=None):
    """One factor: (r (3), J (3 x 6), row (28), weights (4), flags); zeros under a flag.
    wrong: None, "sign" (d d_x / d theta_a negated), "transpose" (W^T in W's place), "swap" (a and b exchanged)."""
    fl = flags_of(z, L, same_pose)
    if fl:
        return [0.0] * 3, [[0.0] * 6 for _ in range(3)], [0.0] * 28, [0.0] * 4, fl
    if wrong == "swap":
        pa, pb = pb, pa
    e, E, _ = error(z, pa, pb)
    if wrong == "sign":
        E[0][2] = -E[0][2]
    W = whitener(L)
    if wrong == "transpose":
        W = [[W[0][0], 0.0, 0.0], [W[0][1], W[1][1], 0.0], [W[0][2], W[1][2], W[2][2]]]
        r = [W[0][0] * e[0], W[1][0] * e[0] + W[1][1] * e[1], W[2][0] * e[0] + W[2][1] * e[1] + W[2][2] * e[2]]
        J = [[W[0][0] * E[0][p] for p in range(6)], [W[1][0] * E[0][p] + W[1][1] * E[1][p] for p in range(6)],
             [W[2][0] * E[0][p] + W[2][1] * E[1][p] + W[2][2] * E[2][p] for p in range(6)]]
    else:
        r = [W[0][0] * e[0] + W[0][1] * e[1] + W[0][2] * e[2], W[1][1] * e[1] + W[1][2] * e[2], W[2][2] * e[2]]
        J = [[W[0][0] * E[0][p] + W[0][1] * E[1][p] + W[0][2] * E[2][p] for p in range(6)],
             [W[1][1] * E[1][p] + W[1][2] * E[2][p] for p in range(6)], [W[2][2] * E[2][p] for p in range(6)]]
    s = r[0] * r[0] + r[1] * r[1] + r[2] * r[2]
    rho, rho1 = loss_value(kind, a, s)
    w = math.sqrt(rho1)
    rt = [w * v for v in r]
    Jt = [[w * v for v in row] for row in J]
    row = []
    for p in range(6):
        for q in range(p, 6):
            row.append(Jt[0][p] * Jt[0][q] + Jt[1][p] * Jt[1][q] + Jt[2][p] * Jt[2][q])
    for p in range(6):
        row.append(Jt[0][p] * rt[0] + Jt[1][p] * rt[1] + Jt[2][p] * rt[2])
    row.append(rho)
    return r, J, row, [s, rho, rho1, w], fl


def evaluate(case, kind="none", a=1.0, wrong=None):
    """The factors of a case (see `case`) one by one: (r (F, 3), J (F, 3, 6), rows (F, 28), weights (F, 4), flags (F,)).  A pose id
    outside [0, n) is zeros (and no flag), as on the device."""
    P, n = case["poses"], len(case["poses"])
    out = []
    for f in range(len(case["pose_i"])):
        ia, ib = int(case["pose_i"][f]), int(case["pose_j"][f])
        if not (0 <= ia < n and 0 <= ib < n):
            out.append(([0.0] * 3, [[0.0] * 6 for _ in range(3)], [0.0] * 28, [0.0] * 4,
                        flags_of([float(v) for v in case["z"][f]], [float(v) for v in case["info"][f]], ia == ib)))
            continue
        out.append(factor([float(v) for v in case["z"][f]], [float(v) for v in case["info"][f]], [float(v) for v in P[ia]],
                          [float(v) for v in P[ib]], ia == ib, kind, a, wrong))
    return (np.array([o[0] for o in out]).reshape(-1, 3), np.array([o[1] for o in out]).reshape(-1, 3, 6),
            np.array([o[2] for o in out]).reshape(-1, 28), np.array([o[3] for o in out]).reshape(-1, 4),
            np.array([o[4] for o in out], dtype=np.int32))


def evaluate_errors(case, trig):
    """(F, 2) e_x, e_y of a case recomputed in plain floats from given (c_a, s_a, ...) arrays (a device run's); zeros where a
    pose id is out of range."""
    P, n = case["poses"], len(case["poses"])
    out = np.zeros((len(case["pose_i"]), 2))
    for f in range(len(out)):
        ia, ib = int(case["pose_i"][f]), int(case["pose_j"][f])
        if not (0 <= ia < n and 0 <= ib < n):
            continue
        ca, sa = float(trig[0][f]), float(trig[1][f])
        Dx, Dy = float(P[ib][0]) - float(P[ia][0]), float(P[ib][1]) - float(P[ia][1])
        out[f] = (ca * Dx + sa * Dy) - float(case["z"][f][0]), ((-sa) * Dx + ca * Dy) - float(case["z"][f][1])
    return out


# ------------------------------------------------------------------------------------------------ the case list
def sym6(M):
    return [M[0][0], M[0][1], M[0][2], M[1][1], M[1][2], M[2][2]]


def correlated_info(cond=1e8):
    """I + (cond - 1) v v^T for a unit v off every axis: eigenvalues 1, 1, cond."""
    v = np.array([0.6, 0.64, 0.48])
    return sym6(np.eye(3) + (cond - 1.0) * np.outer(v, v))


ROOM_INFO = [420.0, -35.0, 610.0, 230.0, 95.0, 16000.0]  # the size of a room pair's H (translation 140-710, rotation ~10^4)
PI = math.pi
# (name, pose a, pose b, z = (x, y, theta) of the measurement or 4 raw doubles, information, flags expected)
SPECIAL = [
    ("zero error", (1.0, 2.0, 0.0), (3.0, 5.0, 0.0), (2.0, 3.0, 0.0), ROOM_INFO, 0),
    ("difference pi", (0.5, -1.0, 0.0), (1.5, 0.25, PI), (1.0, 1.25, 0.0), ROOM_INFO, 0),
    ("pi, one ulp below", (0.5, -1.0, 0.0), (1.5, 0.25, math.nextafter(PI, 0.0)), (1.0, 1.25, 0.0), ROOM_INFO, 0),
    ("pi, one ulp above", (0.5, -1.0, 0.0), (1.5, 0.25, math.nextafter(PI, 4.0)), (1.0, 1.25, 0.0), ROOM_INFO, 0),
    ("difference -pi", (0.5, -1.0, 0.0), (1.5, 0.25, -PI), (1.0, 1.25, 0.0), ROOM_INFO, 0),
    ("-pi, one ulp below", (0.5, -1.0, 0.0), (1.5, 0.25, math.nextafter(-PI, -4.0)), (1.0, 1.25, 0.0), ROOM_INFO, 0),
    ("-pi, one ulp above", (0.5, -1.0, 0.0), (1.5, 0.25, math.nextafter(-PI, 0.0)), (1.0, 1.25, 0.0), ROOM_INFO, 0),
    ("pi by the measurement", (2.0, 1.0, 0.3), (2.5, 1.5, 0.3), (0.6, 0.3, PI), ROOM_INFO, 0),
    ("equal headings", (2.0, 1.0, 0.7), (2.5, 1.5, 0.7), (0.6, 0.3, 0.01), ROOM_INFO, 0),
    ("far from the origin", (1000.0, -987.5, 2.9), (1001.0, -986.0, -3.0), (-1.2, -1.3, 0.35), ROOM_INFO, 0),
    ("far apart", (-1000.0, 1000.0, -1.0), (1000.0, -1000.0, 2.0), (500.0, 300.0, 3.0), ROOM_INFO, 0),
    ("information 1e-12", (0.1, 0.2, 0.3), (1.0, -0.5, 0.9), (0.7, -0.9, 0.55), [v * 1e-12 for v in ROOM_INFO], 0),
    ("information 1", (0.1, 0.2, 0.3), (1.0, -0.5, 0.9), (0.7, -0.9, 0.55), [1.0, 0.0, 0.0, 1.0, 0.0, 1.0], 0),
    ("information 1e12", (0.1, 0.2, 0.3), (1.0, -0.5, 0.9), (0.7, -0.9, 0.55), [v * 1e12 for v in ROOM_INFO], 0),
    ("correlated, condition 1e8", (0.1, 0.2, 0.3), (1.0, -0.5, 0.9), (0.7, -0.9, 0.55), correlated_info(), 0),
    ("an outlier", (0.1, 0.2, 0.3), (1.0, -0.5, 0.9), (2.7, -0.9, 0.55), ROOM_INFO, 0),
    ("information NaN", (0.1, 0.2, 0.3), (1.0, -0.5, 0.9), (0.7, -0.9, 0.55), [420.0, math.nan, 610.0, 230.0, 95.0, 16000.0], BAD_INFO),
    ("information inf", (0.1, 0.2, 0.3), (1.0, -0.5, 0.9), (0.7, -0.9, 0.55), [420.0, -35.0, 610.0, 230.0, 95.0, math.inf], BAD_INFO),
    ("first pivot 0", (0.1, 0.2, 0.3), (1.0, -0.5, 0.9), (0.7, -0.9, 0.55), [0.0, 0.0, 0.0, 1.0, 0.0, 1.0], BAD_INFO),
    ("second pivot negative", (0.1, 0.2, 0.3), (1.0, -0.5, 0.9), (0.7, -0.9, 0.55), [1.0, 2.0, 0.0, 1.0, 0.0, 1.0], BAD_INFO),
    ("third pivot 0", (0.1, 0.2, 0.3), (1.0, -0.5, 0.9), (0.7, -0.9, 0.55), [1.0, 0.0, 1.0, 1.0, 0.0, 1.0], BAD_INFO),
    ("all zeros", (0.1, 0.2, 0.3), (1.0, -0.5, 0.9), (0.7, -0.9, 0.55), [0.0] * 6, BAD_INFO),
    ("measurement NaN", (0.1, 0.2, 0.3), (1.0, -0.5, 0.9), (0.7, math.nan, 1.0, 0.0), ROOM_INFO, BAD_MEASUREMENT),
    ("measurement inf", (0.1, 0.2, 0.3), (1.0, -0.5, 0.9), (0.7, -0.9, math.inf, 0.0), ROOM_INFO, BAD_MEASUREMENT),
    ("both bad", (0.1, 0.2, 0.3), (1.0, -0.5, 0.9), (math.nan, -0.9, 1.0, 0.0), [-1.0, 0.0, 0.0, 1.0, 0.0, 1.0],
     BAD_INFO | BAD_MEASUREMENT),
    ("same pose", (0.1, 0.2, 0.3), None, (0.0, 0.0, 0.0), ROOM_INFO, SAME_POSE),
    ("same pose, bad information", (0.1, 0.2, 0.3), None, (0.0, 0.0, 0.0), [math.nan] * 6, SAME_POSE | BAD_INFO),
]


def _z(m):
    return [m[0], m[1], math.cos(m[2]), math.sin(m[2])] if len(m) == 3 else list(m)


def case(n, seed=5, special=True, flagged=True):
    """n factors over N_POSES poses: the SPECIAL cases first (each owns its poses; without `flagged` only those that expect no
    flag; as many as fit), then random room-sized factors -- poses within 10 m, measurements within centimetres and hundredths of
    a radian of the truth, every seventh a metre off (an outlier to every loss), informations ROOM_INFO scaled by 0.3 .. 3."""
    rng = np.random.default_rng(seed)
    poses = np.concatenate([rng.uniform(-10, 10, (N_POSES, 2)), rng.uniform(-PI, PI, (N_POSES, 1))], axis=1)
    pose_i, pose_j, z, info, want, names = [], [], [], [], [], []
    slots = {}  # the special cases' poses, shared by value

    def slot_of(p):
        if p not in slots:
            slots[p] = len(slots)
            poses[slots[p]] = p
        return slots[p]
    for name, pa, pb, m, L, fl in (SPECIAL if special else []):
        if len(pose_i) >= n or (fl and not flagged):
            continue
        assert len(slots) + 2 <= N_POSES - 8
        ia = slot_of(pa)
        ib = ia if pb is None else slot_of(pb)
        pose_i.append(ia), pose_j.append(ib), z.append(_z(m)), info.append(list(L)), want.append(fl), names.append(name)
    free = np.arange(len(slots), N_POSES)
    k = 0
    while len(pose_i) < n:
        ia, ib = (int(v) for v in rng.choice(free, 2, replace=False))
        pa, pb = poses[ia], poses[ib]
        ca, sa = math.cos(pa[2]), math.sin(pa[2])
        d = [ca * (pb[0] - pa[0]) + sa * (pb[1] - pa[1]), -sa * (pb[0] - pa[0]) + ca * (pb[1] - pa[1]), pb[2] - pa[2]]
        noise = rng.normal(0, [0.02, 0.02, 0.005])
        if k % 7 == 3:
            noise[0] += 1.0
        scale = float(rng.uniform(0.3, 3.0))
        pose_i.append(ia), pose_j.append(ib), z.append(_z(tuple(d + noise))), info.append([v * scale for v in ROOM_INFO])
        want.append(0), names.append("random %d" % k)
        k += 1
    return {"poses": np.ascontiguousarray(poses), "pose_i": np.array(pose_i, dtype=np.int32), "pose_j": np.array(pose_j, dtype=np.int32),
            "z": np.array(z, dtype=np.float64).reshape(-1, 4), "info": np.array(info, dtype=np.float64).reshape(-1, 6),
            "flags": np.array(want, dtype=np.int32), "names": names}


# ------------------------------------------------------------------------------------------------ bounds
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def info_matrix(L):
    return np.array([[L[0], L[1], L[2]], [L[1], L[3], L[4]], [L[2], L[4], L[5]]], dtype=np.float64)


def recompose_bound(L, terms=1):
    """8 * 2^-53 * ||Lambda|| (Frobenius) times the number of terms a sum runs over: what W^T W may miss Lambda by."""
    return 8.0 * U * float(np.linalg.norm(info_matrix(L))) * terms


def gauge_bound(pa, pb):
    """8 * 2^-53 * (1 + |t|), |t| the largest coordinate magnitude the error's sums see before and after a rigid motion."""
    return 8.0 * U * (1.0 + max(abs(v) for v in (pa[0], pa[1], pb[0], pb[1])))


def rigid(pose, angle, shift):
    """The pose after the rigid motion x -> R(angle) x + shift of the world."""
    c, s = math.cos(angle), math.sin(angle)
    return (c * pose[0] - s * pose[1] + shift[0], s * pose[0] + c * pose[1] + shift[1], pose[2] + angle)


def trig_reference(poses, pose_i, pose_j, z):
    """(F, 5) float64-rounded mpmath values of c_a, s_a, c_b, s_b, e_theta at the given (double) inputs, e_theta as the angle of
    the exact (c_e, s_e) -- the definition's products and sums without rounding."""
    import mpmath as mp
    mp.mp.prec = 200
    out = np.zeros((len(pose_i), 5), dtype=object)
    for f, (ia, ib) in enumerate(zip(pose_i, pose_j)):
        ta, tb = mp.mpf(float(poses[ia][2])), mp.mpf(float(poses[ib][2]))
        ca, sa, cb, sb = mp.cos(ta), mp.sin(ta), mp.cos(tb), mp.sin(tb)
        cz, sz = mp.mpf(float(z[f][2])), mp.mpf(float(z[f][3]))
        cr, sr = ca * cb + sa * sb, ca * sb - sa * cb
        out[f] = [ca, sa, cb, sb, mp.atan2(sr * cz - cr * sz, cr * cz + sr * sz)]
    return out
