"""Definitions of the four cost functors the residual kernels evaluate, in high precision, with an error bound beside
every value, and the inputs the residual kernels are tested on.

Written from the functor definitions (slam_residuals.h:18-40 OdometryResidual, :65-89 LIDARNormalResidual, :124-145
LIDARPointResidual, :180-200 PointToLineResidual; slam_util.h:20-28, 87-110), not from a kernel and not from
oracle/residuals_oracle.cc:

  LIDAR        q = A(target)^-1 A(source) p = R(th_s - th_t) p + R(th_t)^T (t_s - t_t),  A(x, y, th) = T(x, y) R(th)
               normal:  r = (n_t . (q - t),  n_s . (t - q))         point:  r = t - q
               dq/dt_s = R(th_t)^T   dq/dth_s = (-u_y, u_x), u = R(th_s - th_t) p   dq/dt_t = -R(th_t)^T   dq/dth_t = (q_y, -q_x)
  point-line   P = A(pose) p, S_k = A(line_pose) s_k; n = perp(S_1 - S_0) / len; sd = n . (P - S_0);
               r = |sd| if the projection P - sd n lies between the ends in x and in y, else min(|P - S_0|, |P - S_1|)
  odometry     r = (tw (t_i + t_odom - t_j),  rw wrap(th_i + r_odom - th_j)),  wrap(d) = atan2(sin d, cos d)

PRECISION.  Whatever depends on a pose alone -- sines, cosines, R(th_t)^T (t_s - t_t), the transformed segment ends, pose
minus segment end -- is computed with mpmath at MP_BITS bits and rounded once to numpy.longdouble (64-bit mantissa); the
per-row formulas then run on longdouble arrays and never subtract two absolute translations.  tests/test_resid_targets_cpu.py
holds the result against an all-mpmath evaluation: its own error is below 1 % of the bounds.

BOUNDS.  Beside every value stands a MAGNITUDE: the same expression with every term replaced by its absolute value,
translations taken one by one as the functor takes them (|x_s| + |x_t|, not |x_s - x_t|).  An output may differ from
the reference by K * 2**-53 * magnitude; a sum over n rows by (K + n) * 2**-53 * (sum of magnitudes).  A magnitude of
zero means the value is a constant of the functor (a zero of the odometry Jacobian) and must be equal.

K is one number per family.  It is the worst ratio |Jet oracle - reference| / (2**-53 * magnitude) over the family's
inputs below, measured on the CPU (tests/test_resid_targets_cpu.py prints and checks it), times 4 for a GPU's
different sin / cos and operation order, rounded up to a power of two, never below 4.  Never taken from a kernel.

WHERE THE FUNCTOR IS DISCONTINUOUS the double-precision evaluation is the definition: the branch of DistanceToLineSegment
is taken by restating its lines in IEEE double, operation by operation (p2l_branch_double) -- IsBetween(proj.y, 3, 3)
on a horizontal segment holds only when two roundings cancel, and that is what a drop-in must reproduce.  The inputs
make that restatement deterministic (headings of exactly 0 where it matters, a margin from every boundary elsewhere);
the odometry wrap cases are built so that th_i + r_odom - th_j is exact in double."""
import functools
import math
from types import SimpleNamespace as NS

import mpmath as mp
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "numpy.longdouble is not the 80-bit extended format here"
MP_BITS = 256
U = 2.0 ** -53
NORMAL, POINT = 0, 1

# Measured on the CPU: worst |Jet oracle - reference| / (2**-53 magnitude) over the family's builders (the closed-form
# oracle, analytic=True, in brackets), and the K that follows: max(4, 4 * ratio rounded up to a power of two).
#   LIDAR rows, blocks_by_size (both kinds, all four shifts)   residuals 2.12 (1.61)   Jacobians 4.51 (3.50)
#   LIDAR rows, tile_edges                                     residuals 1.16 (1.29)   Jacobians 2.69 (2.69)
#   (the worst are the Jet's theta columns on the pose pair near the origin; 4 * 4.51 = 18.04 -> 32)
#   The oracle's 28 normal-equation numbers, its rows summed in longdouble, meet (K + n) as it stands on every block.
K_LIDAR = 32
#   point-to-line (segments)    values 0.33   Jacobians 0.76   -> the floor of 4
K_P2L = 4
#   odometry (odometry_edges)   residuals 1.56 (a wrapped angle beside +-pi carries an ulp of 4 * 2**-53 on a magnitude of
#   pi)   Jacobians 0   -> 8
K_ODOM = 8


def k_rule(ratio):
    """The K the measured ratio calls for."""
    return max(4, 2 ** math.ceil(math.log2(max(4.0 * ratio, 1e-300))))


def _mpf(x):
    return mp.mpf(float(x))


def _ld(x):
    """An mpf rounded to longdouble (two doubles carry 106 bits)."""
    hi = float(x)
    return LD(hi) + LD(float(x - hi))


def ratio(got, ref, mag):
    """Worst |got - ref| / (2**-53 mag) over the entries where ref is finite; an entry of magnitude zero must be equal
    (inf otherwise).  NaN in `got` where ref is finite counts as inf."""
    got, ref, mag = np.asarray(got, LD), np.asarray(ref, LD), np.asarray(mag, LD)
    assert got.shape == ref.shape == mag.shape, (got.shape, ref.shape, mag.shape)
    fin = np.isfinite(ref)
    if not fin.any():
        return 0.0
    err = np.abs(got[fin] - ref[fin])
    m = mag[fin]
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(m > 0, err / (LD(U) * np.where(m > 0, m, 1)), np.where(err == 0, LD(0), LD(np.inf)))
    q = np.where(np.isnan(q), LD(np.inf), q)
    return float(q.max())


# ------------------------------------------------------------------------------------------------ LIDAR functors
def lidar_consts(source_pose, target_pose, as_ld=True):
    """What a block's two poses determine, at MP_BITS bits: cos / sin of th_s - th_t, o = R(th_t)^T (t_s - t_t), cos / sin
    of th_t, and the magnitudes of the S2T entries and of o as the functor forms them."""
    with mp.workprec(MP_BITS):
        xs, ys, ths = map(_mpf, source_pose)
        xt, yt, tht = map(_mpf, target_pose)
        cs, ss, ct, st = mp.cos(ths), mp.sin(ths), mp.cos(tht), mp.sin(tht)
        k = dict(cd=ct * cs + st * ss, sd=ct * ss - st * cs, ct=ct, st=st,
                 ox=ct * (xs - xt) + st * (ys - yt), oy=-st * (xs - xt) + ct * (ys - yt),
                 mc=abs(ct * cs) + abs(st * ss), ms=abs(ct * ss) + abs(st * cs),
                 mox=abs(ct) * (abs(xs) + abs(xt)) + abs(st) * (abs(ys) + abs(yt)),
                 moy=abs(st) * (abs(xs) + abs(xt)) + abs(ct) * (abs(ys) + abs(yt)))
        return NS(**{n: _ld(v) if as_ld else v for n, v in k.items()})


def lidar_rows(kind, k, px, py, tx, ty, nsx, nsy, ntx, nty):
    """One block's rows from its constants: (r, mr, J, mJ) -- r[a], J[a][c] for residual a of the pair and column c of
    (x_s, y_s, th_s, x_t, y_t, th_t), magnitudes beside them.  Plain + - * abs, so it runs on longdouble arrays and on
    mpf scalars alike."""
    ux, uy = k.cd * px - k.sd * py, k.sd * px + k.cd * py
    qx, qy = ux + k.ox, uy + k.oy
    mux, muy = k.mc * abs(px) + k.ms * abs(py), k.ms * abs(px) + k.mc * abs(py)
    mqx, mqy = mux + k.mox, muy + k.moy
    act, ast = abs(k.ct), abs(k.st)
    dqx = (k.ct, k.st, -uy, -k.ct, -k.st, qy)       # d q_x / d (x_s, y_s, th_s, x_t, y_t, th_t)
    dqy = (-k.st, k.ct, ux, k.st, -k.ct, -qx)
    mdx = (act, ast, muy, act, ast, mqy)
    mdy = (ast, act, mux, ast, act, mqx)
    if kind == NORMAL:
        ex, ey, mex, mey = qx - tx, qy - ty, mqx + abs(tx), mqy + abs(ty)
        r = (ntx * ex + nty * ey, -(nsx * ex + nsy * ey))
        mr = (abs(ntx) * mex + abs(nty) * mey, abs(nsx) * mex + abs(nsy) * mey)
        J = ([ntx * a + nty * b for a, b in zip(dqx, dqy)], [-(nsx * a + nsy * b) for a, b in zip(dqx, dqy)])
        mJ = ([abs(ntx) * a + abs(nty) * b for a, b in zip(mdx, mdy)], [abs(nsx) * a + abs(nsy) * b for a, b in zip(mdx, mdy)])
    else:
        r, mr = (tx - qx, ty - qy), (abs(tx) + mqx, abs(ty) + mqy)
        J, mJ = ([-a for a in dqx], [-b for b in dqy]), (list(mdx), list(mdy))
    return r, mr, J, mJ


def _stack(n, rows):
    """rows[a][c] (arrays of n or scalars) -> (n, len(rows), len(rows[0])) longdouble."""
    return np.stack([np.stack([np.broadcast_to(np.asarray(v, LD), (n,)) for v in row], axis=1) for row in rows], axis=1)


_TRIU = np.triu_indices(6)


def normal_equations(r, J):
    """The 28 numbers of one block from (n, 2) residuals and (n, 2, 6) Jacobians: upper triangle of J^T J (row major),
    J^T r, r^T r -- whatever the dtype of the inputs."""
    JtJ = np.einsum("nap,naq->pq", J, J)
    return np.concatenate([JtJ[_TRIU], np.einsum("nap,na->p", J, r), [np.einsum("na,na->", r, r)]])


def lidar_reference(kind, corr, offsets, block_src, block_tgt, poses):
    """The whole batch.  res (2n,), js / jt (2n, 3) in the layout of nhip_resid_lidar_dev; m_* their magnitudes;
    ne, m_ne (n_blocks, 28) the normal-equation numbers and the sums of their terms' magnitudes.  All longdouble."""
    corr = np.asarray(corr, np.float32).reshape(-1, 8)
    n, nb = len(corr), len(block_src)
    out = NS(res=np.zeros(2 * n, LD), js=np.zeros((2 * n, 3), LD), jt=np.zeros((2 * n, 3), LD),
             ne=np.zeros((nb, 28), LD), m_ne=np.zeros((nb, 28), LD))
    out.m_res, out.m_js, out.m_jt = np.zeros_like(out.res), np.zeros_like(out.js), np.zeros_like(out.jt)
    for b in range(nb):
        o, e = int(offsets[b]), int(offsets[b + 1])
        if e == o:
            continue
        k = lidar_consts(poses[block_src[b]], poses[block_tgt[b]])
        r, mr, J, mJ = lidar_rows(kind, k, *[corr[o:e, c].astype(LD) for c in range(8)])
        r, mr, J, mJ = _stack(e - o, [r])[:, 0], _stack(e - o, [mr])[:, 0], _stack(e - o, J), _stack(e - o, mJ)
        out.res[2 * o:2 * e], out.m_res[2 * o:2 * e] = r.reshape(-1), mr.reshape(-1)
        out.js[2 * o:2 * e], out.jt[2 * o:2 * e] = J[:, :, :3].reshape(-1, 3), J[:, :, 3:].reshape(-1, 3)
        out.m_js[2 * o:2 * e], out.m_jt[2 * o:2 * e] = mJ[:, :, :3].reshape(-1, 3), mJ[:, :, 3:].reshape(-1, 3)
        out.ne[b], out.m_ne[b] = normal_equations(r, J), normal_equations(mr, mJ)
    return out


def lidar_functor_mp(kind, row, source_pose, target_pose):
    """The functor's own lines on ONE row in mpmath, as a function of the six pose parameters: A(target)^-1 A(source) as
    3 x 3 matrices, nothing simplified.  For the CPU test, which differentiates it numerically."""
    px, py, tx, ty, nsx, nsy, ntx, nty = map(_mpf, row)

    def A(x, y, th):
        return mp.matrix([[mp.cos(th), -mp.sin(th), x], [mp.sin(th), mp.cos(th), y], [0, 0, 1]])

    def f(xs, ys, ths, xt, yt, tht):
        q = mp.inverse(A(xt, yt, tht)) * A(xs, ys, ths) * mp.matrix([px, py, 1])
        if kind == NORMAL:
            return [ntx * (q[0] - tx) + nty * (q[1] - ty), nsx * (tx - q[0]) + nsy * (ty - q[1])]
        return [tx - q[0], ty - q[1]]
    return f, [_mpf(v) for v in list(source_pose) + list(target_pose)]


# ------------------------------------------------------------------------------------------------ point to line
def p2l_branch_double(seg, pts, pose, line_pose):
    """DistanceToLineSegment's branch as IEEE double takes it: slam_residuals.h:186-194 and slam_util.h:92-110 restated one
    operation at a time (products and sums rounded singly, left to right).  Returns (inside, nearer_end, sd < 0)."""
    seg, pts = np.asarray(seg, np.float32).astype(np.float64), np.asarray(pts, np.float32).reshape(-1, 2).astype(np.float64)
    x, y, th = (np.float64(v) for v in pose)
    lx, ly, lth = (np.float64(v) for v in line_pose)
    c, s, lc, ls = np.cos(th), np.sin(th), np.cos(lth), np.sin(lth)
    sx0, sy0 = lc * seg[0] - ls * seg[1] + lx, ls * seg[0] + lc * seg[1] + ly
    sx1, sy1 = lc * seg[2] - ls * seg[3] + lx, ls * seg[2] + lc * seg[3] + ly
    px, py = c * pts[:, 0] - s * pts[:, 1] + x, s * pts[:, 0] + c * pts[:, 1] + y
    with np.errstate(invalid="ignore", divide="ignore"):
        dx, dy = sx1 - sx0, sy1 - sy0
        nx, ny = -dy, dx
        ln = np.sqrt(nx * nx + ny * ny)
        nx, ny = nx / ln, ny / ln
        off = -(sx0 * nx + sy0 * ny)
        sd = nx * px + ny * py + off
        prx, pry = px - sd * nx, py - sd * ny

        def between(v, a, b):
            return ((v >= a) & (v <= b)) | ((v >= b) & (v <= a))
        inside = between(prx, sx0, sx1) & between(pry, sy0, sy1)
        ax, ay, bx, by = px - sx0, py - sy0, px - sx1, py - sy1
        nearer_end = np.sqrt(bx * bx + by * by) < np.sqrt(ax * ax + ay * ay)
        return inside, nearer_end, sd < 0.0


def p2l_reference(seg, pts, pose, line_pose):
    """One block.  res (n,), jp / jl (n, 3) longdouble with magnitudes m_res, m_jp, m_jl; `inside`, `nearer_end` (the
    double branch), `t` (projection parameter along the segment, exact arithmetic: 0 at the start, 1 at the end; NaN for a
    zero-length segment), `sd` and `d_end` (distance to the nearer end).
    Magnitudes: M = sum of the absolute coordinates and translations involved; values and theta columns M max(1, M / len),
    translation columns max(1, M / len); past the ends both carry max(1, M / d_end) more, the conditioning of the
    direction (P - S_k) / |P - S_k|.  A zero-length segment has no len to divide by: factor 1.
    Jacobians follow the Jet rules at the kinks: |sd| at sd = 0 differentiates as +sd; sqrt at 0 gives NaN."""
    seg = np.asarray(seg, np.float32).reshape(4)
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    n = len(pts)
    with mp.workprec(MP_BITS):
        x, y, th = map(_mpf, pose)
        lx, ly, lth = map(_mpf, line_pose)
        s0x, s0y, s1x, s1y = map(_mpf, seg)
        c, s, lc, ls = mp.cos(th), mp.sin(th), mp.cos(lth), mp.sin(lth)
        g0 = (lc * s0x - ls * s0y, ls * s0x + lc * s0y)               # R(l_th) s_0: S_0 - l_t
        g1 = (lc * s1x - ls * s1y, ls * s1x + lc * s1y)
        e = (lc * (s1x - s0x) - ls * (s1y - s0y), ls * (s1x - s0x) + lc * (s1y - s0y))   # S_1 - S_0
        w0 = (x - lx - g0[0], y - ly - g0[1])                          # t - S_0: P - S_0 = R(th) p + w0
        w1 = (x - lx - g1[0], y - ly - g1[1])
        ln = mp.sqrt(e[0] ** 2 + e[1] ** 2)
        M0 = float(sum(abs(v) for v in (x, y, lx, ly, s0x, s0y, s1x, s1y)))
        c, s, ln_f = _ld(c), _ld(s), float(ln)
        g0, g1, e, w0, w1 = ([_ld(v) for v in t] for t in (g0, g1, e, w0, w1))
        ln = _ld(ln)
    px, py = pts[:, 0].astype(LD), pts[:, 1].astype(LD)
    rx, ry = c * px - s * py, s * px + c * py
    ax, ay, bx, by = rx + w0[0], ry + w0[1], rx + w1[0], ry + w1[1]
    inside, nearer_end, _ = p2l_branch_double(seg, pts, pose, line_pose)
    with np.errstate(invalid="ignore", divide="ignore"):
        nx, ny = -e[1] / ln, e[0] / ln
        sd = nx * ax + ny * ay
        t = (ax * e[0] + ay * e[1]) / (ln * ln)
        sg = np.where(sd < 0, LD(-1), LD(1))
        vx, vy = np.where(nearer_end, bx, ax), np.where(nearer_end, by, ay)
        gx, gy = (np.where(nearer_end, g1[k], g0[k]) for k in (0, 1))
        d_end = np.sqrt(vx * vx + vy * vy)
        hx, hy = vx / d_end, vy / d_end
        res = np.where(inside, np.abs(sd), d_end)
        # columns: x, y, th of the pose; x, y, th of the line pose
        j_in = [sg * nx, sg * ny, sg * (-nx * ry + ny * rx), -sg * nx, -sg * ny,
                sg * ((-ny * ax + nx * ay) - (-nx * g0[1] + ny * g0[0]))]
        j_end = [hx, hy, -hx * ry + hy * rx, -hx, -hy, -(-hx * gy + hy * gx)]
        J = np.stack([np.where(inside, a, b) for a, b in zip(j_in, j_end)], axis=1)
        M = M0 + np.abs(px) + np.abs(py)
        f = np.maximum(1, M / ln) if ln_f > 0 else np.ones(n, LD)
        f = np.where(inside, f, f * np.maximum(1, M / np.where(d_end > 0, d_end, 1)))
    m_col = np.stack([f, f, M * f, f, f, M * f], axis=1)
    return NS(res=res, m_res=M * f, jp=J[:, :3], jl=J[:, 3:], m_jp=m_col[:, :3], m_jl=m_col[:, 3:],
              inside=inside, nearer_end=nearer_end, t=t, sd=sd, d_end=d_end, len=ln_f)


def p2l_functor_mp(seg, pt, pose, line_pose, inside, nearer_end):
    """The functor's own lines on ONE point in mpmath as a function of the six parameters, on the branch given."""
    s0x, s0y, s1x, s1y = map(_mpf, seg)
    px, py = map(_mpf, pt)

    def f(x, y, th, lx, ly, lth):
        S0 = (mp.cos(lth) * s0x - mp.sin(lth) * s0y + lx, mp.sin(lth) * s0x + mp.cos(lth) * s0y + ly)
        S1 = (mp.cos(lth) * s1x - mp.sin(lth) * s1y + lx, mp.sin(lth) * s1x + mp.cos(lth) * s1y + ly)
        P = (mp.cos(th) * px - mp.sin(th) * py + x, mp.sin(th) * px + mp.cos(th) * py + y)
        if inside:
            ln = mp.sqrt((S1[0] - S0[0]) ** 2 + (S1[1] - S0[1]) ** 2)
            nx, ny = -(S1[1] - S0[1]) / ln, (S1[0] - S0[0]) / ln
            return abs(nx * P[0] + ny * P[1] - (S0[0] * nx + S0[1] * ny))
        E = S1 if nearer_end else S0
        return mp.sqrt((P[0] - E[0]) ** 2 + (P[1] - E[1]) ** 2)
    return f, [_mpf(v) for v in list(pose) + list(line_pose)]


# ------------------------------------------------------------------------------------------------ odometry
def odometry_reference(t_odom, r_odom, tw, rw, pose_i, pose_j):
    """n factors: res (n, 3), ji / jj (n, 3, 3) longdouble, magnitudes m_res, m_ji (= m_jj), `d` the exact rotation
    difference and `w` its wrap into (-pi, pi] (float)."""
    t_odom = np.asarray(t_odom, np.float32).reshape(-1, 2)
    r_odom = np.asarray(r_odom, np.float32).reshape(-1)
    pi_, pj_ = np.asarray(pose_i, np.float64).reshape(-1, 3), np.asarray(pose_j, np.float64).reshape(-1, 3)
    n = len(r_odom)
    res, m_res = np.zeros((n, 3), LD), np.zeros((n, 3), LD)
    d, w = np.zeros(n), np.zeros(n)
    with mp.workprec(MP_BITS):
        for f in range(n):
            for k in range(2):
                res[f, k] = _ld(_mpf(tw) * (_mpf(pi_[f, k]) + _mpf(t_odom[f, k]) - _mpf(pj_[f, k])))
                m_res[f, k] = LD(abs(tw)) * (LD(abs(pi_[f, k])) + LD(abs(float(t_odom[f, k]))) + LD(abs(pj_[f, k])))
            dd = _mpf(pi_[f, 2]) + _mpf(r_odom[f]) - _mpf(pj_[f, 2])
            ww = dd - 2 * mp.pi * mp.ceil(dd / (2 * mp.pi) - mp.mpf(1) / 2)     # into (-pi, pi]
            res[f, 2] = _ld(_mpf(rw) * ww)
            m_res[f, 2] = LD(abs(rw)) * (LD(abs(pi_[f, 2])) + LD(abs(float(r_odom[f]))) + LD(abs(pj_[f, 2])))
            d[f], w[f] = float(dd), float(ww)
    ji = np.zeros((n, 3, 3), LD)
    ji[:, 0, 0] = ji[:, 1, 1] = LD(tw)
    ji[:, 2, 2] = LD(rw)
    return NS(res=res, m_res=m_res, ji=ji, jj=-ji, m_ji=np.abs(ji), d=d, w=w)


# ------------------------------------------------------------------------------------------------ inputs
BLOCK_SIZES = (0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1279, 1280, 1281, 2560, 2561, 3000)
PI_ = math.pi - 1e-9
# pose pairs (source, target): near the origin; one pose twice; +-(pi - 1e-9) about 250 m out; 1e4 m out at 1000.3 rad
PAIR_POSES = np.array([[0.3, -0.2, 0.1], [-0.1, 0.4, -0.25],
                       [12.5, -7.25, 2.1], [12.5, -7.25, 2.1],
                       [100.0, -250.0, PI_], [-80.0, 40.0, -PI_],
                       [8000.0, -6000.0, 1000.3], [8000.3, -5999.6, 1000.32]])


def _rows_for_pair(rng, n, source_pose, target_pose):
    """n correspondences of a block: source points O(1) to O(10) m, the target point within centimetres of the
    transformed source point (the residual is the small difference of two larger numbers), unit normals."""
    k = lidar_consts(source_pose, target_pose)
    p = (rng.uniform(-1, 1, (n, 2)) * rng.choice([1.0, 10.0], (n, 1))).astype(np.float32)
    px, py = p[:, 0].astype(LD), p[:, 1].astype(LD)
    q = np.stack([k.cd * px - k.sd * py + k.ox, k.sd * px + k.cd * py + k.oy], axis=1).astype(np.float64)
    t = (q + rng.normal(0, 0.03, (n, 2))).astype(np.float32)
    a = rng.uniform(0, 2 * math.pi, (n, 2))
    ns = np.stack([np.cos(a[:, 0]), np.sin(a[:, 0])], axis=1).astype(np.float32)
    nt = np.stack([np.cos(a[:, 1]), np.sin(a[:, 1])], axis=1).astype(np.float32)
    return np.concatenate([p, t, ns, nt], axis=1)


@functools.lru_cache(maxsize=None)
def blocks_by_size(kind, shift=0):
    """One batch with a block of every size of BLOCK_SIZES in shuffled order; block b sits on pose pair (b + shift) % 4,
    so the four shifts put every size on every pair.  -> NS(corr, offsets, corr_block, src, tgt, poses, sizes)"""
    rng = np.random.default_rng(1000 + 10 * kind + shift)
    sizes = np.array(BLOCK_SIZES)[rng.permutation(len(BLOCK_SIZES))]
    z = int(np.flatnonzero(sizes == 0)[0])
    if z in (0, len(sizes) - 1):                              # the empty block sits between full ones
        sizes[[z, 7]] = sizes[[7, z]]
    pair = (np.arange(len(sizes)) + shift) % 4
    src, tgt = (2 * pair).astype(np.int32), (2 * pair + 1).astype(np.int32)
    corr = np.concatenate([_rows_for_pair(rng, int(n), PAIR_POSES[s], PAIR_POSES[t]) for n, s, t in zip(sizes, src, tgt)])
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    assert 0 < int(np.flatnonzero(sizes == 0)[0]) < len(sizes) - 1
    assert sorted(sizes) == sorted(BLOCK_SIZES) and len(corr) == sum(BLOCK_SIZES) == 13308
    assert np.abs(corr[:, :2]).max() <= 10 and np.abs(np.hypot(corr[:, 4], corr[:, 5]) - 1).max() < 1e-6
    assert np.abs(np.hypot(corr[:, 6], corr[:, 7]) - 1).max() < 1e-6
    assert np.array_equal(PAIR_POSES[2], PAIR_POSES[3]) and abs(np.hypot(*PAIR_POSES[6, :2]) - 1e4) < 1e-6
    assert abs(np.hypot(*(PAIR_POSES[7, :2] - PAIR_POSES[6, :2])) - 0.5) < 1e-9
    corr.setflags(write=False)
    return NS(corr=corr, offsets=offsets, corr_block=np.repeat(np.arange(len(sizes), dtype=np.int32), sizes),
              src=src, tgt=tgt, poses=PAIR_POSES, sizes=sizes)


@functools.lru_cache(maxsize=None)
def blocks_reference(kind, shift=0):
    b = blocks_by_size(kind, shift)
    return lidar_reference(kind, b.corr, b.offsets, b.src, b.tgt, b.poses)


TILE_EDGE_N = (1, 255, 256, 257, 511, 512, 513)
TILE_POSES = np.array([[0.2, -0.1, 0.3], [1.0, 2.0, -2.9], [-3.0, 0.5, 1.57], [25.0, -40.0, 7.0]])


@functools.lru_cache(maxsize=None)
def tile_edges():
    """n_corr on and beside the multiples of the kernel's 256-row tile, each spread over three blocks (sizes n // 3,
    n // 3, the rest: the single row has two empty blocks before it)."""
    rng = np.random.default_rng(77)
    out = []
    for n in TILE_EDGE_N:
        sizes = np.array([n // 3, n // 3, n - 2 * (n // 3)])
        src, tgt = np.array([0, 1, 3], np.int32), np.array([1, 2, 0], np.int32)
        corr = np.concatenate([_rows_for_pair(rng, int(k), TILE_POSES[s], TILE_POSES[t]) for k, s, t in zip(sizes, src, tgt)])
        assert len(corr) == n
        corr.setflags(write=False)
        out.append(NS(n=n, corr=corr, offsets=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32),
                      corr_block=np.repeat(np.arange(3, dtype=np.int32), sizes), src=src, tgt=tgt, poses=TILE_POSES, sizes=sizes))
    assert [c.n for c in out] == list(TILE_EDGE_N)
    return out


@functools.lru_cache(maxsize=None)
def tile_reference(kind, i):
    c = tile_edges()[i]
    return lidar_reference(kind, c.corr, c.offsets, c.src, c.tgt, c.poses)


AXIS_SEGMENTS = ([-1, 3, 4, 3], [2, -2, 2, 5], [1e3, -5, 1e3, 5])
MARGIN = 1e-9       # distance kept from every branch boundary where the branch is not pinned by exact arithmetic


@functools.lru_cache(maxsize=None)
def segments():
    """Blocks for PointToLineResidual, one per (segment, pose, line pose): a list of NS(tag, seg, pts, pose, line, ref).
    tags: 'rotated' (general poses; segments well off the axes, every point MARGIN away from a boundary), 'axis'
    (axis-aligned segments at headings of exactly 0, where the IsBetween quirk decides), 'exact' (small-integer poses, points
    exactly on the line and on the ends), 'zero' (zero-length segments)."""
    rng = np.random.default_rng(2024)
    cases = []

    def add(tag, seg, pts, pose, line):
        seg, pts = np.asarray(seg, np.float32), np.asarray(pts, np.float32).reshape(-1, 2)
        pose, line = np.asarray(pose, np.float64), np.asarray(line, np.float64)
        cases.append(NS(tag=tag, seg=seg, pts=pts, pose=pose, line=line, ref=p2l_reference(seg, pts, pose, line)))
        return cases[-1]

    poses = [[0.2, -0.1, 0.3], [1.0, 2.0, -2.9], [-3.0, 0.5, 1.57]]
    lines = [[0.0, 0.0, 0.0], [0.1, -0.2, 0.05], [-0.5, 0.3, -0.4]]
    for i, seg in enumerate([[0, 0, 2, 2], [0.5, 0.5, -3, 1], [-2, 1, 3, -1.5], [0, 0, 2, 2]]):
        c = add("rotated", seg, rng.uniform(-6, 6, (300, 2)), poses[i % 3], lines[(2 * i + 1) % 3])
        r = c.ref
        lth = c.line[2]
        dx = math.cos(lth) * (c.seg[2] - c.seg[0]) - math.sin(lth) * (c.seg[3] - c.seg[1])
        dy = math.sin(lth) * (c.seg[2] - c.seg[0]) + math.cos(lth) * (c.seg[3] - c.seg[1])
        assert min(abs(dx), abs(dy)) >= 1e-3 * r.len
        t = r.t.astype(np.float64)
        assert np.array_equal(r.inside, (t >= 0) & (t <= 1)), "double branch differs from the exact one"
        assert np.minimum(np.abs(t), np.abs(t - 1)).min() * r.len > MARGIN and np.abs(r.sd).min() > MARGIN
        assert np.array_equal(r.nearer_end[~r.inside], t[~r.inside] > 1) and r.d_end.min() > MARGIN
    for seg in AXIS_SEGMENTS:
        mid = np.array([(seg[0] + seg[2]) / 2, (seg[1] + seg[3]) / 2])
        add("axis", seg, mid + rng.uniform(-6, 6, (400, 2)) - [0.1, -0.2], [0.1, -0.2, 0.0], [0.05, 0.3, 0.0])
    # exact arithmetic: pose (2, -1, 0), line pose (1, 1, 0); local point = world point - (2, -1)
    w = np.array([[2, 4], [0.5, 4], [4.75, 4], [7, 4], [-3, 4], [0, 4], [5, 4], [2, 6], [2, 1.5], [6, 5], [-1, 3]], np.float64)
    add("exact", [-1, 3, 4, 3], w - [2, -1], [2, -1, 0], [1, 1, 0])            # world segment (0, 4) - (5, 4)
    w = np.array([[3, 1], [3, 4], [3, 6.5], [3, -3], [3, 9], [3, -1], [3, 6], [5, 2], [0.5, 3], [4, 8], [2, -2]], np.float64)
    add("exact", [2, -2, 2, 5], w - [2, -1], [2, -1, 0], [1, 1, 0])            # world segment (3, -1) - (3, 6)
    w = np.array([[1, 1], [0.5, 0.5], [4, 4], [-2, -2], [0, 0], [2, 2], [0, 2], [2, 0], [3, 1]], np.float64)
    add("exact", [0, 0, 2, 2], w, [0, 0, 0], [0, 0, 0])                        # the segment of the reference's own tests
    # zero-length segments: with the coincident point (exact arithmetic: world (2, 3)) and without
    add("zero", [1, 2, 1, 2], np.concatenate([[[0, 4]], rng.uniform(-4, 4, (40, 2))]), [2, -1, 0], [1, 1, 0])
    add("zero", [1, 2, 1, 2], rng.uniform(-4, 4, (40, 2)), [0.2, -0.1, 0.3], [0.1, -0.2, 0.05])

    def all_of(tag, field):
        return np.concatenate([np.asarray(getattr(c.ref, field)) for c in cases if c.tag == tag])
    ins, sd, end = all_of("rotated", "inside"), all_of("rotated", "sd"), all_of("rotated", "nearer_end")
    for name, cnt in (("inside, sd > 0", (ins & (sd > 0)).sum()), ("inside, sd < 0", (ins & (sd < 0)).sum()),
                      ("nearer start", (~ins & ~end).sum()), ("nearer end", (~ins & end).sum())):
        assert cnt >= 20, name
    # the quirk: points whose projection lies inside an axis-aligned segment in exact arithmetic, both outcomes
    t, ins = all_of("axis", "t").astype(np.float64), all_of("axis", "inside")
    proj_in = (t > 0) & (t < 1)
    assert not ins[~proj_in].any()
    assert (ins & proj_in).sum() >= 20 and (~ins & proj_in).sum() >= 20, ((ins & proj_in).sum(), (~ins & proj_in).sum())
    # exact: on the line inside (sd == 0, residual 0) and beyond; on each end
    for c in cases:
        if c.tag == "exact":
            r, t = c.ref, c.ref.t.astype(np.float64)
            on = r.sd == 0
            assert (on & (t > 0) & (t < 1)).sum() >= 2 and (on & (t > 1)).sum() >= 1 and (on & (t < 0)).sum() >= 1
            assert (on & (t == 0)).sum() == 1 and (on & (t == 1)).sum() == 1 and (~on).sum() >= 3
            assert np.all(r.res[on & (t >= 0) & (t <= 1)] == 0)
    z = [c for c in cases if c.tag == "zero"]
    assert all(c.ref.len == 0 and not c.ref.inside.any() for c in z)
    assert (z[0].ref.res == 0).sum() == 1 and z[0].ref.res[0] == 0 and (z[1].ref.res > 0).all()
    return cases


def segments_arrays():
    """segments() in the layout of nhip_resid_point_to_line: every case is a block with its own pose and line pose."""
    cs = segments()
    return NS(segs=np.stack([c.seg for c in cs]), pts=np.concatenate([c.pts for c in cs]),
              pblock=np.concatenate([np.full(len(c.pts), b, np.int32) for b, c in enumerate(cs)]),
              bpose=np.arange(len(cs), dtype=np.int32), bline=np.arange(len(cs), dtype=np.int32),
              poses=np.stack([c.pose for c in cs]), lines=np.stack([c.line for c in cs]))


ODOM_WEIGHTS = ((1.0, 2.5), (0.75, 3.0))


@functools.lru_cache(maxsize=None)
def odometry_edges():
    """Factors whose rotation difference d = th_i + r_odom - th_j sits on and beside the wrap, exact in double (so the side
    of the wrap is a fact, not a rounding), around th = 0 and th = 1e3; then 200 random factors kept MARGIN off the wrap.
    -> NS(t_odom, r_odom, pose_i, pose_j (n, 3 each), n_edge)"""
    rng = np.random.default_rng(5)
    pi, up, dn = math.pi, (lambda v: np.nextafter(v, np.inf)), (lambda v: np.nextafter(v, -np.inf))
    ds = [0.0, pi, -pi, 2 * pi, -2 * pi, up(pi), dn(pi), up(-pi), dn(-pi), pi + 1e-9, pi - 1e-9, -pi + 1e-9, -pi - 1e-9]
    rows = [(d, 0.0, 0.0) for d in ds]                                   # (th_i, r_odom, th_j), around 0
    for d in ds:                                                         # around 1e3: steps of th_i there are 1.1e-13
        thi = 1e3 + d
        rows += [(thi, 0.0, 1e3)] + ([(up(thi), 0.0, 1e3), (dn(thi), 0.0, 1e3)] if abs(abs(d) - pi) < 1e-12 else [])
        rows += [(-thi, 0.0, -1e3)]
    rows += [(0.0, float(np.float32(pi)), 0.0), (0.0, -float(np.float32(pi)), 0.0), (0.5, 2.5, -0.25), (1e3, 0.0, 1e3),
             (1e3, float(np.float32(pi)), 1e3)]
    n_edge = len(rows)
    th = np.array(rows)
    nr = 200
    th = np.concatenate([th, np.stack([rng.uniform(-7, 7, nr), rng.uniform(-3.2, 3.2, nr).astype(np.float32).astype(np.float64),
                                       rng.uniform(-7, 7, nr)], axis=1)])
    n = len(th)
    pose_i, pose_j = rng.normal(0, 3, (n, 3)), rng.normal(0, 3, (n, 3))
    pose_i[::7, :2] += 1e5
    pose_j[::7, :2] += 1e5
    pose_i[:, 2], pose_j[:, 2] = th[:, 0], th[:, 2]
    r_odom = th[:, 1].astype(np.float32)
    assert np.array_equal(r_odom.astype(np.float64), th[:, 1])
    t_odom = rng.normal(0, 0.3, (n, 2)).astype(np.float32)
    ref = odometry_reference(t_odom, r_odom, 1.0, 1.0, pose_i, pose_j)
    d_double = (pose_i[:, 2] + r_odom.astype(np.float64)) - pose_j[:, 2]
    assert np.array_equal(d_double[:n_edge], ref.d[:n_edge]), "an edge case's rotation difference is not exact in double"
    with mp.workprec(MP_BITS):
        for f in range(n_edge):
            assert _mpf(pose_i[f, 2]) + _mpf(r_odom[f]) - _mpf(pose_j[f, 2]) == _mpf(d_double[f])
    assert np.abs(np.abs(ref.w[n_edge:]) - pi).min() > MARGIN
    for v in (0.0, pi, -pi, 2 * pi, -2 * pi, up(pi), dn(pi), up(-pi), dn(-pi)):
        assert (d_double[:n_edge] == v).any(), v
    assert (ref.w[:n_edge] > 3.14).sum() >= 8 and (ref.w[:n_edge] < -3.14).sum() >= 8
    return NS(t_odom=t_odom, r_odom=r_odom, pose_i=pose_i, pose_j=pose_j, n_edge=n_edge)
