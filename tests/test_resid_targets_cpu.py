"""tests/resid_reference.py tied to the CPU oracle, without a GPU: the Jet<6> restatement of the four functors (and the
closed-form LIDAR oracle) lies within the reference's bounds on every input family -- this is where K of each family
is measured (run with -s to see the ratios) --, the reference's own error is below 1 % of those bounds against an
all-mpmath evaluation and against the functors' own lines differentiated numerically, the discontinuous cases come
out as the oracle takes them, and the builders' preconditions hold."""
import mpmath as mp
import numpy as np
import pytest

from oracle import oracle as O
from tests import resid_reference as RR

LD = RR.LD
KINDS = [RR.NORMAL, RR.POINT]


def _measure(what, K, **ratios):
    """Print the measured ratios; the family's K must be at least what the rule makes of the worst (resid_reference.py)."""
    worst = max(ratios.values())
    print("%-28s %s -> K rule %d, K %d" % (what, "  ".join("%s %.3g" % kv for kv in ratios.items()), RR.k_rule(worst), K))
    assert RR.k_rule(worst) <= K, (what, ratios)


def _ne_of_rows(batch, r, js, jt):
    """(n_blocks, 28) from a batch's rows in the API layout, accumulated in longdouble (the rows' error alone)."""
    out = np.zeros((len(batch.src), 28), LD)
    J = np.concatenate([js.reshape(-1, 2, 3), jt.reshape(-1, 2, 3)], axis=2).astype(LD)
    r = r.reshape(-1, 2).astype(LD)
    for b in range(len(batch.src)):
        o, e = batch.offsets[b], batch.offsets[b + 1]
        if e > o:
            out[b] = RR.normal_equations(r[o:e], J[o:e])
    return out


def _lidar_ratios(kind, batch, ref, analytic):
    """Ratios of the oracle's rows; its 28 numbers per block (rows summed in longdouble, so two row errors per term and no
    summation error) must meet the sum bound as it stands."""
    r, js, jt = O.lidar_batch(kind, batch.corr, batch.offsets, batch.src, batch.tgt, batch.poses, analytic=analytic)
    ne = _ne_of_rows(batch, r, js, jt)
    for b in range(len(batch.src)):
        n = int(batch.offsets[b + 1] - batch.offsets[b])
        assert RR.ratio(ne[b], ref.ne[b], ref.m_ne[b]) <= RR.K_LIDAR + n, (b, n)
    return dict(res=RR.ratio(r, ref.res, ref.m_res), jac=max(RR.ratio(js, ref.js, ref.m_js), RR.ratio(jt, ref.jt, ref.m_jt)))


@pytest.mark.parametrize("shift", range(4))
@pytest.mark.parametrize("kind", KINDS)
def test_lidar_oracles_within_bounds_on_blocks_by_size(kind, shift):
    batch, ref = RR.blocks_by_size(kind, shift), RR.blocks_reference(kind, shift)
    for analytic in (False, True):
        q = _lidar_ratios(kind, batch, ref, analytic)
        _measure("lidar kind %d shift %d %s" % (kind, shift, "closed form" if analytic else "Jet"), RR.K_LIDAR, **q)
    # block by block (oracle.lidar_block) it is the same function
    r, js, jt = O.lidar_batch(kind, batch.corr, batch.offsets, batch.src, batch.tgt, batch.poses)
    for b in np.flatnonzero(batch.sizes > 0)[:6]:
        c = batch.corr[batch.offsets[b]:batch.offsets[b + 1]]
        br, b0, b1 = O.lidar_block(kind, c[:, 0:2], c[:, 2:4], c[:, 4:6], c[:, 6:8], batch.poses[batch.src[b]], batch.poses[batch.tgt[b]])
        rows = slice(2 * batch.offsets[b], 2 * batch.offsets[b + 1])
        assert np.array_equal(br, r[rows]) and np.array_equal(b0, js[rows]) and np.array_equal(b1, jt[rows])
    z = int(np.flatnonzero(batch.sizes == 0)[0])
    assert not ref.ne[z].any() and not ref.m_ne[z].any()


@pytest.mark.parametrize("kind", KINDS)
def test_lidar_oracles_within_bounds_on_tile_edges(kind):
    for i, c in enumerate(RR.tile_edges()):
        for analytic in (False, True):
            q = _lidar_ratios(kind, c, RR.tile_reference(kind, i), analytic)
            _measure("tile n=%d kind %d %s" % (c.n, kind, "closed form" if analytic else "Jet"), RR.K_LIDAR, **q)


def _mp_rows(kind, batch, rows):
    """lidar_rows on mpf scalars with unrounded constants: (r, J) per row as nested lists of mpf."""
    out = []
    blk = np.searchsorted(batch.offsets, rows, side="right") - 1
    for i, b in zip(rows, blk):
        k = RR.lidar_consts(batch.poses[batch.src[b]], batch.poses[batch.tgt[b]], as_ld=False)
        r, _, J, _ = RR.lidar_rows(kind, k, *[mp.mpf(float(v)) for v in batch.corr[i]])
        out.append((r, J))
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_lidar_reference_own_error_is_below_one_percent_of_the_bounds(kind):
    worst = 0.0
    with mp.workprec(RR.MP_BITS):
        for shift in range(4):
            batch, ref = RR.blocks_by_size(kind, shift), RR.blocks_reference(kind, shift)
            rows = np.random.default_rng(shift).choice(len(batch.corr), 60, replace=False)
            for i, (r, J) in zip(rows, _mp_rows(kind, batch, rows)):
                for a in range(2):
                    want = [RR._ld(r[a])] + [RR._ld(v) for v in J[a]]
                    got = np.concatenate([[ref.res[2 * i + a]], ref.js[2 * i + a], ref.jt[2 * i + a]])
                    mag = np.concatenate([[ref.m_res[2 * i + a]], ref.m_js[2 * i + a], ref.m_jt[2 * i + a]])
                    worst = max(worst, RR.ratio(got, np.array(want, LD), mag))
        assert worst <= 0.01 * RR.K_LIDAR, worst
        # the 28 sums of whole blocks, all in mpmath: a short block, one wave, the longest (most additions)
        batch, ref = RR.blocks_by_size(kind, 3), RR.blocks_reference(kind, 3)
        for size in (2, 64, 3000):
            b = int(np.flatnonzero(batch.sizes == size)[0])
            acc = [mp.mpf(0)] * 28
            for r, J in _mp_rows(kind, batch, np.arange(batch.offsets[b], batch.offsets[b + 1])):
                k = 0
                for p in range(6):
                    for q in range(p, 6):
                        acc[k] += J[0][p] * J[0][q] + J[1][p] * J[1][q]
                        k += 1
                for p in range(6):
                    acc[21 + p] += J[0][p] * r[0] + J[1][p] * r[1]
                acc[27] += r[0] * r[0] + r[1] * r[1]
            got = RR.ratio(ref.ne[b], np.array([RR._ld(v) for v in acc], LD), ref.m_ne[b])
            assert got <= 0.01 * (RR.K_LIDAR + size), (size, got)
            worst = max(worst, got)
    print("lidar kind %d: reference against mpmath, worst ratio %.3g" % (kind, worst))


@pytest.mark.parametrize("kind", KINDS)
def test_lidar_reference_is_the_functor_and_its_derivative(kind):
    """A(target)^-1 A(source) p written out as matrices in mpmath and differentiated numerically, against the closed forms."""
    worst = 0.0
    with mp.workprec(RR.MP_BITS):
        for shift in range(4):
            batch, ref = RR.blocks_by_size(kind, shift), RR.blocks_reference(kind, shift)
            rows = np.random.default_rng(10 + shift).choice(len(batch.corr), 4, replace=False)
            for i in rows:
                b = int(np.searchsorted(batch.offsets, i, side="right") - 1)
                f, x = RR.lidar_functor_mp(kind, batch.corr[i], batch.poses[batch.src[b]], batch.poses[batch.tgt[b]])
                val = f(*x)
                for a in range(2):
                    want = [val[a]] + [mp.diff(lambda *p: f(*p)[a], tuple(x), tuple(int(c == j) for j in range(6))) for c in range(6)]
                    got = np.concatenate([[ref.res[2 * i + a]], ref.js[2 * i + a], ref.jt[2 * i + a]])
                    mag = np.concatenate([[ref.m_res[2 * i + a]], ref.m_js[2 * i + a], ref.m_jt[2 * i + a]])
                    worst = max(worst, RR.ratio(got, np.array([RR._ld(v) for v in want], LD), mag))
    assert worst <= 0.01 * RR.K_LIDAR, worst


def test_point_to_line_oracle_within_bounds_and_takes_the_same_branches():
    q_val = q_jac = 0.0
    for c in RR.segments():
        r = c.ref
        wr, w0, w1 = O.point_to_line_block(c.seg, c.pts, c.pose, c.line)
        # NaN exactly where the definition has none to give: the Jacobians of a distance of zero past the ends
        nan = ~r.inside & (r.res == 0)
        assert np.isfinite(wr).all() and np.array_equal(np.isnan(w0).any(axis=1), nan) and np.array_equal(np.isnan(w0).all(axis=1), nan)
        assert np.array_equal(np.isnan(w1).all(axis=1), nan) and np.array_equal(np.isnan(r.jp).all(axis=1), nan)
        assert np.array_equal(np.isnan(r.jl).any(axis=1), nan) and (c.tag in ("exact", "zero") or not nan.any())
        q_val = max(q_val, RR.ratio(wr, r.res, r.m_res))
        q_jac = max(q_jac, RR.ratio(w0, r.jp, r.m_jp), RR.ratio(w1, r.jl, r.m_jl))
        if c.tag == "axis":
            # the oracle's outcome point for point: which of |sd| and the end distance it returned
            sd, de = np.abs(r.sd).astype(np.float64), r.d_end.astype(np.float64)
            assert np.all(de - sd > 1e-6) or np.all((de - sd > 1e-6) | ~r.inside)
            took_inside = np.abs(wr - sd) < np.abs(wr - de)
            clear = de - sd > 1e-6
            assert np.array_equal(took_inside[clear], r.inside[clear]) and not r.inside[~clear].any()
    _measure("point to line", RR.K_P2L, val=q_val, jac=q_jac)


def test_point_to_line_reference_is_the_functor_and_its_derivative():
    worst = 0.0
    with mp.workprec(RR.MP_BITS):
        for ci, c in enumerate(RR.segments()):
            r = c.ref
            ok = np.flatnonzero(~(~r.inside & (r.res == 0)) & ((r.sd != 0) | ~r.inside))     # (not at a kink of the functor)
            for i in np.random.default_rng(ci).choice(ok, min(5, len(ok)), replace=False):
                f, x = RR.p2l_functor_mp(c.seg, c.pts[i], c.pose, c.line, bool(r.inside[i]), bool(r.nearer_end[i]))
                want = [f(*x)] + [mp.diff(f, tuple(x), tuple(int(k == j) for j in range(6))) for k in range(6)]
                got = np.concatenate([[r.res[i]], r.jp[i], r.jl[i]])
                mag = np.concatenate([[r.m_res[i]], r.m_jp[i], r.m_jl[i]])
                worst = max(worst, RR.ratio(got, np.array([RR._ld(v) for v in want], LD), mag))
    print("point to line: reference against mpmath, worst ratio %.3g" % worst)
    assert worst <= 0.01 * RR.K_P2L, worst


def test_odometry_oracle_within_bounds_and_wraps_to_the_same_side():
    e = RR.odometry_edges()
    n = len(e.r_odom)
    q_res = q_jac = 0.0
    for tw, rw in RR.ODOM_WEIGHTS:
        ref = RR.odometry_reference(e.t_odom, e.r_odom, tw, rw, e.pose_i, e.pose_j)
        for f in range(n):
            wr, w0, w1 = O.odometry_block(e.t_odom[f], e.r_odom[f], tw, rw, e.pose_i[f], e.pose_j[f])
            q_res = max(q_res, RR.ratio(wr, ref.res[f], ref.m_res[f]))
            q_jac = max(q_jac, RR.ratio(w0, ref.ji[f], ref.m_ji[f]), RR.ratio(w1, ref.jj[f], ref.m_ji[f]))
            if f < e.n_edge:
                assert np.sign(wr[2]) == np.sign(ref.w[f]) and (ref.w[f] != 0 or ref.d[f] == 0), (f, wr[2], ref.w[f])
    _measure("odometry", RR.K_ODOM, res=q_res, jac=q_jac)


def test_builders_hold_their_preconditions():
    for kind in KINDS:
        for shift in range(4):
            b = RR.blocks_by_size(kind, shift)
            assert set(zip(b.sizes.tolist(), ((np.arange(18) + shift) % 4).tolist())) == set(zip(b.sizes.tolist(), (b.src // 2).tolist()))
        # across the four shifts every size meets every pose pair
        seen = {(int(s), int(p)) for shift in range(4) for s, p in zip(RR.blocks_by_size(kind, shift).sizes, RR.blocks_by_size(kind, shift).src // 2)}
        assert len({p for s, p in seen if s == 3000}) >= 2
    assert [c.n for c in RR.tile_edges()] == [1, 255, 256, 257, 511, 512, 513]
    tags = [c.tag for c in RR.segments()]
    assert tags.count("axis") == 3 and tags.count("zero") == 2 and tags.count("exact") == 3 and tags.count("rotated") == 4
    for c in RR.segments():
        assert (c.tag != "axis" and c.tag != "exact") or (c.pose[2] == 0 and c.line[2] == 0)
        assert c.tag != "axis" or len(c.pts) == 400
    e = RR.odometry_edges()
    assert len(e.r_odom) == e.n_edge + 200 and RR.k_rule(0.0) == 4 and RR.k_rule(1.7) == 8 and RR.k_rule(2.0) == 8
