"""Relative-pose factors without a device ("Relative-pose factors"): the per-factor restatement
(tests/relpose_reference.py) and the vectorised host form (hostside.relpose_rows) agree bit for bit; the Jacobian is the
derivative of the error; the whitener recomposes the information; the error does not change under a common rigid motion of both
poses, where the world-frame factor's does; three wrong rules leave the reference; nhip_relpose_information equals its Python
mirror; the argument errors need no device; and the loop on the CPU backend closes tighter with the factor than without.
The GPU half: tests/test_relpose_gpu.py, tests/test_relpose_loop_gpu.py."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

from nautilus_amd import _lib, hostside, posegraph
from nautilus_amd.loss import Loss
from tests import loss_loop as LL
from tests import relpose_reference as RP

bits = RP.bits


def host_rows(case, kind="none", a=1.0, **kw):
    loss = None if kind is None else Loss(kind, a)
    return hostside.relpose_rows(case["z"], case["info"], case["pose_i"], case["pose_j"], case["poses"], loss=loss, **kw)


@pytest.mark.parametrize("kind", RP.KINDS)
def test_restatement_and_host_form_agree_bit_for_bit(kind):
    case = RP.case(96)
    assert len(set(case["names"][:len(RP.SPECIAL)])) == len(RP.SPECIAL), "every special case is on the list"
    a = RP.SCALE_OF[kind]
    r, J, rows, wt, fl = RP.evaluate(case, kind, a)
    hr, hji, hjj, hrows, hwt, hfl = host_rows(case, kind, a)
    assert np.array_equal(fl, case["flags"]) and np.array_equal(hfl, case["flags"])
    assert np.array_equal(bits(r), bits(hr)) and np.array_equal(bits(J[:, :, :3]), bits(hji)) and np.array_equal(bits(J[:, :, 3:]), bits(hjj))
    assert np.array_equal(bits(rows), bits(hrows)) and np.array_equal(bits(wt), bits(hwt))
    flagged = fl != 0
    assert flagged.sum() >= 10 and not hrows[flagged].any() and not hwt[flagged].any() and not hr[flagged].any()
    assert np.isfinite(hrows).all() and np.isfinite(hwt).all()
    if kind == "none":
        assert np.all(hwt[~flagged, 2:] == 1.0) and np.array_equal(bits(hwt[:, 0]), bits(hwt[:, 1]))
        none = host_rows(case, None)
        assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(none, (hr, hji, hjj, hrows, hwt)))
    else:
        assert hwt[~flagged, 2].min() < 0.5 < hwt[~flagged, 2].max() <= 1.0, "inliers and outliers"
    zero = case["names"].index("zero error")
    assert not hr[zero].any() and hji[zero].any()


def test_pinned_log1p_is_one_function_in_c_numpy_and_plain_floats():
    """CAUCHY's logarithm under the relative-pose rows: the library's host compilation of the kernel's text
    (nhip_loss_log1p_pinned), loss.log1p_pinned in numpy and the per-value restatement return the same doubles at the branch seams
    and on 4,000 drawn arguments, within 1 ulp of mpmath; inf and NaN pass through; a pinned Loss takes it and says so."""
    import mpmath as mp
    from nautilus_amd.loss import log1p_pinned
    x = RP.log1p_cases()
    got = log1p_pinned(x)
    ref = np.array([RP.log1p_pinned(float(v)) for v in x])
    c = np.full(len(x), -1.0)
    _lib.check(_lib.load().nhip_loss_log1p_pinned(_lib.ptr(x), len(x), _lib.ptr(c)))
    assert np.array_equal(bits(got), bits(ref)) and np.array_equal(bits(c), bits(ref))
    mp.mp.prec = 200
    worst = 0.0
    for v, g in zip(x, got):
        want = mp.log1p(mp.mpf(float(v)))
        if want != 0:
            worst = max(worst, abs(float((mp.mpf(float(g)) - want) / math.ulp(float(want)))))
    differ = float((bits(got) != bits(np.log1p(x))).mean())
    print("log1p_pinned: worst %.3f ulp from mpmath over %d arguments; numpy's log1p differs on %.1f %% of them" % (worst, len(x), 100 * differ))
    assert worst <= 1.0
    odd = np.array([np.inf, np.nan])
    c2 = np.zeros(2)
    _lib.check(_lib.load().nhip_loss_log1p_pinned(_lib.ptr(odd), 2, _lib.ptr(c2)))
    assert np.isinf(c2[0]) and np.isnan(c2[1]) and np.isinf(log1p_pinned(odd)[0]) and np.isnan(log1p_pinned(odd)[1])
    loss = Loss("cauchy", 3.0)
    pinned = loss.pinned()
    assert not loss.pinned_log1p and pinned.pinned_log1p and pinned.pinned() is pinned
    s = np.array([0.5, 7.0, 300.0])
    assert np.array_equal(bits(loss.pinned().evaluate(s)[0]), bits(9.0 * log1p_pinned(s / 9.0)))
    assert np.array_equal(bits(loss.evaluate(s)[0]), bits(9.0 * np.log1p(s / 9.0))), "the odometry-style factors keep numpy's"
    assert posegraph.RelativePoseFactors([0], [1], np.zeros((1, 4)), np.ones((1, 6)), loss=loss).loss.pinned_log1p


def test_pose_ids_out_of_range_are_zeros_on_the_host():
    case = RP.case(16, flagged=False)
    clean = host_rows(case, "cauchy", 3.0)
    for lane, bad in ((0, -1), (7, RP.N_POSES), (15, 2 ** 31 - 1)):
        case["pose_j"][lane] = bad
    got = host_rows(case, "cauchy", 3.0)
    keep = np.ones(16, dtype=bool)
    keep[[0, 7, 15]] = False
    for g, c in zip(got[:5], clean[:5]):
        assert not g[~keep].any() and np.array_equal(bits(g[keep]), bits(c[keep]))
    assert not got[5].any()
    ref = RP.evaluate(case, "cauchy", 3.0)
    assert np.array_equal(bits(ref[2]), bits(got[3]))


def test_jacobian_is_the_derivative_of_the_error():
    """E against central differences of e at h = 1e-6, |pose| <= 10: truncation h^2 |e'''| / 6 ~ 1e-12 |d|; rounding: the two
    evaluations each carry a few 2^-53 (|t| + |d|) <= 1e-14, over 2 h: a few 1e-9 at most (measured: 3.1e-9 with poses up to
    28 m apart) -- below the 1e-8 asserted, which a wrong entry misses by the size of the entry."""
    case = RP.case(40, special=False)
    h, worst = 1e-6, 0.0
    for f in range(40):
        pa, pb = (list(case["poses"][case[k][f]]) for k in ("pose_i", "pose_j"))
        z = list(case["z"][f])
        _, E, _ = RP.error(z, pa, pb)
        for p in range(6):
            hi, lo = [pa[:], pb[:]], [pa[:], pb[:]]
            hi[p // 3][p % 3] += h
            lo[p // 3][p % 3] -= h
            e_hi, e_lo = RP.error(z, *hi)[0], RP.error(z, *lo)[0]
            for k in range(3):
                worst = max(worst, abs((e_hi[k] - e_lo[k]) / (2 * h) - E[k][p]))
    print("Jacobian against central differences: worst deviation %.3g" % worst)
    assert worst <= 1e-8


def test_whitener_recomposes_the_information_and_the_rows_are_E_Lambda_E():
    """W^T W against Lambda within 8 * 2^-53 * ||Lambda||; slots 0..20 against the exact E^T Lambda E (rationals, of the E the
    factor forms) within the same relative bound times the 9 terms of the double sum over Lambda's entries, each scaled by its
    two entries of E (||E||^2)."""
    case = RP.case(64, flagged=False)
    r, J, rows, wt, fl = RP.evaluate(case)
    assert not fl.any()
    worst_w = worst_r = 0.0
    for f in range(64):
        L = [float(v) for v in case["info"][f]]
        W = np.array(RP.whitener(L))
        Lam = RP.info_matrix(L)
        exact = [[sum(Fraction(W[m][i]) * Fraction(W[m][j]) for m in range(3)) for j in range(3)] for i in range(3)]
        dev = max(abs(float(exact[i][j] - Fraction(Lam[i][j]))) for i in range(3) for j in range(3))
        worst_w = max(worst_w, dev / RP.recompose_bound(L))
        assert dev <= RP.recompose_bound(L), case["names"][f]
        pa, pb = (list(case["poses"][case[k][f]]) for k in ("pose_i", "pose_j"))
        _, E, _ = RP.error(list(case["z"][f]), pa, pb)
        EF, LF = [[Fraction(v) for v in row] for row in E], [[Fraction(v) for v in row] for row in Lam]
        e2 = float(sum(v * v for row in E for v in row))
        k = 0
        for p in range(6):
            for q in range(p, 6):
                want = sum(EF[m][p] * LF[m][n] * EF[n][q] for m in range(3) for n in range(3))
                dev = abs(float(Fraction(rows[f][k]) - want))
                worst_r = max(worst_r, dev / (RP.recompose_bound(L, 9) * e2))
                assert dev <= RP.recompose_bound(L, 9) * e2, (case["names"][f], p, q)
                k += 1
    print("W^T W - Lambda: worst %.3f of the bound; rows - E^T Lambda E: worst %.3f of the bound" % (worst_w, worst_r))


GAUGE_ANGLE = round(math.radians(20.0) * 2 ** 20) / 2 ** 20  # 20 degrees on a grid on which heading + angle is exact
GAUGE_SHIFT = (3.0, -1.0)


def _moved(pose):
    """The pose after the rigid motion, every coordinate rounded once (the motion itself in 200 bits)."""
    import mpmath as mp
    mp.mp.prec = 200
    c, s = mp.cos(mp.mpf(GAUGE_ANGLE)), mp.sin(mp.mpf(GAUGE_ANGLE))
    x, y = mp.mpf(pose[0]), mp.mpf(pose[1])
    th = pose[2] + GAUGE_ANGLE
    assert mp.mpf(th) == mp.mpf(pose[2]) + mp.mpf(GAUGE_ANGLE)
    return [float(c * x - s * y + GAUGE_SHIFT[0]), float(s * x + c * y + GAUGE_SHIFT[1]), th]


def test_error_is_invariant_under_a_rigid_motion_and_the_world_frame_factor_is_not():
    """Closures of a room (the two scans within 3.5 m of each other, |pose| <= 10, headings on a 2^-20 grid so that the moved
    heading is exact): a motion of 20 degrees and (3, -1) m applied to both poses changes e by at most 8 * 2^-53 * (1 + |t|).
    The world-frame factor made at the first poses (loop_closure_factors) changes by centimetres and more."""
    from oracle.cpu_backend import OracleBackend
    rng = np.random.default_rng(3)
    n = 32
    grid = lambda v: np.round(v * 2 ** 20) / 2 ** 20
    a = np.concatenate([rng.uniform(-10, 10, (n, 2)), grid(rng.uniform(-3, 3, (n, 1)))], axis=1)
    rel = np.concatenate([rng.uniform(-2.4, 2.4, (n, 2)), grid(rng.uniform(-0.5, 0.5, (n, 1)))], axis=1)
    rel[:, :2] += np.sign(rel[:, :2]) * 0.05
    b = np.array([posegraph.compose(a[k], rel[k]) for k in range(n)])
    b[:, 2] = grid(b[:, 2])
    noise = rng.normal(0, [0.02, 0.02, 0.005], (n, 3))
    worst = 0.0
    for k in range(n):
        z = [rel[k, 0] + noise[k, 0], rel[k, 1] + noise[k, 1], math.cos(rel[k, 2] + noise[k, 2]), math.sin(rel[k, 2] + noise[k, 2])]
        pa, pb = list(a[k]), list(b[k])
        ma, mb = _moved(pa), _moved(pb)
        e0, e1 = RP.error(z, pa, pb)[0], RP.error(z, ma, mb)[0]
        bound = max(RP.gauge_bound(pa, pb), RP.gauge_bound(ma, mb))
        dev = max(abs(x - y) for x, y in zip(e0, e1))
        worst = max(worst, dev / bound)
        assert dev <= bound, (k, dev, bound)
        # the host form, whitened by the identity, is the same error
        r0 = hostside.relpose_rows([z], [[1.0, 0.0, 0.0, 1.0, 0.0, 1.0]], [0], [1], [pa, pb])[0][0]
        assert np.array_equal(bits(r0), bits(e0))
    # the world-frame factor, made at the first poses with the same measurements, at unit weights: metres and radians
    poses0 = np.concatenate([a, b])
    moved = np.array([_moved(list(p)) for p in poses0])
    src, tgt = np.arange(n, 2 * n), np.arange(n)
    world = posegraph.loop_closure_factors(poses0, src, tgt, rel + noise, tw=1.0, rw=1.0)
    w0, _, _ = world.evaluate(OracleBackend(), poses0)
    w1, _, _ = world.evaluate(OracleBackend(), moved)
    change = np.linalg.norm((w1 - w0)[:, :2], axis=1)
    print("rigid motion: relative-pose error moves by at most %.3f of its bound; the world-frame residual by %.3f .. %.3f m"
          % (worst, change.min(), change.max()))
    assert change.min() >= 0.01 and change.max() >= 0.3
    # ... and the relative factors built by the graph's own constructor see the same invariance
    fac = posegraph.relative_pose_factors(src, tgt, rel + noise, np.tile([1.0, 0.0, 0.0, 1.0, 0.0, 1.0], (n, 1)))
    f0, _, _ = fac.evaluate(OracleBackend(), poses0)
    f1, _, _ = fac.evaluate(OracleBackend(), moved)
    assert np.abs(f1 - f0).max() <= 8.0 * RP.U * 20.0


@pytest.mark.parametrize("wrong", ["sign", "transpose", "swap"])
def test_a_wrong_rule_leaves_the_reference(wrong):
    """A flipped sign in d d_x / d theta_a, W transposed, and a and b exchanged each move rows of the case list off the host form:
    the byte comparison is a test of these choices."""
    case = RP.case(64)
    hrows = host_rows(case)[3]
    right = RP.evaluate(case)[2]
    off = RP.evaluate(case, wrong=wrong)[2]
    assert np.array_equal(bits(right), bits(hrows))
    moved = (bits(off) != bits(hrows)).any(axis=1)
    print("%s: %d of %d rows differ" % (wrong, moved.sum(), len(moved)))
    assert moved.sum() >= 20


def test_information_in_c_equals_the_python_mirror():
    lib = _lib.load()
    rng = np.random.default_rng(9)
    n = 24
    ref = np.zeros(n, dtype=hostside.REFINED_DTYPE)
    ref["info"] = rng.uniform(-50, 50, (n, 6))
    ref["info"][:, [0, 3]] = rng.uniform(140, 710, (n, 2))
    ref["info"][:, 5] = rng.uniform(7800, 25000, n)
    ref["flags"] = np.array([0, 32, 4, 8, 16, 1, 2, 36] * 3, dtype=np.uint32)
    ref["info"][ref["flags"] & ~np.uint32(32) != 0] = 0.0  # (a record that kept its lattice pose: zeros)
    want_mask = np.array([True, True, False, False, False, False, False, False] * 3)
    for sigma, w in ((1.0, (10.0, 10.0)), (0.01, (10.0, 7.0)), (3.7, (0.5, 2.0))):
        info, mask = np.full((n, 6), -1.0), np.full(n, 9, dtype=np.uint8)
        _lib.check(lib.nhip_relpose_information(_lib.ptr(ref), n, sigma, w[0], w[1], _lib.ptr(info), _lib.ptr(mask)))
        hinfo, hmask = hostside.relpose_information(ref, sigma_m=sigma, weights=w)
        assert np.array_equal(bits(info), bits(hinfo)) and np.array_equal(mask.astype(bool), hmask) and np.array_equal(hmask, want_mask)
        inv = 1.0 / (sigma * sigma)
        assert np.array_equal(bits(info[want_mask]), bits(ref["info"][want_mask] * inv))
        assert np.all(info[~want_mask] == [w[0] * w[0], 0.0, 0.0, w[0] * w[0], 0.0, w[1] * w[1]])
        # never refined: the weights everywhere; the mask may be left out
        none = np.full((n, 6), -1.0)
        _lib.check(lib.nhip_relpose_information(None, n, sigma, w[0], w[1], _lib.ptr(none), None))
        h2, m2 = hostside.relpose_information(None, n=n, sigma_m=sigma, weights=w)
        assert np.array_equal(bits(none), bits(h2)) and not m2.any() and np.all(none == info[2])
    for bad in (0.0, -1.0, math.nan, math.inf):
        assert lib.nhip_relpose_information(_lib.ptr(ref), n, bad, 10.0, 10.0, _lib.ptr(info), None) == _lib.NHIP_ERR_ARG
        assert b"sigma_m" in lib.nhip_last_error()
        with pytest.raises(ValueError):
            hostside.relpose_information(ref, sigma_m=bad)
    assert lib.nhip_relpose_information(_lib.ptr(ref), -1, 1.0, 10.0, 10.0, _lib.ptr(info), None) == _lib.NHIP_ERR_ARG
    assert lib.nhip_relpose_information(_lib.ptr(ref), n, 1.0, 10.0, 10.0, None, None) == _lib.NHIP_ERR_ARG


def test_argument_errors_come_back_without_a_device():
    """A bad loss spec, a negative size and a null required pointer are NHIP_ERR_ARG before the device is asked for."""
    lib = _lib.load()
    buf = np.zeros(64)
    idx = np.zeros(4, dtype=np.int32)
    p, q = _lib.ptr(buf), _lib.ptr(idx)
    ok_loss = Loss("cauchy", 1.0).spec()
    rows = lambda *, z=p, info=p, pi=q, pj=q, n=1, loss=C.byref(ok_loss), poses=p, n_poses=2, out=p: \
        lib.nhip_resid_relpose_normal_eq_dev(z, info, pi, pj, n, loss, poses, n_poses, out, None, None, None)
    for spec in (_lib.LossSpec(7, 0, 1.0), _lib.LossSpec(-1, 0, 1.0), _lib.LossSpec(1, 1, 1.0), _lib.LossSpec(1, 0, 0.0),
                 _lib.LossSpec(3, 0, math.nan), _lib.LossSpec(2, 0, math.inf)):
        assert rows(loss=C.byref(spec)) == _lib.NHIP_ERR_ARG and b"loss" in lib.nhip_last_error()
    for kw in (dict(n=-1), dict(n_poses=-1), dict(z=None), dict(info=None), dict(pi=None), dict(pj=None), dict(poses=None), dict(out=None)):
        assert rows(**kw) == _lib.NHIP_ERR_ARG, kw
    plain = lambda *, z=p, info=p, pi=q, pj=q, n=1, poses=p, n_poses=2, res=p: \
        lib.nhip_resid_relpose_dev(z, info, pi, pj, n, poses, n_poses, res, None, None, None, None, None)
    for kw in (dict(n=-1), dict(n_poses=-1), dict(z=None), dict(info=None), dict(pi=None), dict(pj=None), dict(poses=None), dict(res=None)):
        assert plain(**kw) == _lib.NHIP_ERR_ARG, kw
    host = lambda *, z=p, n=1, res=p, pj=q: lib.nhip_resid_relpose(z, p, q, pj, n, p, 2, res, None, None, None, None)
    assert host(n=-1) == host(z=None) == host(res=None) == _lib.NHIP_ERR_ARG
    assert host(pj=_lib.ptr(np.array([5], dtype=np.int32))) == _lib.NHIP_ERR_ARG and b"out of range" in lib.nhip_last_error()
    if _lib.device_count() == 0:  # with valid arguments the call refuses to compute: no fallback
        assert rows() == _lib.NHIP_ERR_NODEV and plain() == _lib.NHIP_ERR_NODEV


def test_factors_reject_a_pose_paired_with_itself():
    with pytest.raises(ValueError):
        posegraph.RelativePoseFactors([0, 3], [1, 3], np.zeros((2, 4)), np.ones((2, 6)))
    with pytest.raises(ValueError):
        posegraph.RelativePoseFactors([0, 3], [1, 2], np.zeros((2, 4)), np.ones((3, 6)))
    fac = posegraph.relative_pose_factors([4, 5], [1, 2], [[1.0, 2.0, 0.5], [0.0, 1.0, -0.25]], [[0.0] * 6, [4.0, 0.0, 0.0, 5.0, 0.0, 6.0]],
                                          weights=(10.0, 7.0))
    assert fac.n == 2 and fac.pose_i.tolist() == [1, 2] and fac.pose_j.tolist() == [4, 5], "pose_i is the target"
    assert fac.info.tolist() == [[100.0, 0.0, 0.0, 100.0, 0.0, 49.0], [4.0, 0.0, 0.0, 5.0, 0.0, 6.0]], "weights fill the all-zero rows"
    assert fac.z.tolist() == [[1.0, 2.0, math.cos(0.5), math.sin(0.5)], [0.0, 1.0, math.cos(-0.25), math.sin(-0.25)]]
    fac = posegraph.relative_pose_factors([4], [1], [[1.0, 2.0, 0.5]], [[1.0, 0.0, 0.0, 1.0, 0.0, 1.0]], rel_cs=[[0.8, 0.6]])
    assert fac.z.tolist() == [[1.0, 2.0, 0.8, 0.6]]


# ------------------------------------------------------------------------------------------------ the loop on the CPU backend
@pytest.fixture(scope="module")
def cpu_loops():
    import examples.slam_loop as loop
    from oracle.cpu_backend import OracleBackend
    run = lambda **kw: loop.run(backend=OracleBackend(), lc_refine="icp", **dict(LL.KW, **kw))
    return {(drift, factor): run(drift_th_deg=drift, lc_factor=factor) for drift in (0.3, 5.0) for factor in (None, "relative")}


def check_loop_ratios(runs):
    """What tests/test_relpose_loop_gpu.py holds on the device as well."""
    for drift, ratio in ((5.0, 0.5), (0.3, 1.25)):
        world, rel = runs[(drift, None)], runs[(drift, "relative")]
        print("drift %.1f deg: err_lc_m world %.5f, relative %.5f (%.2f x); %d closures, %d with their H, eigenvalues %.0f .. %.0f"
              % (drift, world["err_lc_m"], rel["err_lc_m"], rel["err_lc_m"] / world["err_lc_m"], rel["lc_accepted"],
                 rel["lc_info_from_icp"], rel["lc_info_eig_min"], rel["lc_info_eig_max"]))
        assert rel["err_lc_m"] <= ratio * world["err_lc_m"]
        assert rel["lc_info_from_icp"] == rel["lc_accepted"] == world["lc_accepted"] >= 20
        assert rel["lc_factor"] == "relative" and rel["lc_info_sigma_m"] == 1.0 and 0 < rel["lc_info_eig_min"] <= rel["lc_info_eig_max"]
        for k in world:  # the factor changes nothing in front of the closure solve
            if not k.endswith(LL.TIMING) and k not in ("err_lc_m",) + LL.SOLVER_COUNTS:
                assert rel[k] == world[k], k
        assert set(rel) - set(world) == {"lc_factor", "lc_info_from_icp", "lc_info_sigma_m", "lc_info_eig_min", "lc_info_eig_max"}


def test_loop_closes_tighter_with_relative_factors(cpu_loops):
    check_loop_ratios(cpu_loops)


def test_lc_factor_none_is_the_call_without_it(cpu_loops):
    import examples.slam_loop as loop
    from oracle.cpu_backend import OracleBackend
    plain = loop.run(backend=OracleBackend(), lc_refine="icp", drift_th_deg=0.3, **LL.KW)
    none = cpu_loops[(0.3, None)]
    assert set(none) == set(plain) and not [k for k in plain if k.startswith(("lc_factor", "lc_info"))]
    for k in plain:
        if not k.endswith(LL.TIMING):
            assert none[k] == plain[k], k


def test_relative_factors_without_refinement_take_the_weights_and_a_loss():
    import examples.slam_loop as loop
    from oracle.cpu_backend import OracleBackend
    out = loop.run(backend=OracleBackend(), lc_factor="relative", lc_loss="cauchy", lc_loss_scale=3.0, **LL.KW)
    assert out["lc_info_from_icp"] == 0 and out["lc_info_eig_min"] is None and out["lc_accepted"] >= 20
    assert len(out["lc_weights"]) == out["lc_accepted"] and 0.0 < out["lc_weight_min"] <= 1.0
    with pytest.raises(ValueError):
        loop.run(backend=OracleBackend(), lc_factor="sideways", **LL.KW)
