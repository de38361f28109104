"""The robust loss without a GPU ("Robust loss"): nautilus_amd/loss.py against the mpmath definition
(tests/loss_reference.py) within the derived bounds, the spec check of the C ABI, and the loop on the CPU backend with displaced
loop-closure records.  The GPU half: tests/test_loss_gpu.py, tests/test_loss_loop_gpu.py."""
import ctypes as C
import inspect

import mpmath as mp
import numpy as np
import pytest

from nautilus_amd import _lib
from tests import loss_loop as LL
from tests import loss_reference as LS


@pytest.mark.parametrize("a", LS.SCALES)
@pytest.mark.parametrize("kind", LS.KINDS)
def test_evaluate_meets_the_reference_on_the_case_list(kind, a):
    from nautilus_amd.loss import Loss
    s = LS.case_list(a)
    rho, rho1 = Loss(kind, a).evaluate(s)
    assert rho.dtype == np.float64 and rho.shape == rho1.shape == s.shape
    LS.check_values(kind, a, s, rho, rho1, np.sqrt(rho1), "numpy")
    wt = Loss(kind, a).weights(np.stack([np.sqrt(s), 0 * s, 0 * s], axis=1))
    assert wt.shape == (len(s), 4) and np.array_equal(wt[:, 3], np.sqrt(wt[:, 2]))
    if kind == "huber":  # the seam: the inlier branch at s == b and below (one ulp above, rho' is within an ulp of 1)
        b = a * a
        assert rho1[2] == 1.0 and rho1[3] == 1.0 and rho[2] == b and rho[3] == s[3] and rho1[4] <= 1.0


@pytest.mark.parametrize("kind", LS.KINDS)
def test_rho1_is_the_derivative_of_rho(kind):
    from nautilus_amd.loss import Loss
    for a in LS.SCALES:
        b = a * a
        s = np.array([1e-8 * b, 0.25 * b, 0.999 * b, 1.001 * b, 4.0 * b, 1e6 * b])  # (off huber's seam: rho' has a kink's neighbour there)
        _, rho1 = Loss(kind, a).evaluate(s)
        with mp.workprec(LS.MP_BITS):
            for v, got in zip(s.tolist(), rho1.tolist()):
                d = mp.diff(lambda t: LS.rho_mp(kind, a, t), mp.mpf(v), h=mp.mpf(v) * mp.mpf(2) ** -60)
                assert abs(d - LS.rho1_mp(kind, a, v)) <= mp.mpf(2) ** -40 * abs(d), (kind, a, v)
                assert abs(mp.mpf(got) - d) <= mp.mpf(2) ** -40 * abs(d), (kind, a, v, got)


def test_none_returns_its_inputs_bit_for_bit():
    from nautilus_amd.loss import Loss
    rng = np.random.default_rng(3)
    r, J = rng.normal(size=(37, 3)) * 10.0 ** rng.integers(-9, 9, (37, 1)), rng.normal(size=(37, 3, 6))
    J[:, 0, 1] = 0.0
    J[:, 1, 2] = -0.0
    r2, J2, rho = Loss("none", 0.5).rows(r, J)
    bits = lambda a: np.ascontiguousarray(a).view(np.int64)
    assert np.array_equal(bits(r2), bits(r)) and np.array_equal(bits(J2), bits(J))
    assert np.array_equal(bits(rho), bits(LS.squared_norm(r)))
    # a real loss: the rows are the reference's, from its own weights
    loss = Loss("cauchy", 0.37)
    r3, J3, rho3 = loss.rows(r, J)
    wt = loss.weights(r)
    assert np.array_equal(bits(wt[:, 0]), bits(LS.squared_norm(r))) and np.array_equal(bits(rho3), bits(wt[:, 1]))
    assert np.array_equal(bits(r3), bits(wt[:, 3:4] * r)) and np.array_equal(bits(J3), bits(wt[:, 3, None, None] * J))
    assert wt[:, 2].max() <= 1.0 and 0.0 < wt[:, 2].min() < 1e-3


def test_loss_arguments():
    from nautilus_amd.loss import Loss
    for bad in [("tukey", 1.0), ("cauchy", 0.0), ("huber", -1.0), ("soft_l1", float("inf")), ("cauchy", float("nan"))]:
        with pytest.raises(ValueError):
            Loss(*bad)
    assert Loss("none", 0.0).spec().kind == 0  # (none never reads its scale)
    spec = Loss("soft_l1", 0.37).spec()
    assert (spec.kind, spec.flags, spec.scale) == (_lib.NHIP_LOSS_SOFT_L1, 0, 0.37)


def test_abi_checks_the_spec_with_or_without_a_device():
    lib = _lib.load()
    assert C.sizeof(_lib.LossSpec) == 16
    f4, i4, f8 = np.zeros(8, np.float32), np.zeros(8, np.int32), np.zeros(64, np.float64)
    P = _lib.ptr

    def call(spec, n=0, n_poses=2, t=f4, out=f8, poses=f8, weights=None):
        rc = lib.nhip_resid_odometry_robust_normal_eq_dev(P(t), P(f4), P(i4), P(i4), n, 1.0, 1.0,
                                                          None if spec is None else C.byref(spec), P(poses), n_poses, P(out),
                                                          P(weights), None)
        return rc, lib.nhip_last_error().decode()

    S = _lib.LossSpec
    inf, nan = float("inf"), float("nan")
    bad = [(S(4, 0, 1.0), "kind"), (S(-1, 0, 1.0), "kind"), (S(3, 1, 1.0), "flags"), (S(0, 2, 1.0), "flags")]
    bad += [(S(k, 0, v), "scale") for k in (1, 2, 3) for v in (0.0, -1.0, inf, nan)]
    for spec, field in bad:
        rc, msg = call(spec)
        assert rc == _lib.NHIP_ERR_ARG and field in msg, (spec.kind, spec.flags, spec.scale, msg)
    good = S(3, 0, 1.0)
    for kw, word in [(dict(n=-1), "n_factors"), (dict(n_poses=-1), "n_poses"), (dict(t=None), "null"), (dict(out=None), "null"),
                     (dict(poses=None), "null")]:
        rc, msg = call(good, **kw)
        assert rc == _lib.NHIP_ERR_ARG and word in msg, (kw, msg)
    rc, msg = call(None)
    assert rc == _lib.NHIP_ERR_ARG and "loss" in msg
    # a valid call (no factors: nothing would be launched): no device is the only thing in its way
    want = _lib.NHIP_OK if _lib.device_count() > 0 else _lib.NHIP_ERR_NODEV
    for spec in (good, S(0, 0, nan), S(1, 0, 0.37)):  # (none never reads its scale)
        assert call(spec)[0] == want and call(spec, weights=f8)[0] == want
    assert not f8.any()


# ------------------------------------------------------------------------------------------------ the loop on the CPU backend
@pytest.fixture(scope="module")
def runs():
    from oracle.cpu_backend import OracleBackend
    return LL.five_runs(OracleBackend)


def test_the_loss_gives_back_what_displaced_closures_cost(runs):
    LL.check_loop_conditions(runs)


def test_usage_errors():
    import examples.slam_loop as loop
    from oracle.cpu_backend import OracleBackend
    assert {"lc_loss", "lc_loss_scale"} <= set(inspect.signature(loop.run).parameters)
    for bad in (dict(lc_loss="tukey"), dict(lc_loss="cauchy", lc_loss_scale=0), dict(lc_loss="huber", lc_loss_scale=float("nan"))):
        with pytest.raises(ValueError):
            loop.run(backend=OracleBackend(), **dict(LL.KW, **bad))
