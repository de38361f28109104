"""The relative-pose kernels on the GPU through the C ABI ("Relative-pose factors"; nautilus_amd/csrc/
nhip_relpose.hip): nhip_resid_relpose_dev's r and J and nhip_resid_relpose_normal_eq_dev's rows, weights and flags bit for bit
against the host form on the kernel's own cos, sin and atan2 (hostside.relpose_rows(trig=...)) and against the sums formed on the
host from the plain call's r and J, for every loss, at the workgroup's seams and on the case list (tests/relpose_reference.py);
those cos, sin and atan2 against mpmath; pose ids out of range; the optional outputs.  The CPU half: tests/test_relpose_cpu.py."""
import ctypes as C
import math

import numpy as np
import pytest

from nautilus_amd import _lib, hostside
from nautilus_amd.loss import Loss
from tests import loss_reference as LS
from tests import relpose_reference as RP

pytestmark = pytest.mark.gpu

SENTINEL, PAD = -7.25, 256
COUNTS = [1, 255, 256, 257, 513]  # the partial last workgroup and the staged span's seams
STORES = ["staged", "direct"]
bits = RP.bits


@pytest.fixture(params=STORES)
def store(request, monkeypatch):
    """Both forms of the row store (the test process runs with NHIP_TUNABLES=1: tests/conftest.py); "staged" ships."""
    monkeypatch.setenv("NHIP_RELPOSE_STORE", request.param)
    return request.param


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _status():
    info = (C.c_int32 * 4)()
    return _lib.load().nhip_dev_status(_stream(), info), list(info)


def _guarded(n, per, dtype=None):
    import torch
    dtype = torch.float64 if dtype is None else dtype
    return torch.full((per * n + PAD,), SENTINEL if dtype == torch.float64 else -7, dtype=dtype, device="cuda:0")


def _inputs(case):
    import torch
    n = len(case["pose_i"])
    z = lambda a, dt: _dev(a) if len(a) else torch.zeros(8, dtype=dt, device="cuda:0")
    return (z(case["z"], torch.float64), z(case["info"], torch.float64), z(case["pose_i"], torch.int32), z(case["pose_j"], torch.int32),
            _dev(case["poses"]), n)


def plain(case):
    """nhip_resid_relpose_dev: (r (n, 3), J_i (n, 3, 3), J_j (n, 3, 3), parts (n, 8), flags (n,)), the sentinels behind each checked."""
    import torch
    d_z, d_l, d_i, d_j, d_p, n = _inputs(case)
    outs = [_guarded(n, 3), _guarded(n, 9), _guarded(n, 9), _guarded(n, 8), _guarded(n, 1, torch.int32)]
    _lib.check(_lib.load().nhip_resid_relpose_dev(d_z.data_ptr(), d_l.data_ptr(), d_i.data_ptr(), d_j.data_ptr(), n, d_p.data_ptr(),
                                                  len(case["poses"]), *(o.data_ptr() for o in outs), _stream()))
    host = [o.cpu().numpy() for o in outs]
    for h, per in zip(host, (3, 9, 9, 8, 1)):
        assert np.all(h[per * n:] == (SENTINEL if h.dtype == np.float64 else -7)), "the sentinels behind every output"
    return (host[0][:3 * n].reshape(n, 3), host[1][:9 * n].reshape(n, 3, 3), host[2][:9 * n].reshape(n, 3, 3),
            host[3][:8 * n].reshape(n, 8), host[4][:n])


def rows_of(case, spec, weights=True, flags=True):
    """nhip_resid_relpose_normal_eq_dev: the raw (28 n + PAD,), (4 n + PAD,) or None, (n + PAD,) or None."""
    import torch
    d_z, d_l, d_i, d_j, d_p, n = _inputs(case)
    d_out = _guarded(n, 28)
    d_w = _guarded(n, 4) if weights else None
    d_f = _guarded(n, 1, torch.int32) if flags else None
    _lib.check(_lib.load().nhip_resid_relpose_normal_eq_dev(
        d_z.data_ptr(), d_l.data_ptr(), d_i.data_ptr(), d_j.data_ptr(), n, None if spec is None else C.byref(spec), d_p.data_ptr(),
        len(case["poses"]), d_out.data_ptr(), d_w.data_ptr() if weights else None, d_f.data_ptr() if flags else None, _stream()))
    return d_out.cpu().numpy(), d_w.cpu().numpy() if weights else None, d_f.cpu().numpy() if flags else None


def trig_of(parts):
    return parts[:, 0], parts[:, 1], parts[:, 2], parts[:, 3], parts[:, 6]


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("kind", RP.KINDS)
def test_rows_are_bit_equal_to_the_host_form_on_the_kernels_own_trig(gpu, store, kind, n):
    case = RP.case(n)
    loss = Loss(kind, RP.SCALE_OF[kind])
    r, ji, jj, parts, fl = plain(case)
    out, wt, fl2 = rows_of(case, loss.spec())
    assert _status()[0] == _lib.NHIP_OK
    assert np.all(out[28 * n:] == SENTINEL) and np.all(wt[4 * n:] == SENTINEL) and np.all(fl2[n:] == -7), "the sentinels behind the outputs"
    rows, wt4, fl2 = out[:28 * n].reshape(n, 28), wt[:4 * n].reshape(n, 4), fl2[:n]
    assert np.array_equal(fl, case["flags"]) and np.array_equal(fl2, case["flags"])
    assert np.all(parts[:, 7] == 0.0)
    # the plain call against the host form on its own trig
    hr, hji, hjj, hrows, hwt, hfl = hostside.relpose_rows(case["z"], case["info"], case["pose_i"], case["pose_j"], case["poses"],
                                                          loss=loss, trig=trig_of(parts))
    assert np.array_equal(hfl, fl)
    assert np.array_equal(bits(r), bits(hr)) and np.array_equal(bits(ji), bits(hji)) and np.array_equal(bits(jj), bits(hjj))
    assert np.array_equal(bits(parts[:, 4:6]), bits(np.where((fl == 0)[:, None], RP.evaluate_errors(case, trig_of(parts)), 0.0)))
    # the rows against the sums formed on the host from the plain call's own r and J (tests/test_loss_gpu.py's pattern)
    own = LS.rows(r, ji, jj, wt4[:, 3], wt4[:, 1])
    assert np.array_equal(bits(rows[:, :27]), bits(own[:, :27]))
    assert np.array_equal(bits(rows[:, 27]), bits(wt4[:, 1])), "slot 27 is the kernel's own rho"
    assert np.array_equal(bits(wt4[:, 0]), bits(LS.squared_norm(r))), "s is the sum of the kernel's own r"
    # ... and against the host form
    agree = bits(hwt) == bits(wt4)
    print("device == host form bit for bit: s %d, rho %d, rho' %d, sqrt(rho') %d of %d; rows %d of %d"
          % (*agree.sum(axis=0), n, (bits(hrows) == bits(rows)).all(axis=1).sum(), n))
    assert np.array_equal(bits(rows[:, :27]), bits(hrows[:, :27]))
    assert agree[:, [0, 2, 3]].all(), "s, rho' and sqrt(rho')"  # (rho and slot 27: test_rho_is_bit_equal_to_the_host_form)
    if kind != "none":  # rho, rho' and sqrt(rho') against the definition in mpmath within the loss' derived bounds (K18's check)
        LS.check_values(kind, loss.scale, wt4[~(fl != 0), 0], wt4[~(fl != 0), 1], wt4[~(fl != 0), 2], wt4[~(fl != 0), 3],
                        "device relpose n=%d %s" % (n, store))
    flagged = fl != 0
    assert not rows[flagged].any() and not wt4[flagged].any() and not r[flagged].any() and not parts[flagged].any()
    if kind == "none":
        assert np.all(wt4[~flagged, 2:] == 1.0) and np.array_equal(bits(wt4[:, 1]), bits(wt4[:, 0]))
        null, null_wt, _ = rows_of(case, None)
        assert np.array_equal(bits(null), bits(out)) and np.array_equal(bits(null_wt), bits(wt)), "a NULL loss is NONE"
    elif n >= 255:
        assert wt4[~flagged, 2].min() < 0.5 < wt4[~flagged, 2].max() <= 1.0, "inliers and outliers"
    # two runs give the same bytes; the optional outputs change nothing else
    again, again_wt, again_fl = rows_of(case, loss.spec())
    assert np.array_equal(bits(again), bits(out)) and np.array_equal(bits(again_wt), bits(wt)) and np.array_equal(again_fl[:n], fl2)
    bare, _, _ = rows_of(case, loss.spec(), weights=False, flags=False)
    no_w, _, f3 = rows_of(case, loss.spec(), weights=False)
    no_f, w3, _ = rows_of(case, loss.spec(), flags=False)
    assert all(np.array_equal(bits(x), bits(out)) for x in (bare, no_w, no_f))
    assert np.array_equal(bits(w3), bits(wt)) and np.array_equal(f3[:n], fl2)
    assert _status()[0] == _lib.NHIP_OK


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("kind", RP.KINDS)
def test_rho_is_bit_equal_to_the_host_form(gpu, kind, n):
    """The weights' rho and slot 27 against hostside.relpose_rows on the kernel's own trig, bit for bit, for every loss kind.
    NONE, HUBER and SOFT_L1 are products, quotients and square roots.  CAUCHY's rho = b log1p(s / b): with the device library's
    log1p on one side and numpy's on the other this test failed at 255, 256, 257 and 513 factors -- 6, 6, 7 and 16 values one
    ulp apart, each side within 1.3 ulp of mpmath, neither the closer one throughout -- which is why the relative-pose rows take
    log1p_pinned, fdlibm's log1p in IEEE operations, on the device and on the host (nhip_loss_shared.h, nautilus_amd/loss.py)."""
    import mpmath as mp
    case = RP.case(n)
    loss = Loss(kind, RP.SCALE_OF[kind])
    _, _, _, parts, fl = plain(case)
    out, wt, _ = rows_of(case, loss.spec())
    rows, wt4 = out[:28 * n].reshape(n, 28), wt[:4 * n].reshape(n, 4)
    host = hostside.relpose_rows(case["z"], case["info"], case["pose_i"], case["pose_j"], case["poses"], loss=loss, trig=trig_of(parts))
    off = np.nonzero(bits(wt4[:, 1]) != bits(host[4][:, 1]))[0]
    if len(off):  # each side's distance from b log1p(s / b) in mpmath at the code's own s, in ulp of rho
        mp.mp.prec = 200
        b = mp.mpf(loss.scale * loss.scale)
        for f in off:
            want = b * mp.log1p(mp.mpf(float(wt4[f, 0])) / b) if kind == "cauchy" else mp.mpf(float(host[4][f, 1]))
            ulp = math.ulp(float(want))
            print("rho of factor %d (%s): device %r, host %r; from mpmath in ulp: device %.3f, host %.3f"
                  % (f, case["names"][f], wt4[f, 1], host[4][f, 1], float((mp.mpf(float(wt4[f, 1])) - want) / ulp),
                     float((mp.mpf(float(host[4][f, 1])) - want) / ulp)))
    print("rho: %d of %d differ from the host form (%s, n = %d)" % (len(off), n, kind, n))
    assert np.array_equal(bits(rows[:, 27]), bits(wt4[:, 1]))
    assert np.array_equal(bits(wt4[:, 1]), bits(host[4][:, 1])), "rho"
    assert np.array_equal(bits(rows[:, 27]), bits(host[3][:, 27])), "slot 27"


def test_device_trig_against_mpmath(gpu):
    """c_a, s_a, c_b, s_b and e_theta of the case list against mpmath at the kernel's inputs: absolute deviation <= 2^-40 -- a
    sanity gate (a wrong angle, sign or frame shows at 1e-3 and beyond), with the measured worst deviation in ulp printed.
    e_theta is an angle: its deviation is taken modulo 2 pi (at a difference of +-pi the sign of a rounded s_e picks the side)."""
    import mpmath as mp
    case = RP.case(96, flagged=False)
    _, _, _, parts, fl = plain(case)
    assert not fl.any()
    want = RP.trig_reference(case["poses"], case["pose_i"], case["pose_j"], case["z"])
    got = np.stack(trig_of(parts), axis=1)
    worst_abs, worst_ulp = np.zeros(5), np.zeros(5)
    for f in range(len(got)):
        for k in range(5):
            d = abs(mp.mpf(float(got[f, k])) - want[f, k])
            if k == 4:
                d = min(d, abs(d - 2 * mp.pi))
            # (in ulp of the value for the cosines and sines; e_theta, whose exact value may be 1e-17 where the rounded one is
            # 0, in ulp of 1 -- its error is that of s_e and c_e, which are of size 1)
            ulp = 2.0 ** -52 if k == 4 or float(want[f, k]) == 0.0 else math.ulp(float(want[f, k]))
            worst_abs[k], worst_ulp[k] = max(worst_abs[k], float(d)), max(worst_ulp[k], float(d / ulp))
    print("device trig against mpmath: worst |deviation| c_a %.3g s_a %.3g c_b %.3g s_b %.3g e_theta %.3g; in ulp of the value "
          "%.2f %.2f %.2f %.2f, e_theta in ulp of 1: %.2f" % (*worst_abs, *worst_ulp))
    assert worst_abs.max() <= 2.0 ** -40
    # the cut: pi and its neighbours come back as +-pi to that accuracy
    for name in ("difference pi", "pi, one ulp below", "pi, one ulp above", "difference -pi", "pi by the measurement"):
        assert abs(abs(parts[case["names"].index(name), 6]) - math.pi) <= 2.0 ** -40, name
    assert parts[case["names"].index("zero error"), 4:7].tolist() == [0.0, 0.0, 0.0]
    assert abs(parts[case["names"].index("equal headings"), 6] + 0.01) <= 2.0 ** -40


@pytest.mark.parametrize("lane", [0, 128, 255, 256])
def test_pose_ids_out_of_range_are_zeros_and_reported(gpu, store, lane):
    """At the first, a middle and the last lane of a full workgroup and in the partial one behind it: never dereferenced, zeros,
    kind 16 with the id and the factor, the neighbours' bytes unchanged."""
    n = 257
    case = RP.case(n)
    spec = Loss("cauchy", 3.0).spec()
    good, good_wt, good_fl = rows_of(case, spec)
    good_plain = plain(case)
    assert _status()[0] == _lib.NHIP_OK
    lane_ok = [f for f in range(n) if case["flags"][f] == 0]
    lane = min(lane_ok, key=lambda f: abs(f - lane)) if case["flags"][lane] else lane
    for which, bad in (("pose_i", -1), ("pose_j", RP.N_POSES), ("pose_j", 2 ** 31 - 1), ("pose_i", -2 ** 31)):
        hit = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in case.items()}
        hit[which][lane] = bad
        out, wt, fl = rows_of(hit, spec)
        rc, info = _status()
        assert rc == _lib.NHIP_ERR_ARG and info[0] & 16 and info[1] == 16 and info[2] == bad and info[3] == lane, (which, bad, info)
        keep = np.arange(n) != lane
        rows, wt4 = out[:28 * n].reshape(n, 28), wt[:4 * n].reshape(n, 4)
        assert not rows[lane].any() and not wt4[lane].any()
        assert np.array_equal(bits(rows[keep]), bits(good[:28 * n].reshape(n, 28)[keep]))
        assert np.array_equal(bits(wt4[keep]), bits(good_wt[:4 * n].reshape(n, 4)[keep]))
        assert np.array_equal(fl[:n][keep], good_fl[:n][keep])
        assert np.all(out[28 * n:] == SENTINEL) and np.all(wt[4 * n:] == SENTINEL) and _status()[0] == _lib.NHIP_OK
        got = plain(hit)
        rc, info = _status()
        assert rc == _lib.NHIP_ERR_ARG and info[1] == 16 and info[2] == bad and info[3] == lane
        for g, w in zip(got[:4], good_plain[:4]):
            assert not g[lane].any() and np.array_equal(bits(g[keep]), bits(w[keep]))


def test_no_factors_touch_nothing(gpu, store):
    case = {"poses": np.zeros((3, 3)), "pose_i": np.zeros(0, np.int32), "pose_j": np.zeros(0, np.int32), "z": np.zeros((0, 4)),
            "info": np.zeros((0, 6))}
    out, wt, fl = rows_of(case, Loss("huber", 1.0).spec())
    assert np.all(out == SENTINEL) and np.all(wt == SENTINEL) and np.all(fl == -7) and _status()[0] == _lib.NHIP_OK
    r, ji, jj, parts, fl = plain(case)
    assert len(r) == 0 and _status()[0] == _lib.NHIP_OK


def test_host_pointer_call_is_the_device_call(gpu):
    """nhip_resid_relpose on host arrays: the bytes of nhip_resid_relpose_dev; its optional outputs may be left out."""
    case = RP.case(70)
    n = 70
    want = plain(case)
    r, ji, jj, parts, fl = np.empty((n, 3)), np.empty((n, 3, 3)), np.empty((n, 3, 3)), np.empty((n, 8)), np.empty(n, np.int32)
    lib = _lib.load()
    args = (_lib.ptr(case["z"]), _lib.ptr(case["info"]), _lib.ptr(case["pose_i"]), _lib.ptr(case["pose_j"]), n, _lib.ptr(case["poses"]),
            len(case["poses"]))
    _lib.check(lib.nhip_resid_relpose(*args, _lib.ptr(r), _lib.ptr(ji), _lib.ptr(jj), _lib.ptr(parts), _lib.ptr(fl)))
    for g, w in zip((r, ji, jj, parts), want[:4]):
        assert np.array_equal(bits(g), bits(w))
    assert np.array_equal(fl, want[4])
    r2 = np.empty((n, 3))
    _lib.check(lib.nhip_resid_relpose(*args, _lib.ptr(r2), None, None, None, None))
    assert np.array_equal(bits(r2), bits(r))
