"""The float norm of the distance gates (nhip_common.h: float_norm / float_norm_root, read back through the instrument
nhip_round_norm_dev) against numpy's float32 chain fl(sqrt(fl(fl(dx * dx) + fl(dy * dy)))), as bit patterns.  numpy rounds
every float32 operation on its own and takes a correctly rounded root; the gates promise the reference's decisions bit for
bit, so the device function has to be the same function -- over every binade, not at a handful of thresholds."""
import ctypes as C

import numpy as np
import pytest

from nautilus_amd import _lib
from tests import threshold_edges as E

pytestmark = pytest.mark.gpu
F32 = np.float32


def _device(dx, dy=None):
    """d_out of nhip_round_norm_dev: the norm of (dx, dy), or with dy None the root of dx alone."""
    import torch
    dev = torch.device("cuda:0")
    d_dx = torch.from_numpy(np.ascontiguousarray(dx, F32)).to(dev)
    d_dy = None if dy is None else torch.from_numpy(np.ascontiguousarray(dy, F32)).to(dev)
    d_out = torch.full((len(dx),), -7.0, dtype=torch.float32, device=dev)
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.load().nhip_round_norm_dev(d_dx.data_ptr(), None if d_dy is None else d_dy.data_ptr(), len(dx),
                                               1 if dy is None else 0, d_out.data_ptr(), sp))
    return d_out.cpu().numpy()


def _want(dx, dy=None):
    with np.errstate(all="ignore"):
        d2 = np.asarray(dx, F32) if dy is None else E.chain_d2(dx, dy)
        return np.sqrt(d2).astype(F32)


def _compare(what, got, want, dx, dy=None):
    """Prints the share of outputs that differ (and a few of them) before asserting that none does.  NaN equals NaN."""
    nan = np.isnan(want)
    bad = np.where(nan, ~np.isnan(got), got.view(np.uint32) != want.view(np.uint32))
    print("%s: %d of %d outputs differ from the correctly rounded chain (%.4f %%)" % (what, bad.sum(), len(bad), 100.0 * bad.mean()))
    for i in np.nonzero(bad)[0][:6]:
        print("   dx %s dy %s: device %s (0x%08x), correctly rounded %s (0x%08x)" % (
            float(dx[i]).hex(), "-" if dy is None else float(dy[i]).hex(), float(got[i]).hex(), got.view(np.uint32)[i],
            float(want[i]).hex(), want.view(np.uint32)[i]))
    assert not bad.any(), "%s: %d of %d differ" % (what, bad.sum(), len(bad))


def _random_floats(rng, n, exp_lo=1, exp_hi=254, signed=True):
    """float32 with a uniformly random biased exponent in [exp_lo, exp_hi] and random mantissa bits."""
    bits = (rng.integers(exp_lo, exp_hi + 1, n, dtype=np.uint32) << np.uint32(23)) | rng.integers(0, 1 << 23, n, dtype=np.uint32)
    if signed:
        bits |= rng.integers(0, 2, n, dtype=np.uint32) << np.uint32(31)
    return bits.view(F32)


def test_root_is_correctly_rounded_in_every_binade(gpu):
    rng = np.random.default_rng(41)
    d2 = _random_floats(rng, 1 << 22, signed=False)
    assert len(np.unique(d2.view(np.uint32) >> 23)) == 254
    _compare("root, 2^22 inputs over the 254 normal binades", _device(d2), _want(d2), d2)


def test_norm_chain_is_correctly_rounded_in_every_binade(gpu):
    """dy within three binades of dx for half of the inputs (both squares count), anywhere for the rest."""
    rng = np.random.default_rng(43)
    n = 1 << 22
    dx = _random_floats(rng, n)
    ex = (dx.view(np.uint32) >> 23) & 0xff
    ey = np.where(np.arange(n) % 2 == 0, np.clip(ex.astype(np.int64) + rng.integers(-3, 4, n), 1, 254), rng.integers(1, 255, n))
    dy = ((ey.astype(np.uint32) << np.uint32(23)) | rng.integers(0, 1 << 23, n, dtype=np.uint32) |
          (rng.integers(0, 2, n, dtype=np.uint32) << np.uint32(31))).view(F32)
    want = _want(dx, dy)
    assert len(np.unique(ex)) == 254 and np.isinf(want).any() and (want == 0).any() and ((want > 0) & (want < 1e-19)).any()  # (overflow, underflow, denormal d2)
    assert all(((dx < 0) == a).any() and ((dy < 0) == a).any() for a in (True, False))
    _compare("norm, 2^22 inputs over the 254 normal binades", _device(dx, dy), want, dx, dy)


def test_denormals_and_special_values(gpu):
    rng = np.random.default_rng(47)
    den = np.concatenate([((np.uint32(1) << np.uint32(b)) | rng.integers(0, 1 << b, 64, dtype=np.uint32)).astype(np.uint32) for b in range(23)] +
                         [np.uint32(1) << np.arange(23, dtype=np.uint32), (np.uint32(1) << np.arange(1, 24, dtype=np.uint32)) - np.uint32(1)]).view(F32)
    fmax, fmin = np.finfo(F32).max, np.finfo(F32).tiny
    special = F32([0.0, -0.0, np.inf, -np.inf, np.nan, fmax, -fmax, fmin, -fmin, 1.0, -1.0, 4.0, 2.0, np.nextafter(F32(1), F32(2)),
                   np.nextafter(F32(1), F32(0)), np.nextafter(fmax, F32(0))])
    d2 = np.concatenate([den, -den[:8], special])
    want = _want(d2)
    assert np.signbit(want[len(den) + 8 + 1]) and want[len(den) + 8 + 1] == 0  # sqrt(-0) = -0
    _compare("root, every denormal binade and the special values", _device(d2), want, d2)
    # the chain: squares that are denormal, that underflow to 0, that overflow, and every special value in either place
    tiny = _random_floats(rng, 4096, exp_lo=40, exp_hi=70)       # 2^-87 .. 2^-57: squares from 0 through the denormals
    huge = _random_floats(rng, 1024, exp_lo=185, exp_hi=200)     # 2^58 .. 2^73: squares and sums up to and beyond the largest float
    a = np.concatenate([tiny, tiny, huge, huge, np.repeat(special, len(special)), den, den])
    b = np.concatenate([np.roll(tiny, 1), np.zeros_like(tiny), np.roll(huge, 1), np.zeros_like(huge), np.tile(special, len(special)),
                        np.roll(den, 3), np.full_like(den, 1e-19)])
    want = _want(a, b)
    with np.errstate(all="ignore"):
        d2 = E.chain_d2(a, b)
    assert ((d2 > 0) & (d2 < fmin)).sum() > 500 and np.isinf(d2).sum() > 500 and np.isnan(d2).any() and (d2 == 0).any()
    assert np.isinf(want[2 * len(tiny):2 * len(tiny) + len(huge)]).any() and np.isfinite(want[2 * len(tiny):2 * len(tiny) + len(huge)]).any()
    _compare("norm, denormal and overflowing squares, special values", _device(a, b), want, a, b)


def test_every_designed_threshold_edge_case(gpu):
    """Every d2 value and every offset tests/threshold_edges.py designs, over all its thresholds and the three comparisons
    (native resolution and the lattice's): the device root is lo where the correctly rounded root is lo, hi where hi."""
    d2, ox, oy, roots = [], [], [], []
    for T in E.thresholds():
        for op, kind in (("<", "f32"), ("<", "f64"), ("<=", "f64")):
            for q in (0.0, E.lattice_step(T)[1]):
                e = E.Edge(T, op, kind, quantum=q)
                d2.append(e.d2)
                roots.append(e.d2_root)
                ox.append(e.offsets[:, 0])
                oy.append(e.offsets[:, 1])
    d2, ox, oy, roots = (np.concatenate(v) for v in (d2, ox, oy, roots))
    assert np.array_equal(_want(d2), roots) and len(d2) > 128 * 6 * 3 and len(ox) > 128 * 6 * 12
    _compare("root, the designed d2 values", _device(d2), roots, d2)
    _compare("norm, the designed offsets", _device(ox, oy), _want(ox, oy), ox, oy)
