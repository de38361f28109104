"""Robust loss for odometry-style factors ("Robust loss"): Ceres' HuberLoss, SoftLOneLoss and CauchyLoss
over s = |r|^2, and the first-order correction Ceres' Corrector applies for a loss with rho'' <= 0 -- residual and Jacobian
scaled by w = sqrt(rho'(s)), the factor's cost rho(s) / 2.

numpy only.  This is the arithmetic of the kernel (nautilus_amd/csrc/nhip_loss.hip) in the kernel's operation order, so the
host linear path (PoseGraph._assemble_inner) and a backend without the kernel compute what the device path computes:

    s = r0 r0 + r1 r1 + r2 r2          products rounded, added in that order
    b = a a                            one rounded product; a is the scale, in units of the weighted residual
    none      rho = s                         rho' = 1
    huber     s <= b: rho = s, rho' = 1       else q = sqrt(s): rho = ((2 a) q) - b, rho' = a / q
    soft_l1   x = s / b, q = sqrt(1 + x):     rho = (2 s) / (q + 1), rho' = 1 / q
    cauchy    x = s / b:                      rho = s if x < 2^-54 else b log1p(x), rho' = 1 / (1 + x)
    w = sqrt(rho'),  r~ = w r,  J~ = w J      every entry one rounded product

soft_l1's rho is 2 b (sqrt(1 + x) - 1) with the difference written as x / (sqrt(1 + x) + 1); cauchy's logarithm is log1p, and
below x = 2^-54 its series' first term b x = s: the same functions as Ceres', without the cancellation near s = 0 and without
handing a subnormal quotient to the logarithm (build-defined)."""
import math

import numpy as np

from . import _lib

KINDS = {"none": _lib.NHIP_LOSS_NONE, "huber": _lib.NHIP_LOSS_HUBER, "soft_l1": _lib.NHIP_LOSS_SOFT_L1,
         "cauchy": _lib.NHIP_LOSS_CAUCHY}


class Loss:
    """Loss(kind, scale): kind "none" | "huber" | "soft_l1" | "cauchy"; scale a > 0 and finite (unused by "none").
    pinned_log1p: cauchy's logarithm is log1p_pinned (below) instead of numpy's -- what the relative-pose factors take, whose
    kernel does the same ("Relative-pose factors"); .pinned() returns such a copy."""

    def __init__(self, kind, scale=1.0, pinned_log1p=False):
        if kind not in KINDS:
            raise ValueError("Loss: kind %r (one of %s)" % (kind, ", ".join(repr(k) for k in KINDS)))
        scale = float(scale)
        if kind != "none" and not (math.isfinite(scale) and scale > 0.0):
            raise ValueError("Loss: scale %r must be finite and > 0" % (scale,))
        self.kind, self.scale, self.pinned_log1p = kind, scale, bool(pinned_log1p)

    def __repr__(self):
        return "Loss(%r, %r%s)" % (self.kind, self.scale, ", pinned_log1p=True" if self.pinned_log1p else "")

    def pinned(self):
        """This loss with cauchy's logarithm pinned (itself if it is already)."""
        return self if self.pinned_log1p else Loss(self.kind, self.scale, pinned_log1p=True)

    def spec(self):
        """The nhip_loss_spec_t of this loss."""
        return _lib.LossSpec(KINDS[self.kind], 0, self.scale)

    def evaluate(self, s):
        """(rho(s), rho'(s)) of an array of squared norms, float64."""
        s = np.asarray(s, dtype=np.float64)
        a = np.float64(self.scale)
        b = a * a
        with np.errstate(all="ignore"):
            if self.kind == "huber":
                inlier = s <= b
                q = np.sqrt(np.where(inlier, 1.0, s))
                return np.where(inlier, s, (2.0 * a) * q - b), np.where(inlier, 1.0, a / q)
            if self.kind == "soft_l1":
                q = np.sqrt(1.0 + s / b)
                return (2.0 * s) / (q + 1.0), 1.0 / q
            if self.kind == "cauchy":
                x = s / b
                return np.where(x < 2.0 ** -54, s, b * (log1p_pinned(x) if self.pinned_log1p else np.log1p(x))), 1.0 / (1.0 + x)
        return s.copy(), np.ones_like(s)

    def weights(self, r):
        """(F, 4) {s, rho, rho', sqrt(rho')} of the (F, 3) residuals r."""
        r = np.asarray(r, dtype=np.float64).reshape(-1, 3)
        s = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2]
        rho, rho1 = self.evaluate(s)
        return np.stack([s, rho, rho1, np.sqrt(rho1)], axis=1)

    def rows(self, r, J):
        """The reweighted factors: (r~ (F, 3), J~ (F, 3, C), rho (F,)) of residuals r (F, 3) and Jacobians J (F, 3, C)."""
        r, J = np.asarray(r, dtype=np.float64), np.asarray(J, dtype=np.float64)
        wt = self.weights(r)
        w = wt[:, 3]
        return w[:, None] * r, w[:, None, None] * J, wt[:, 1]


_LN2_HI, _LN2_LO = 6.93147180369123816490e-01, 1.90821492927058770002e-10
_LP = (6.666666666666735130e-01, 3.999999999940941908e-01, 2.857142874366239149e-01, 2.222219843214978396e-01,
       1.818357216161805012e-01, 1.531383769920937332e-01, 1.479819860511658591e-01)


def log1p_pinned(x):
    """log1p(x) for x >= 0 written out in IEEE operations: fdlibm's s_log1p.c, its branches for x >= 0, every sum, product and
    quotient rounded on its own -- the doubles nhip_loss_shared.h's log1p_pinned returns on the device, bit for bit, where numpy's
    and the device library's log1p differ from each other in the last bit on a few values in a hundred.  Error below 1 ulp.
    NaN, inf and anything not >= 0 give x + x."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    shape = x.shape
    x = x.reshape(-1)
    with np.errstate(all="ignore"):
        hx = x.view(np.int64) >> 32
        special = ~(x >= 0.0) | (hx >= 0x7ff00000)
        tiny, small, direct, big = hx < 0x3c900000, hx < 0x3e200000, hx < 0x3FDA827A, hx >= 0x43400000
        u = np.where(big, x, 1.0 + x)
        ub = u.view(np.int64)
        hu = ub >> 32
        k = (hu >> 20) - 1023
        c = np.where(big, 0.0, np.where(k > 0, 1.0 - (u - x), x - (u - 1.0)) / u)
        hu = hu & 0x000fffff
        low = hu < 0x6a09e
        un = ((np.where(low, hu | 0x3ff00000, hu | 0x3fe00000) << 32) | (ub & 0xffffffff)).view(np.float64)
        k = np.where(low, k, k + 1)
        hu = np.where(low, hu, (0x00100000 - hu) >> 2)
        f = np.where(direct, x, un - 1.0)
        k, hu, c = np.where(direct, 0, k), np.where(direct, 1, hu), np.where(direct, 0.0, c)
        hfsq, kd = 0.5 * f * f, k.astype(np.float64)
        R0 = hfsq * (1.0 - 0.66666666666666666 * f)
        near = np.where(f == 0.0, np.where(k == 0, 0.0, kd * _LN2_HI + (c + kd * _LN2_LO)),
                        np.where(k == 0, f - R0, kd * _LN2_HI - ((R0 - (kd * _LN2_LO + c)) - f)))
        s = f / (2.0 + f)
        z = s * s
        R = z * (_LP[0] + z * (_LP[1] + z * (_LP[2] + z * (_LP[3] + z * (_LP[4] + z * (_LP[5] + z * _LP[6]))))))
        far = np.where(k == 0, f - (hfsq - s * (hfsq + R)), kd * _LN2_HI - ((hfsq - (s * (hfsq + R) + (kd * _LN2_LO + c))) - f))
        out = np.where(hu == 0, near, far)
        out = np.where(small, np.where(tiny, x, x - x * x * 0.5), out)
        out = np.where(special, x + x, out)
    return out.reshape(shape)
