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
    """Loss(kind, scale): kind "none" | "huber" | "soft_l1" | "cauchy"; scale a > 0 and finite (unused by "none")."""

    def __init__(self, kind, scale=1.0):
        if kind not in KINDS:
            raise ValueError("Loss: kind %r (one of %s)" % (kind, ", ".join(repr(k) for k in KINDS)))
        scale = float(scale)
        if kind != "none" and not (math.isfinite(scale) and scale > 0.0):
            raise ValueError("Loss: scale %r must be finite and > 0" % (scale,))
        self.kind, self.scale = kind, scale

    def __repr__(self):
        return "Loss(%r, %r)" % (self.kind, self.scale)

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
                return np.where(x < 2.0 ** -54, s, b * np.log1p(x)), 1.0 / (1.0 + x)
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
