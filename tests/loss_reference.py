"""The robust loss of DESIGN.md section 3 ("Robust loss") in high precision, the numpy row builder, and the inputs the loss is
tested on.  Written from the definition -- Ceres' HuberLoss, SoftLOneLoss, CauchyLoss over s = |r|^2 with scale a, b = a a --
not from nautilus_amd/loss.py and not from the kernel:

    none      rho = s                                         rho' = 1
    huber     s <= b: rho = s;  else 2 a sqrt(s) - b          s <= b: 1;  else a / sqrt(s)
    soft_l1   rho = 2 b (sqrt(1 + s/b) - 1)                   rho' = 1 / sqrt(1 + s/b)
    cauchy    rho = b log(1 + s/b)                            rho' = 1 / (1 + s/b)

a, b and s enter as the doubles the code under test holds (b = the double a * a, s the code's own s): the reference has no
input error, and everything after that runs in mpmath at MP_BITS bits, enough for 1 + s/b at the smallest subnormal s.

BOUNDS.  A value may differ from the reference by K * 2**-53 * |reference|.  K counts, in units of 2**-53 relative (half an ulp
at worst), what the operations of the definition's shortest stable evaluation can contribute, each error carried to the result by
the condition number of what follows it:
    a rounded +, -, *, /                                  1
    sqrt                                                  2   (a device library's root may be one ulp off, not half)
    log1p                                                 4   (two ulps: the accuracy device maths libraries document for it)
    through sqrt an incoming error halves; through 1 + x, q + 1 and log1p (condition x / ((1 + x) log1p x) <= 1) it does not grow;
    2 a, 2 s are exact.
  none, and huber at s <= b      values are the inputs and the constant 1: equal (K = 0)
  huber, s > b    rho = (2a) q - b, q = sqrt(s):  q 2, the product 3 -- on a magnitude (2a) q <= 2 rho (a q >= b up to a's own
                  rounding, so the difference is at least half the product): 6 -- the difference 7                       -> K 8
                  rho' = a / q: 2 + 1 = 3                                                                                -> K 4
                  sqrt(rho'): 3 / 2 + 2 = 3.5                                                                            -> K 4
  soft_l1         x = s / b 1; 1 + x 2; q = sqrt 1 + 2 = 3; q + 1 at most 3 + 1 = 4; rho = (2s) / (q + 1) 5              -> K 8
                  (the form sqrt(1 + x) - 1 = x / (sqrt(1 + x) + 1); the plain difference has no such bound near 0)
                  rho' = 1 / q: 3 + 1 = 4                                                                                -> K 4
                  sqrt(rho'): 4 / 2 + 2 = 4                                                                              -> K 4
  cauchy          x 1; log1p 1 + 4 = 5; rho = b log1p 6                                                                  -> K 8
                  (an evaluation may take the series' first term, s, where s/b < 2**-54: off by s/(2b) < 2**-55 relative, inside K)
                  1 + x 2; rho' = 1 / (1 + x) 3                                                                          -> K 4
                  sqrt(rho'): 3 / 2 + 2 = 3.5                                                                            -> K 4
Each K is the count rounded up to a power of two; none is taken from a device's output.  A reference of 0 (s = 0) must be met
exactly."""
import numpy as np
import mpmath as mp

MP_BITS = 2400  # (1 + s/b must hold the smallest subnormal, 2**-1074, beside 1 with bits to spare)
U = 2.0 ** -53
KINDS = ("none", "huber", "soft_l1", "cauchy")
SCALES = (1.0, 0.37)
K_RHO = {"none": 0, "huber": 8, "soft_l1": 8, "cauchy": 8}
K_RHO1 = {"none": 0, "huber": 4, "soft_l1": 4, "cauchy": 4}
K_SQRT_RHO1 = {"none": 0, "huber": 4, "soft_l1": 4, "cauchy": 4}


def _b(a):
    return float(np.float64(a) * np.float64(a))


def rho_mp(kind, a, s):
    """rho(s) as an mpf; a and s doubles (or mpf s, for the derivative)."""
    a, b, s = mp.mpf(float(a)), mp.mpf(_b(a)), mp.mpf(s)
    if kind == "none" or (kind == "huber" and s <= b):
        return s
    if kind == "huber":
        return 2 * a * mp.sqrt(s) - b
    if kind == "soft_l1":
        return 2 * b * (mp.sqrt(1 + s / b) - 1)
    assert kind == "cauchy", kind
    return b * mp.log(1 + s / b)


def rho1_mp(kind, a, s):
    a, b, s = mp.mpf(float(a)), mp.mpf(_b(a)), mp.mpf(s)
    if kind == "none" or (kind == "huber" and s <= b):
        return mp.mpf(1)
    if kind == "huber":
        return a / mp.sqrt(s)
    if kind == "soft_l1":
        return 1 / mp.sqrt(1 + s / b)
    assert kind == "cauchy", kind
    return 1 / (1 + s / b)


def reference(kind, a, s):
    """(rho, rho', sqrt(rho')) of every s as lists of mpf."""
    with mp.workprec(MP_BITS):
        rho = [rho_mp(kind, a, float(v)) for v in s]
        rho1 = [rho1_mp(kind, a, float(v)) for v in s]
        return rho, rho1, [mp.sqrt(v) for v in rho1]


def worst_ratio(got, ref):
    """Worst |got - ref| / (2**-53 |ref|) over the entries; an entry whose reference is 0 must be equal (inf otherwise)."""
    worst = 0.0
    with mp.workprec(MP_BITS):
        for g, r in zip(np.asarray(got, dtype=np.float64).tolist(), ref):
            err = abs(mp.mpf(g) - r) if np.isfinite(g) else mp.inf
            q = err / (mp.mpf(U) * abs(r)) if r != 0 else (mp.mpf(0) if err == 0 else mp.inf)
            worst = max(worst, float(q))
    return worst


def check_values(kind, a, s, rho, rho1, w, what=""):
    """Holds rho, rho' and sqrt(rho') at the squared norms s to the reference within the derived bounds; prints every ratio first."""
    ref = reference(kind, a, s)
    ratios = [worst_ratio(got, r) for got, r in zip((rho, rho1, w), ref)]
    print("LOSS %s %s a=%g: worst |got - ref| / (2^-53 |ref|): rho %.3g (K %d), rho' %.3g (K %d), sqrt(rho') %.3g (K %d)" % (
        what, kind, a, ratios[0], K_RHO[kind], ratios[1], K_RHO1[kind], ratios[2], K_SQRT_RHO1[kind]))
    assert ratios[0] <= K_RHO[kind] and ratios[1] <= K_RHO1[kind] and ratios[2] <= K_SQRT_RHO1[kind], (kind, a, ratios)
    return ratios


def case_list(a):
    """The squared norms every kind is held to at scale a: 0, the smallest subnormal, b and its two neighbours (huber's seam),
    1e-30 b and 1e-8 b (the small arguments of log1p and of sqrt(1 + x) - 1), 4 b, 1e12 b."""
    b = _b(a)
    return np.array([0.0, 5e-324, b, np.nextafter(b, 0.0), np.nextafter(b, np.inf), 1e-30 * b, 1e-8 * b, 4.0 * b, 1e12 * b])


def components(target):
    """(u, v) with fl(fl(u u) + fl(v v)) == target exactly, for residuals (u, v, 0): u is sqrt(target) cut to 26 bits, so u u is
    exact and target - u u is exact and below 2**-24 target; v is the root of that rest, whose rounded square misses it by far
    less than half an ulp of target."""
    target = float(target)
    if target == 0.0:
        return 0.0, 0.0
    root = np.sqrt(np.float64(target))
    m, e = np.frexp(root)
    u = float(np.ldexp(np.floor(np.ldexp(m, 26)), int(e) - 26))
    rest = target - u * u
    assert rest >= 0.0 and (u * u) + rest == target
    v = float(np.sqrt(np.float64(rest)))
    assert (u * u + v * v) + 0.0 * 0.0 == target, (target, u, v)
    return u, v


_IU = np.triu_indices(6)


def rows(r, ji, jj, w, rho):
    """The 28 doubles per factor of the reweighted factors, in numpy: r (F, 3), Jacobians (F, 3, 3) x 2, w = sqrt(rho') (F,) and
    rho (F,).  r~ = w r and J~ = w J, every entry one rounded product; every sum runs over the three residual rows, products
    rounded, added in row order 0, 1, 2; slot 27 is rho."""
    J = w[:, None, None] * np.concatenate([ji, jj], axis=2)
    r = w[:, None] * r
    out = np.zeros((len(r), 28))
    for k, (p, q) in enumerate(zip(*_IU)):
        out[:, k] = (J[:, 0, p] * J[:, 0, q] + J[:, 1, p] * J[:, 1, q]) + J[:, 2, p] * J[:, 2, q]
    for p in range(6):
        out[:, 21 + p] = (J[:, 0, p] * r[:, 0] + J[:, 1, p] * r[:, 1]) + J[:, 2, p] * r[:, 2]
    out[:, 27] = rho
    return out


def squared_norm(r):
    """s of (F, 3) residuals: products rounded, added in the order 0, 1, 2."""
    return (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
