"""Points on the edges of POOLED entries through the branch-and-bound matcher, and bounds whose maximum sits where the
wave-wide reductions end.

The bounds phase needs only the pooled entry of a point's window origin, (floor(m) + K) >> 3 per coordinate (m: the
single-precision quotient v / res, K: the constant added after the clamp, nhip_bnb_origin.h window_origin<true>).  A quotient
that lies on or one float step beside an integer n takes the double-precision floor only where n + K is a multiple of
8 -- the one bucket in which n - 1 and n fall into different entries; in the other seven the lane keeps the float floor.
Here the scans hold such points for every residue of n + K, in x alone, in y alone and in both, next to points that
the clamp takes at either end, a NaN, an infinite coordinate and a quotient beyond 2^22.  The searched rotation is the
identity (theta0 = 0, middle of the lattice), so that xr == x and yr == y exactly.  The records must be the oracle's in
the fused form, the split form forced onto a small list and shared pairs, 8- and 16-bit cells.

Second part: the rotation order (the maximum of a rotation's bounds) and the seeds (a wave's best block) come out of
reductions over the 64 lanes; the optimum is placed in the last of 61 rotations, and in the block that lane 63 holds."""
import functools
import math
import os

import numpy as np
import pytest

from nautilus_amd import csm
from oracle import oracle as O

pytestmark = pytest.mark.gpu

DEG = math.radians(1.0)
RES = 0.05
RANGE = 6.0           # grid side 240 cells (<= 256)
MAX_SHIFT = 12
INV_F = np.float32(1.0 / RES)   # what the kernel multiplies by: RN_f32(1 / res)
FORMS = ({"NHIP_BNB_KERNELS": "1"}, {"NHIP_BNB_KERNELS": "1", "NHIP_BNB_SPLIT": "1"},
         {"NHIP_BNB_SPLIT": "1", "NHIP_BNB_SPLIT_BATCH": "2", "NHIP_BNB_SPLIT_MIN": "1"})


def _quot(v):
    """m = RN_f32(v * RN_f32(1 / res)), the kernel's single-precision quotient"""
    return np.float32(v) * INV_F


def _coord_for(n, side):
    """A float32 coordinate whose quotient is exactly n (side 0) or the float next below / above n (side -1 / +1); None
    when no float32 maps there."""
    want = np.float32(n) if side == 0 else np.nextafter(np.float32(n), np.float32(side * np.inf))
    v = np.float32(want / INV_F)
    for _ in range(4):
        v = np.nextafter(v, np.float32(-np.inf))
    for _ in range(9):
        if _quot(v) == want:
            return v
        v = np.nextafter(v, np.float32(np.inf))
    return None


def _generic(n):
    """a coordinate in the middle of cell n: far from every edge"""
    return np.float32((n + 0.4) * RES)


def _near(m):
    """the kernel's test: m within |m| * 2^-22 of an integer"""
    m = np.asarray(m, np.float32)
    r = m - np.floor(m)
    return ~(np.minimum(r, np.float32(1.0) - r) > np.abs(m) * np.float32(2.0 ** -22))


SIDES9 = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 0), (0, 1), (1, -1), (1, 0), (1, 1))


def _edge_scans():
    """[x edges, y edges, both, both + clamped / non-finite points]; 64 - 200 points each.  Every scan is an L: a run
    along x at y ~ 3.5 m and a run along y at x ~ -5 m, so that the identity is its one best rotation."""
    cells = range(-104, -80)   # 24 consecutive cells: every residue of n + K three times
    run = range(-60, 61, 3)
    sx, sb = [], []
    for i, n in enumerate(cells):
        for side in (-1, 0, 1):
            v = _coord_for(n, side)
            if v is not None:
                sx.append((v, _generic(70 + i % 7)))
    for j in run:
        v = _coord_for(-104 + j % 8, j % 3 - 1)
        if v is not None:
            sx.append((v, _generic(j)))
    sy = [(g, v) for v, g in sx]
    for i, n in enumerate(cells):
        for j, (s0, s1) in enumerate(SIDES9):
            a, b = _coord_for(n, s0), _coord_for(70 + (i + j) % 8, s1)   # (x and y in different residues, too)
            if a is not None and b is not None and (i + j) % 2 == 0:
                sb.append((a, b))
    for j in run:
        s0, s1 = SIDES9[(j // 3) % 9]
        a, b = _coord_for(-104 + j % 8, s0), _coord_for(j, s1)
        if a is not None and b is not None:
            sb.append((a, b))
    odd = [(1000.0, 0.5), (-1000.0, 0.5), (0.5, 1000.0), (0.5, -1000.0), (-1000.0, 1000.0),   # clamped at both ends
           (np.nan, 1.0), (2.0, np.inf),                                                      # not numbers
           (1.5 * 2.0 ** 22 * RES, 0.25), (0.25, -1.5 * 2.0 ** 22 * RES)]                     # |m| >= 2^22, finite
    so = sb[0::2][:40] + odd + sb[1::2][-50:]
    return [np.array(s, np.float32) for s in (sx, sy, sb, so)]


@functools.lru_cache(maxsize=None)
def _edge_case(cell_bits):
    """scans (the last one is the target), the oracle's records: computed once per cell width"""
    srcs = _edge_scans()
    # the target: the same walls (the three sources' points that lie inside the grid)
    tgt = np.concatenate([s[np.isfinite(s).all(axis=1) & (np.abs(s) < RANGE).all(axis=1)] for s in srcs[:3]])
    scans = srcs + [np.unique(tgt, axis=0)]
    xy, off = csm.pack_scans(scans)
    t = len(scans) - 1
    src, slot, th0 = np.arange(t, dtype=np.int32), np.zeros(t, np.int32), np.zeros(t, np.float64)
    ospec = O.grid_spec(RANGE, RES, 2.0, 1e-10, cell_bits)
    ogr = O.grid_build_batch(xy, off, [t], ospec)
    want = O.csm_match_batch(xy, off, ogr, ospec, src, slot, th0, O.search_spec(5, 17, 17, DEG))
    return scans, xy, off, src, slot, th0, want


def _classes(pts, kx, ky):
    """per point and coordinate: 0 not near, 1 near and released (n + K not a multiple of 8), 2 near and kept"""
    out = []
    for v, k in ((pts[:, 0], kx), (pts[:, 1], ky)):
        with np.errstate(invalid="ignore", over="ignore"):
            m = _quot(v)
            ok = np.isfinite(m) & (np.abs(m) < 2.0 ** 22)
            n = np.where(ok, np.rint(np.where(ok, m, 0)), 0).astype(np.int64)
            c = np.where(_near(np.where(ok, m, 0)), np.where((n + k) % 8 == 0, 2, 1), 0)
        out.append(np.where(ok, c, 3))   # 3: not a number or |m| >= 2^22 (always kept)
    return out[0], out[1]


def _match_every_form(st, grids, src, slot, th0, search):
    got, sums = csm.match_pairs(st, grids, src, slot, th0, search)
    for env in FORMS:
        os.environ.update(env)
        try:
            got_v, sums_v = csm.match_pairs(st, grids, src, slot, th0, search)
        finally:
            for k in env:
                os.environ.pop(k, None)
        assert got_v.tobytes() == got.tobytes() and np.array_equal(sums_v, sums), env
    return got, sums


def _assert_oracle(got, sums, want):
    for f in ("itheta", "ix", "iy"):
        assert np.array_equal(got[f], want[f]), (f, got[f], want[f])
    assert np.array_equal(sums, want["sum"]), (sums, want["sum"])


@pytest.mark.parametrize("cell_bits", [8, 16])
def test_points_on_pooled_entry_edges_every_form(gpu, cell_bits):
    scans, xy, off, src, slot, th0, want = _edge_case(cell_bits)
    spec = csm.grid_spec(RANGE, RES, 2.0, 1e-10, MAX_SHIFT, cell_bits)
    search = csm.search_spec(5, 17, 17, DEG)
    lay = csm.grid_layout(spec)
    assert lay.side <= 256 and all(64 <= len(s) <= 200 for s in scans[:-1])
    # CPU precondition: at the identity rotation every class of point is there (K: half + cx - hx + pad, cx = cy = 0)
    kx = lay.side // 2 - (search.nx - 1) // 2 + lay.pad
    ky = lay.side // 2 - (search.ny - 1) // 2 + lay.pad
    assert want["itheta"].tolist() == [2] * len(src)   # (the identity is where the sources match)
    cx, cy = _classes(scans[0], kx, ky)
    assert (cy == 0).all() and (cx == 1).sum() >= 30 and (cx == 2).sum() >= 4      # x alone
    cx, cy = _classes(scans[1], kx, ky)
    assert (cx == 0).all() and (cy == 1).sum() >= 30 and (cy == 2).sum() >= 4      # y alone
    cx, cy = _classes(scans[2], kx, ky)
    for a, b in ((1, 1), (1, 2), (2, 1), (2, 2)):                                  # both together
        assert ((cx == a) & (cy == b)).any(), (a, b)
    for s in scans[:3]:   # on the integer, and one float step to either side of it
        m = np.concatenate([_quot(s[:, 0]), _quot(s[:, 1])])
        m = m[_near(m)]
        assert (m == np.rint(m)).any() and (m < np.rint(m)).any() and (m > np.rint(m)).any()
    odd = scans[3]
    cx, cy = _classes(odd, kx, ky)
    assert np.isnan(odd).any() and np.isinf(odd).any() and ((cx == 3) | (cy == 3)).sum() >= 4
    big = np.abs(_quot(np.where(np.isfinite(odd), odd, 0))) >= 2.0 ** 22
    assert big.any(axis=1).sum() >= 2
    q = np.floor(np.where(np.isfinite(odd), odd, 0).astype(np.float64) / RES)
    assert (q > lay.side).any() and (q < -lay.side).any()                          # clamped at both ends

    st = csm.ScanTable(xy, off)
    grids = csm.LikelihoodGrids(st, [len(scans) - 1], spec)
    try:
        got, sums = _match_every_form(st, grids, src, slot, th0, search)
        _assert_oracle(got, sums, want)
        assert sums.min() > 0  # (the points do score against the target)
    finally:
        grids.close()
        st.close()


# ---- where the reductions end ----------------------------------------------------------------------------------
def _rot(p, a):
    c, s = math.cos(a), math.sin(a)
    return np.ascontiguousarray(p @ np.array([[c, s], [-s, c]], np.float32))


@functools.lru_cache(maxsize=None)
def _order_case(cell_bits):
    rng = np.random.default_rng(5)
    # an L-shaped room with a few pillars: one clear optimum in rotation and translation
    t = np.linspace(-4.0, 4.0, 90, dtype=np.float32)
    wall = np.concatenate([np.stack([t, np.full_like(t, 3.0)], 1), np.stack([np.full_like(t, -3.5), 0.7 * t], 1),
                           rng.uniform(-2.0, 2.0, (20, 2)).astype(np.float32)])
    tgt = wall
    # source 0: the target turned back by 30 steps -- the match is the lattice's LAST rotation (k = 60 of 61);
    # source 1: the target moved so that the match is 12 cells along x and 4 along y from the centre: block (Y, X) = (5, 6), lane 63's slot
    s0 = _rot(wall, -30 * DEG)
    s1 = wall - np.array([12 * RES, 4 * RES], np.float32)
    scans = [s0, s1, tgt]
    xy, off = csm.pack_scans(scans)
    src, slot, th0 = np.arange(2, dtype=np.int32), np.zeros(2, np.int32), np.zeros(2, np.float64)
    ospec = O.grid_spec(RANGE, RES, 2.0, 1e-10, cell_bits)
    ogr = O.grid_build_batch(xy, off, [2], ospec)
    want = O.csm_match_batch(xy, off, ogr, ospec, src, slot, th0, O.search_spec(61, 81, 81, DEG))
    return xy, off, src, slot, th0, want


@pytest.mark.parametrize("cell_bits", [8, 16])
def test_best_block_in_last_rotation_and_in_lane_63(gpu, cell_bits):
    xy, off, src, slot, th0, want = _order_case(cell_bits)
    # CPU precondition: the optimum is where the case wants it
    assert want["itheta"][0] == 60
    assert (want["iy"][1] // 8, want["ix"][1] // 8) == (5, 6)   # slot 63 of the bounds' layout (nhip_bnb_bounds.h slot_block)
    spec = csm.grid_spec(RANGE, RES, 2.0, 1e-10, 40, cell_bits)
    assert csm.grid_layout(spec).side <= 256
    search = csm.search_spec(61, 81, 81, DEG)
    st = csm.ScanTable(xy, off)
    grids = csm.LikelihoodGrids(st, [2], spec)
    try:
        got, sums = _match_every_form(st, grids, src, slot, th0, search)
        _assert_oracle(got, sums, want)
        assert sums.min() > 0
    finally:
        grids.close()
        st.close()
