"""Map windows and localisation without a device: hostside.map_cells / map_windows against the per-cell statement of the spec
(tests/localize_reference.py) bit for bit on every case the GPU tests run too, the rim property that ties a window's points to
the table build's cells, every refusal of the spec and of nhip_mapwin_origins through the C ABI, compose on hand-made records,
the quality of the whole path on the CPU oracle, and the example end to end through the map files."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from nautilus_amd import _lib, csm, hostside, localize, synth
from tests import localize_reference as R
from tests import occupancy_reference as OR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = R.shared_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hostside_equals_reference(case):
    name, grid, spec, origins = case
    g0 = grid.copy()
    want_cells, want = R.shared_results()[name]
    R.same_cells(hostside.map_cells(grid, spec), want_cells, name)
    R.same(hostside.map_windows(grid, spec, origins), want, name)
    assert np.array_equal(grid, g0)
    row_ptr, cols, n_occ = want_cells
    assert row_ptr[0] == 0 and row_ptr[-1] == n_occ == len(cols) == want[2][0] and (np.diff(row_ptr) >= 0).all()
    for y in range(spec.height):  # ascending inside every row, and exactly the occupied cells
        c = cols[row_ptr[y]:row_ptr[y + 1]]
        assert (np.diff(c) > 0).all() and np.array_equal(c, np.nonzero(grid[y] >= spec.occ_min)[0])
    xy, off, stats = want
    assert off[0] == 0 and off[-1] == len(xy) == stats[2] and stats[1] == len(origins) and stats[5] == stats[6] == stats[7] == 0
    assert stats[3] == (np.diff(off) == 0).sum() and stats[4] == np.diff(off).max()


def test_values_around_occ_min():
    """-128 and -1 are never occupied (a signed compare); 99 is not at occ_min 100 and is at occ_min 1; 0 never"""
    grid = np.array([R.VALUES], dtype=np.int8)
    for occ_min, want in ((100, [4, 5]), (1, [3, 4, 5]), (99, [3, 4, 5]), (50, [3, 4, 5])):
        spec = R.make_spec(width=6, height=1, occ_min=occ_min)
        assert R.map_cells(grid, spec)[1].tolist() == want == hostside.map_cells(grid, spec)[1].tolist()


def test_many_queries_and_overflow_statements():
    """2,500 queries with duplicates; the reference's two overflow rules (the GPU tests hold the kernels to them)"""
    name, grid, spec, origins = R.many_queries_case()
    want = R.map_windows(grid, spec, origins)
    R.same(hostside.map_windows(grid, spec, origins), want, name)
    n_occ, total = int(want[2][0]), int(want[2][2])
    assert total > 10000 and n_occ > 100
    R.same(R.map_windows(grid, spec, origins, max_cells=n_occ, capacity=total), want, name)
    short = R.map_windows(grid, spec, origins, max_cells=n_occ - 1)
    assert not short[1].any() and len(short[0]) == 0 and short[2].tolist() == [n_occ, len(origins), 0, len(origins), 0, 1, 0, 0]
    short = R.map_windows(grid, spec, origins, capacity=total - 1)
    assert not short[1].any() and len(short[0]) == 0 and short[2][6] == 1 and short[2][2] == 0 and short[2][4] == want[2][4]


@pytest.mark.parametrize("side", [2, 3, 160, 1200, 8192])
@pytest.mark.parametrize("res", [0.05, 0.01, 0.3])
def test_rim_cells_floor_back(side, res):
    """Item 3: for every k on the window's rim (and the whole range, it is cheap), the table build's floor((double)v / res) of
    the point v = (float)((k + 0.5) res) is k, so the cell is side/2 + k, inside [0, side)."""
    k = np.arange(-(side // 2), side - side // 2, dtype=np.int64)
    assert k[0] == -(side // 2) and k[-1] == side - side // 2 - 1 and len(k) == side
    v = ((k.astype(np.float64) + 0.5) * res).astype(np.float32)
    back = np.floor(v.astype(np.float64) / res)
    assert np.array_equal(back, k.astype(np.float64)), (side, res, k[back != k][:4])
    cell = side // 2 + back
    assert cell[0] == 0 and cell[-1] == side - 1
    # ... and through the product's statement, on a one-row map that fills the window exactly
    spec = R.make_spec(res=res, cell_x0=-(side // 2), cell_y0=0, width=side, height=1, side=side)
    xy, off, _ = hostside.map_windows(np.full((1, side), 100, np.int8), spec, [(0, 0)])
    assert off[-1] == side and np.array_equal(np.floor(xy[:, 0].astype(np.float64) / res), k.astype(np.float64))
    assert (np.floor(xy[:, 1].astype(np.float64) / res) == 0).all()


# ---------------------------------------------------------------- refusals through the C ABI, without a device
def product_spec(**kw):
    s = localize.default_spec()
    s.width, s.height, s.side = 8, 8, 8
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def spec_verdicts(s):
    """(accepted, message) of the check in each of the three entry points that take a spec: the calls are made with no buffers,
    so an accepted spec ends at the missing device or at the null pointers, never at a launch"""
    lib = _lib.load()
    out = []
    for call in (lambda: lib.nhip_mapwin_cells_dev(None, C.byref(s), 0, None, None, None, None),
                 lambda: lib.nhip_mapwin_gather_dev(None, None, C.byref(s), None, 0, None, 0, None, None, None, 1 << 20, None),
                 lambda: lib.nhip_map_windows(None, C.byref(s), None, 0, None, 0, None, None)):
        rc = call()
        msg = lib.nhip_last_error().decode()
        if rc == _lib.NHIP_ERR_NODEV or (rc == _lib.NHIP_ERR_ARG and "null pointer" in msg):
            out.append((True, msg))
        else:
            assert rc == _lib.NHIP_ERR_ARG, (rc, msg)
            out.append((False, msg))
    return out


EDGES = [("width", 1, 16384, "window"), ("height", 1, 16384, "window"), ("side", 2, 8192, "side"), ("occ_min", 1, 100, "occ_min"),
         ("flags", 0, 0, "flags"), ("reserved", 0, 0, "reserved")]


@pytest.mark.parametrize("field,lo,hi,word", EDGES, ids=[e[0] for e in EDGES])
def test_spec_edges(field, lo, hi, word):
    for v, ok in ((lo, True), (hi, True), (lo - 1, False), (hi + 1, False)):
        s = product_spec(**{field: v})
        for accepted, msg in spec_verdicts(s):
            assert accepted == ok, (field, v, msg)
            if not ok:
                assert word in msg and len(msg) > 10, (field, v, msg)
        if ok:
            hostside.mapwin_spec_check(s)
        else:
            with pytest.raises(ValueError, match=field):
                hostside.mapwin_spec_check(s)


def test_spec_res_defaults_and_counts():
    d = localize.default_spec()
    assert (d.res, d.occ_min, d.flags, d.reserved) == (0.05, 100, 0, 0) and C.sizeof(_lib.MapwinSpec) == 40
    assert (d.cell_x0, d.cell_y0, d.width, d.height, d.side) == (0, 0, 0, 0, 0)
    for res, ok in ((5e-324, True), (1.7976931348623157e308, True), (0.0, False), (-0.05, False), (math.inf, False), (math.nan, False)):
        s = product_spec(res=res)
        for accepted, msg in spec_verdicts(s):
            assert accepted == ok and (ok or "res" in msg), (res, msg)
        if not ok:
            with pytest.raises(ValueError, match="res"):
                hostside.mapwin_spec_check(s)
    lib, s = _lib.load(), product_spec()
    assert lib.nhip_mapwin_spec_default(None) == _lib.NHIP_ERR_ARG
    assert lib.nhip_mapwin_cells_dev(None, None, 0, None, None, None, None) == _lib.NHIP_ERR_ARG and b"null spec" in lib.nhip_last_error()
    assert lib.nhip_mapwin_cells_dev(None, C.byref(s), -1, None, None, None, None) == _lib.NHIP_ERR_ARG and b"max_cells" in lib.nhip_last_error()
    assert lib.nhip_mapwin_gather_dev(None, None, C.byref(s), None, -1, None, 0, None, None, None, 1 << 20, None) == _lib.NHIP_ERR_ARG
    assert b"n_queries" in lib.nhip_last_error()
    assert lib.nhip_mapwin_gather_dev(None, None, C.byref(s), None, 0, None, -1, None, None, None, 1 << 20, None) == _lib.NHIP_ERR_ARG
    assert b"out_capacity" in lib.nhip_last_error()
    assert lib.nhip_mapwin_gather_dev(None, None, C.byref(s), None, 100, None, 0, None, None, None, 399, None) == _lib.NHIP_ERR_ARG
    assert b"workspace" in lib.nhip_last_error()
    assert lib.nhip_map_windows(None, C.byref(s), None, -1, None, 0, None, None) == _lib.NHIP_ERR_ARG and b"n_queries" in lib.nhip_last_error()
    assert lib.nhip_map_windows(None, C.byref(s), None, 0, None, -1, None, None) == _lib.NHIP_ERR_ARG and b"capacity" in lib.nhip_last_error()
    w = lib.nhip_mapwin_workspace_bytes
    assert w(-1) == 0 and w(0) > 0 and w(1) >= 4 and w(10000) >= 40000 and w(2 ** 31 - 1) >= 4 * (2 ** 31 - 1) and w(10000) % 256 == 0
    with pytest.raises(ValueError, match="res"):
        localize.spec(OR.make_spec(res=0.1, width=8, height=8), csm.grid_spec(4.0, 0.05, 2.0, 1e-10, 8))
    mw = localize.spec(OR.make_spec(res=0.05, cell_x0=-3, cell_y0=9, width=11, height=13), csm.grid_spec(4.0, 0.05, 2.0, 1e-10, 8), occ_min=50)
    assert (mw.res, mw.cell_x0, mw.cell_y0, mw.width, mw.height, mw.side, mw.occ_min) == (0.05, -3, 9, 11, 13, 160, 50)


def test_origins_and_their_refusals():
    res = 0.05
    P = np.array([[0.0, 0.0, 0.1], [-1e-9, 0.0499999, -3.0], [1.0, -1.0, 7.0], [-0.05, 0.05, 0.0], [12.345, -67.891, 1.0]])
    org, th = localize.origins(P, res)
    want, want_th = hostside.map_window_origins(P, res)
    assert org.dtype == np.int32 and np.array_equal(org, want) and np.array_equal(th, want_th) and np.array_equal(th, P[:, 2])
    assert np.array_equal(org, np.floor(P[:, :2] / res).astype(np.int64)) and org[1].tolist() == [-1, 0]
    lib = _lib.load()
    for bad in (math.nan, math.inf, -math.inf):
        for col in range(3):
            Q = P.copy()
            Q[2, col] = bad
            o = np.zeros((len(Q), 2), np.int32)
            assert lib.nhip_mapwin_origins(_lib.ptr(Q), len(Q), res, _lib.ptr(o), None) == _lib.NHIP_ERR_ARG
            assert b"pose 2 is not finite" in lib.nhip_last_error()
            with pytest.raises(ValueError, match="pose 2 is not finite"):
                hostside.map_window_origins(Q, res)
    for col, v in ((0, 2.0 ** 30), (1, -2.0 ** 30 - 1), (0, 1e300), (1, -1e18)):
        Q = P.copy()
        Q[4, col] = v * res if abs(v) < 1e17 else v
        o = np.zeros((len(Q), 2), np.int32)
        assert lib.nhip_mapwin_origins(_lib.ptr(Q), len(Q), res, _lib.ptr(o), None) == _lib.NHIP_ERR_ARG
        assert b"pose 4 lies 2^30 cells or more" in lib.nhip_last_error()
        with pytest.raises(ValueError, match="pose 4 lies"):
            hostside.map_window_origins(Q, res)
    Q = np.array([[2.0 ** 30 - 0.5, -(2.0 ** 30) + 1.5, 0.0]])  # the largest floors that are accepted (res 1: exact)
    assert localize.origins(Q, 1.0)[0].tolist() == [[2 ** 30 - 1, -2 ** 30 + 1]] == hostside.map_window_origins(Q, 1.0)[0].tolist()
    Q = np.array([[-(2.0 ** 30), 0.0, 0.0]])  # the floor -2^30 has magnitude 2^30: refused
    assert lib.nhip_mapwin_origins(_lib.ptr(Q), 1, 1.0, _lib.ptr(np.zeros((1, 2), np.int32)), None) == _lib.NHIP_ERR_ARG
    for res_bad in (0.0, -1.0, math.nan, math.inf):
        assert lib.nhip_mapwin_origins(_lib.ptr(P), len(P), res_bad, _lib.ptr(np.zeros((5, 2), np.int32)), None) == _lib.NHIP_ERR_ARG
        assert b"res" in lib.nhip_last_error()
        with pytest.raises(ValueError, match="res"):
            hostside.map_window_origins(P, res_bad)
    assert lib.nhip_mapwin_origins(None, -1, res, None, None) == _lib.NHIP_ERR_ARG and b"n -1" in lib.nhip_last_error()
    assert lib.nhip_mapwin_origins(None, 0, res, None, None) == _lib.NHIP_OK
    assert lib.nhip_mapwin_origins(None, 1, res, None, None) == _lib.NHIP_ERR_ARG and b"null pointer" in lib.nhip_last_error()


def test_compose_on_hand_made_records():
    gs, srch = csm.grid_spec(4.0, 0.05, 2.0, 1e-10, 8), csm.search_spec(21, 17, 17, math.radians(1.0))
    rec = np.zeros(4, dtype=csm.MATCH_DTYPE)
    rec[0] = (10, 8, 8, -1.5)    # the lattice's centre: the origin cell's corner, the prior's heading
    rec[1] = (0, 0, 16, -2.0)    # its ends
    rec[2] = (-1, -1, -1, -np.inf)  # a rejected record of the gated call
    rec[3] = (20, 16, 0, -2.5)
    org = np.array([[100, -200], [-3, 7], [5, 5], [2 ** 30 - 1, -2 ** 30 + 1]], np.int32)
    th0 = np.array([0.25, 3.1, 1.0, -3.1])
    for fn in (localize.compose, hostside.localize_compose):
        p = fn(rec, org, th0, gs, srch)
        assert p.dtype == np.float64 and p.shape == (4, 3)
        assert p[0].tolist() == [100 * 0.05, -200 * 0.05, 0.25]
        assert p[1, 0] == (-3 - 8) * 0.05 and p[1, 1] == (7 + 8) * 0.05 and p[1, 2] == csm.angle_mod(3.1 - 10 * math.radians(1.0))
        assert np.isnan(p[2]).all()
        assert p[3, 0] == (2 ** 30 - 1 + 8) * 0.05 and p[3, 1] == (-2 ** 30 + 1 - 8) * 0.05
        assert p[3, 2] == csm.angle_mod(-3.1 + 10 * math.radians(1.0)) and abs(p[3, 2]) <= math.pi
    # the same numbers as the matcher's own conversion gives for the translation inside the window's frame
    tx, ty, th = csm.match_to_transform(rec[1], gs, srch, th0[1])
    assert np.float32(p[1, 0] - org[1, 0] * 0.05) == tx and np.float32(p[1, 1] - org[1, 1] * 0.05) == ty
    with pytest.raises(ValueError):
        localize.compose(rec, org[:3], th0, gs, srch)


# ---------------------------------------------------------------- quality, on the reference alone
def test_quality_on_the_cpu_oracle():
    """The prototype's setup: SynthBag(120); the map from the 60 even scans at their truth poses through
    tests/occupancy_reference.occupancy with the defaults on hostside.map_window(truth, 30, 0.05) -- 1513 x 1500 cells, 3,121
    occupied; the queries are the 30 scans 1, 5, ..., 117 through hostside.localize on the oracle's CPU backend (config #2's
    table and lattice: +-2 m, +-30 degrees), 2,494 - 3,121 points per window.
    Conditions: priors 1.0 m off in a seeded direction and 10.4 degrees, and 1.9 m / 27.3 degrees -- neither a multiple of
    the lattice -- end within 0.15 m (three cells) and 1.0 degree (one step) of the truth; a second prior in the same window of
    the lattice (moved by whole and part cells, same heading) gives the same pose, bit for bit.
    Measured here: 1.0 m / 10.4 degrees: largest position error 0.090 m, mean 0.049 m, largest heading error 0.60 degrees,
    scores -3.10 .. -1.42; 1.9 m / 27.3 degrees: 0.094 m, mean 0.046 m, 0.30 degrees.  Priors 3 m off, outside the lattice (not
    a condition): scores fall to -18.1, all 30 poses are more than 0.15 m off (up to 3.7 m and 11.6 degrees), and 2 of those
    wrong poses still score above -5 (the best -2.68, inside the range of the right ones): a score gate
    helps but does not decide."""
    from oracle.cpu_backend import OracleBackend
    bag = synth.SynthBag(120)
    even = list(range(0, 120, 2))
    xy, off = csm.pack_scans([bag.scans[i] for i in even])
    x0, y0, w, h = hostside.map_window(bag.truth, 30.0, 0.05)
    occ = OR.make_spec(cell_x0=x0, cell_y0=y0, width=w, height=h)
    grid = OR.occupancy(xy, off, bag.truth[even], occ)[0]
    assert grid.shape == (1513, 1500) and int((grid == 100).sum()) == 3121
    q = list(range(1, 120, 4))
    n = len(q)
    truth = bag.truth[q]
    rng = np.random.default_rng(3)
    d = rng.uniform(0.0, 2.0 * math.pi, n)

    def off_by(r, deg):
        return truth + np.stack([r * np.cos(d), r * np.sin(d), np.full(n, math.radians(deg))], axis=1)
    near, far, outside = off_by(1.0, 10.4), off_by(1.9, 27.3), off_by(3.0, 10.4)
    moved = near + np.stack([3 * 0.05 + 0.013 * np.cos(d), -2 * 0.05 + 0.011 * np.sin(d), np.zeros(n)], axis=1)
    priors = np.concatenate([near, far, moved, outside])
    qxy, qoff = csm.pack_scans([bag.scans[i] for i in q] * 4)
    r = hostside.localize(OracleBackend(), qxy, qoff, priors, grid, occ)
    assert not r["rejected"].any() and r["poses"].shape == (4 * n, 3)
    e = r["poses"] - np.tile(truth, (4, 1))
    pos, ang = np.hypot(e[:, 0], e[:, 1]), np.degrees(np.abs(csm.angle_mod(e[:, 2])))
    score = r["records"]["score"]
    for k, name in enumerate(("1.0 m / 10.4 deg", "1.9 m / 27.3 deg", "moved inside the lattice", "3.0 m / 10.4 deg")):
        s = slice(k * n, (k + 1) * n)
        print("%-26s position error max %.3f m mean %.3f m, heading error max %.2f deg, scores %.2f .. %.2f, points per window %d .. %d"
              % (name, pos[s].max(), pos[s].mean(), ang[s].max(), score[s].min(), score[s].max(), r["points_per_window"][s].min(),
                 r["points_per_window"][s].max()))
    wrong = pos[3 * n:] > 0.15
    print("3.0 m: %d of %d poses more than 0.15 m off; %d of those score above -5" % (wrong.sum(), n, (score[3 * n:][wrong] > -5).sum()))
    assert pos[:2 * n].max() <= 0.15 and ang[:2 * n].max() <= 1.0
    assert not np.array_equal(r["origins"][:n], r["origins"][2 * n:3 * n])
    assert r["poses"][:n].tobytes() == r["poses"][2 * n:3 * n].tobytes()


def test_localize_refuses_mismatched_tables():
    grid = np.zeros((8, 8), np.int8)
    with pytest.raises(ValueError, match="res"):
        hostside.localize(None, np.zeros((0, 2), np.float32), [0], np.zeros((0, 3)), grid, OR.make_spec(res=0.1, width=8, height=8))
    with pytest.raises(ValueError, match="priors"):
        hostside.localize(None, np.zeros((0, 2), np.float32), [0], np.zeros((2, 3)), grid, OR.make_spec(width=8, height=8))
    mw = localize.spec(OR.make_spec(width=8, height=8), csm.grid_spec(4.0, 0.05, 2.0, 1e-10, 8))
    with pytest.raises(ValueError, match="side"):  # a window spec made for other tables than the call's (config #2: side 1200)
        localize.localize(np.zeros((0, 2), np.float32), [0], np.zeros((0, 3)), grid, mw)
    with pytest.raises(ValueError, match="res"):
        localize.localize(np.zeros((0, 2), np.float32), [0], np.zeros((0, 3)), grid, OR.make_spec(res=0.1, width=8, height=8))


def test_example_end_to_end_on_the_oracle(tmp_path):
    """examples/localize.py --backend oracle on a small bag, through the map files"""
    stem = str(tmp_path / "map")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "localize.py"), "--backend", "oracle", "--scans", "24", "--map-scans",
                          "16", "--map-poses", "truth", "--map", stem], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert os.path.exists(stem + ".pgm") and os.path.exists(stem + ".yaml")
    assert res["backend"] == "oracle" and res["queries"] == 8 and res["rejected"] == 0 and len(res["poses"]) == 8
    assert res["position_error_max_m"] <= 0.15 and res["heading_error_max_deg"] <= 1.0
    assert res["points_per_window_min"] > 100
    grid, info = hostside.read_occupancy_map(stem)
    assert info["resolution"] == 0.05 and int((grid == 100).sum()) == res["map_cells_occupied"]
