"""Map vectorisation on the GPU (K13, nhip_vectorize.hip) against the numpy statement of the spec
(tests/vectorize_reference.py).  Everything the device computes is integer: counts, cell list, initial votes, the votes and
live bytes left at the end, records and stats are compared for EQUALITY; the lines (host, double) on their bits.  The shapes
are the smallest at which each loop can go wrong: windows that are no multiple of any tile, a votes row in several LDS
slabs (16384 x 1), along-line bins at both extremes (1 x 16384), one and several runs per round, every way a call ends."""
import ctypes as C

import numpy as np
import pytest

from nautilus_amd import _lib, csm, synth, vectorize
from tests import vectorize_reference as R

pytestmark = pytest.mark.gpu

BAD_MAP_SCAN_OFFSETS = 16384


def product_spec(spec):
    return vectorize.spec(**{f: getattr(spec, f) for f in R.FIELDS})


def check(xy, off, poses, spec, max_rounds=None, max_cells=None, check_every=8):
    """one device call against the reference; returns (got, want)"""
    s = product_spec(spec)
    kw = dict(max_rounds=vectorize.MAX_ROUNDS if max_rounds is None else max_rounds, max_cells=max_cells, check_every=check_every)
    lines, rec, stats, planes = vectorize.vectorize(xy, off, poses, s, planes=True, **kw)
    want = R.vectorize(xy, off, poses, spec, max_rounds=max_rounds, max_cells=max_cells)
    assert np.array_equal(planes["counts"], want["counts"])
    assert stats.tolist() == want["stats"].tolist()
    assert rec.tolist() == want["records"].tolist()
    assert np.array_equal(lines.view(np.uint32), want["lines"].view(np.uint32))
    if stats[3] != 3:
        assert np.array_equal(planes["cells"], want["cells"])
        assert np.array_equal(planes["live"].astype(bool), want["live"])
        # the votes left: those of the cells still live
        left = R.hough(want["cells"][want["live"]], spec, max_rounds=0)[2]
        assert np.array_equal(planes["votes"], left)
        # the initial votes: a call of no rounds
        first = vectorize.vectorize(xy, off, poses, s, planes=True, max_rounds=0, max_cells=max_cells)[3]
        assert np.array_equal(first["votes"], want["votes"]) and first["live"].all()
    return (lines, rec, stats, planes), want


def crafted(name):
    cells, spec = R.crafted()[name]
    return R.scan_of_cells(cells, spec) + (spec,)


@pytest.mark.parametrize("name", sorted(R.crafted()))
def test_crafted_cases_96x64(gpu, name):
    """one line; equal votes (the smaller index wins); a cross (the shared cell goes to the first line); a dotted line with
    gaps of exactly max_gap and max_gap + 1 (two runs in one round); runs of min_length - 1 and min_length; a band edge at
    exactly the half width, and one unit inside; a blob that only retires; a retired stub beside a short line"""
    xy, off, poses, spec = crafted(name)
    (_, rec, stats, _), _ = check(xy, off, poses, spec)
    if name == "blob":
        assert stats[1] == 0 and stats[5] > 0
    if name == "dotted":
        assert stats[1] == 2 and stats[2] == 1


def test_window_1x1(gpu):
    spec = R.make_spec(width=1, height=1, min_hits=2, min_votes=1, min_length=1, n_theta=3, cell_x0=-3, cell_y0=7)
    xy, off, poses = R.scan_of_cells([(0, 0)], spec)
    (_, rec, stats, _), _ = check(xy, off, poses, spec)
    assert stats[:4].tolist() == [1, 1, 1, 0] and rec[0, 4] == 1


def test_window_7x5(gpu):
    spec = R.make_spec(width=7, height=5, min_hits=1, min_votes=2, min_length=3, max_gap=1, n_theta=4)
    cells = [(0, 0), (1, 1), (2, 2), (3, 3), (4, 4), (6, 0), (6, 1), (6, 2), (6, 4), (0, 4)]
    (_, rec, stats, _), _ = check(*R.scan_of_cells(cells, spec), spec)
    assert stats[1] >= 2


def test_window_130x67_random_lines(gpu):
    """neither axis a multiple of 32 or 64; rows of 130 cells: a partial second ballot group in the pack; 45 directions"""
    rng = np.random.default_rng(3)
    spec = R.make_spec(width=130, height=67, min_hits=1, min_votes=8, min_length=8, n_theta=45, cell_x0=-40, cell_y0=100)
    cells = set()
    for _ in range(9):
        x0, y0, x1, y1 = rng.uniform(0, 130), rng.uniform(0, 67), rng.uniform(0, 130), rng.uniform(0, 67)
        for t in np.linspace(0, 1, 200):
            cells.add((int(x0 + t * (x1 - x0)), int(y0 + t * (y1 - y0))))
    cells |= {(int(x), int(y)) for x, y in rng.uniform(0, 67, (150, 2))}
    cells = [c for c in cells if c[0] < 130 and c[1] < 67]
    (_, rec, stats, _), _ = check(*R.scan_of_cells(cells, spec), spec)
    assert stats[1] >= 5 and stats[5] > 0 and stats[2] > stats[1] // 2


@pytest.mark.parametrize("w,h", [(16384, 1), (1, 16384)])
def test_long_narrow_windows(gpu, w, h):
    """n_rho = 32770 / 16387: the votes rows in five / three LDS slabs; cells at both ends of the window: rho and the
    along-line bin at both extremes (a < 0 in the tall window's rows with C < 0)"""
    spec = R.make_spec(width=w, height=h, min_hits=1, min_votes=5, min_length=10, n_theta=12)
    n = max(w, h)
    pos = list(range(0, 60)) + list(range(8000, 8060, 2)) + list(range(n - 90, n)) + [n // 2]
    cells = [(p, 0) if h == 1 else (0, p) for p in pos]
    (_, rec, stats, _), want = check(*R.scan_of_cells(cells, spec), spec)
    assert stats[0] == len(pos) and stats[1] >= 3


def edge_points(spec):
    """points one float either side of cell edges at the window's four corners, and on its far edges"""
    f = np.float32
    x_lo, x_hi = spec.cell_x0 * spec.res, (spec.cell_x0 + spec.width) * spec.res
    y_lo, y_hi = spec.cell_y0 * spec.res, (spec.cell_y0 + spec.height) * spec.res
    pts = []
    for x in (x_lo, x_lo + spec.res, x_hi - spec.res, x_hi):
        for y in (y_lo, y_lo + spec.res, y_hi - spec.res, y_hi):
            for dx in (-1, 0, 1):
                for dy in (-1, 0, 1):
                    px = np.nextafter(f(x), f(np.inf) * dx) if dx else f(x)
                    py = np.nextafter(f(y), f(np.inf) * dy) if dy else f(y)
                    pts.append((px, py))
    return np.array(pts, dtype=f)


def test_cell_edges_corners_and_dropped_points(gpu):
    spec = R.make_spec(width=16, height=12, cell_x0=-8, cell_y0=-5, min_hits=1, min_votes=2, min_length=2, n_theta=4)
    edges = edge_points(spec)
    junk = np.array([[np.nan, 0.1], [0.1, np.nan], [np.inf, 0.1], [0.1, -np.inf], [1e30, 0.1], [0.1, -1e30], [3e38, 3e38],
                     [-1e30, -1e30]], dtype=np.float32)
    inside = np.array([[0.01, 0.01], [0.01, 0.01], [-0.01, -0.01]], dtype=np.float32)
    xy = np.concatenate([edges, junk, inside])
    off = np.array([0, len(edges), len(edges) + len(junk), len(xy)], dtype=np.int32)
    (_, _, _, planes), want = check(xy, off, np.zeros((3, 3)), spec)
    c = planes["counts"]
    assert c[0, 0] > 0 and c[0, -1] > 0 and c[-1, 0] > 0 and c[-1, -1] > 0
    assert c.sum() < len(edges) + 3  # (the far edge and everything past an outer edge is dropped; the junk all of it)
    assert c[5, 8] == 2 and c[4, 7] == 1
    # the same under a pose: the float affine, each operation rounded on its own
    poses = np.array([[0.013, -0.02, 0.7], [0.3, 0.2, -2.0], [-0.11, 0.05, 3.1]])
    check(xy, off, poses, spec)


def test_min_hits_threshold(gpu):
    spec = R.make_spec(width=40, height=9, min_hits=3, min_votes=3, min_length=5, n_theta=4)
    two, _, _ = R.scan_of_cells(R.hline(2, 3, 30), spec, hits=2)   # min_hits - 1: never cells
    three, _, _ = R.scan_of_cells(R.hline(6, 3, 30), spec, hits=3)
    xy = np.concatenate([two, three])
    off = np.array([0, len(two), len(xy)], dtype=np.int32)
    (_, rec, stats, planes), _ = check(xy, off, np.zeros((2, 3)), spec)
    assert stats[0] == 28 and (planes["cells"][:, 1] == 6).all() and planes["counts"][2, 3] == 2


def test_nothing_to_do(gpu):
    spec = R.make_spec(width=33, height=17, min_hits=1)
    none = np.zeros((0, 2), np.float32)
    for off, poses in ((np.array([0], np.int32), np.zeros((0, 3))), (np.array([0, 0, 0], np.int32), np.zeros((2, 3)))):
        (_, rec, stats, _), _ = check(none, off, poses, spec)
        assert stats.tolist() == [0, 0, 0, 0, 0, 0, 2 * 33 + 17 + 1, 0] and len(rec) == 0
    # cells, but too few votes: M > 0, no round
    xy, off, poses = R.scan_of_cells([(1, 1), (20, 9)], spec)
    (_, rec, stats, _), _ = check(xy, off, poses, spec)
    assert stats[:4].tolist() == [2, 0, 0, 0]


@pytest.mark.parametrize("n_theta", [2, 3, 45, 360])
def test_direction_counts(gpu, n_theta):
    xy, off, poses, spec = crafted("cross")
    spec.n_theta = n_theta
    check(xy, off, poses, spec)


def test_max_segments(gpu):
    """0, 1 and exactly the number needed; two runs of ONE round that do not both fit commit nothing"""
    xy, off, poses, spec = crafted("tie")  # two rounds, one segment each
    for cap, flag, segs in ((0, 2, 0), (1, 2, 1), (2, 0, 2)):
        spec.max_segments = cap
        (_, rec, stats, planes), _ = check(xy, off, poses, spec)
        assert (stats[3], stats[1], stats[2]) == (flag, segs, segs)
        assert planes["live"].sum() == 40 - 20 * segs
    xy, off, poses, spec = crafted("dotted")
    spec.max_segments = 1
    (_, rec, stats, planes), _ = check(xy, off, poses, spec)
    assert stats[1:6].tolist() == [0, 0, 2, 0, 0] and planes["live"].all()


def test_max_rounds(gpu):
    xy, off, poses, spec = crafted("tie")
    (_, rec, stats, _), _ = check(xy, off, poses, spec, max_rounds=1)
    assert stats[1:4].tolist() == [1, 1, 1]
    (_, rec, stats, _), _ = check(xy, off, poses, spec, max_rounds=2)
    assert stats[1:4].tolist() == [2, 2, 0]  # (the third round's peak is below min_votes: flag 0, not 1)


def raw_call(xy, off, poses, s, max_cells, fill=0xA5, pad=512):
    """nhip_vectorize_dev on buffers this test owns, every byte preset to `fill`, `pad` guard bytes behind each"""
    import torch
    lib, dev = _lib.load(), torch.device("cuda:0")
    L = vectorize.workspace_layout(s, max_cells)
    guard = lambda n: torch.full((n + pad + 256,), fill, dtype=torch.uint8, device=dev)
    ws_all, rec_all, st_all = guard(L.bytes), guard(80 * max(s.max_segments, 1)), guard(32)
    al = lambda t: t[(-t.data_ptr()) % 256:]
    ws, rec, st = al(ws_all), al(rec_all), al(st_all)
    d_xy = torch.from_numpy(np.ascontiguousarray(xy, np.float32)).to(dev)
    d_off = torch.from_numpy(np.ascontiguousarray(off, np.int32)).to(dev)
    d_aff = torch.from_numpy(vectorize.pose_affines(poses)).to(dev)
    rc = lib.nhip_vectorize_dev(d_xy.data_ptr(), d_off.data_ptr(), d_aff.data_ptr(), len(off) - 1, C.byref(s), max_cells,
                                vectorize.MAX_ROUNDS, 4, rec.data_ptr(), st.data_ptr(), ws.data_ptr(), L.bytes, None)
    info = (C.c_int32 * 4)()
    rc_status = lib.nhip_dev_status(None, info)
    return rc, rc_status, list(info), L, ws.cpu().numpy(), rec.cpu().numpy(), st.cpu().numpy()


def test_max_cells_one_short(gpu):
    """flag 3 and the count needed; no cell, live byte or record is written, nothing behind any buffer"""
    xy, off, poses, spec = crafted("cross")
    s = product_spec(spec)
    rc, rc_status, info, L, ws, rec, st = raw_call(xy, off, poses, s, 80)
    assert rc == 0 and rc_status == 0
    assert st[:32].view(np.int32).tolist() == [81, 0, 0, 3, 0, 0, 2 * 96 + 64 + 1, 0]
    assert (st[32:] == 0xA5).all() and (rec == 0xA5).all() and (ws[L.bytes:] == 0xA5).all()
    assert (ws[L.cells_offset:L.cells_offset + 8 * 80] == 0xA5).all() and (ws[L.live_offset:L.live_offset + 80] == 0xA5).all()
    check(xy, off, poses, spec, max_cells=80)
    # exactly enough: the whole call, and still nothing behind the buffers
    rc, rc_status, info, L, ws, rec, st = raw_call(xy, off, poses, s, 81)
    want = R.vectorize(xy, off, poses, spec)
    assert rc == 0 and st[:32].view(np.int32).tolist() == want["stats"].tolist()
    assert (ws[L.bytes:] == 0xA5).all() and (st[32:] == 0xA5).all()
    assert rec[:160].view(np.int64).reshape(2, 10).tolist() == want["records"].tolist() and (rec[80 * s.max_segments:] == 0xA5).all()


def test_bad_scan_offset_is_an_empty_scan(gpu):
    """scan 1's end lies before its start: kind 16384, the scan is empty, scans 0 and 2 as ever"""
    xy, off, poses, spec = crafted("cross")
    s = product_spec(spec)
    n = len(xy)
    off = np.array([0, 30, 10, n], dtype=np.int32)
    rc, rc_status, info, L, ws, rec, st = raw_call(xy, off, np.zeros((3, 3)), s, 4096)
    assert rc == 0 and rc_status == _lib.NHIP_ERR_ARG and b"nhip_vectorize_dev" in _lib.load().nhip_last_error()
    assert info == [BAD_MAP_SCAN_OFFSETS, BAD_MAP_SCAN_OFFSETS, 10, 2]
    want = R.vectorize(xy, off, np.zeros((3, 3)), spec)
    assert st[:32].view(np.int32).tolist() == want["stats"].tolist()
    k = int(want["stats"][1])
    assert rec[:80 * k].view(np.int64).reshape(k, 10).tolist() == want["records"].tolist()
    counts = ws[L.counts_offset:L.counts_offset + 4 * 96 * 64].view(np.int32).reshape(64, 96)
    assert np.array_equal(counts, want["counts"])
    with pytest.raises(_lib.NhipError, match="scan offset"):
        vectorize.vectorize(xy, np.array([-1, 30, n], np.int32), np.zeros((2, 3)), s)


@pytest.fixture(scope="module")
def bag40():
    """SynthBag(40) at its odometry poses, defaults: thousands of cells, tens of rounds, retirements; the reference once"""
    bag = synth.SynthBag(40)
    xy, off = csm.pack_scans(bag.scans)
    s = vectorize.window_spec(bag.odom, 30.0)
    return xy, off, bag.odom, s, R.vectorize(xy, off, bag.odom, s)


def test_realistic_bag(gpu, bag40):
    xy, off, poses, s, want = bag40
    assert want["stats"][0] > 3000 and want["stats"][2] >= 15 and want["stats"][5] > 0
    lines, rec, stats, planes = vectorize.vectorize(xy, off, poses, s, planes=True)
    assert np.array_equal(planes["counts"], want["counts"]) and np.array_equal(planes["cells"], want["cells"])
    assert stats.tolist() == want["stats"].tolist() and rec.tolist() == want["records"].tolist()
    assert np.array_equal(planes["live"].astype(bool), want["live"])
    assert np.array_equal(lines.view(np.uint32), want["lines"].view(np.uint32))
    first = vectorize.vectorize(xy, off, poses, s, planes=True, max_rounds=0)[3]
    assert np.array_equal(first["votes"], want["votes"])


def test_check_every_and_repeat_give_the_same_bytes(gpu, bag40):
    xy, off, poses, s, want = bag40
    runs = [vectorize.vectorize(xy, off, poses, s, planes=True, check_every=k) for k in (1, 3, 1000, 1000)]
    for lines, rec, stats, planes in runs:
        assert stats.tobytes() == runs[0][2].tobytes() == want["stats"].tobytes()
        assert rec.tobytes() == runs[0][1].tobytes() and lines.tobytes() == runs[0][0].tobytes()
        for k in ("counts", "cells", "votes", "live"):
            assert planes[k].tobytes() == runs[0][3][k].tobytes()


def test_handle_form_equals_device_form(gpu, bag40):
    xy, off, poses, s, want = bag40
    scans = csm.ScanTable(xy, off)
    lines, rec, stats = vectorize.vectorize_on_handle(scans, poses, s)
    scans.close()
    assert stats.tolist() == want["stats"].tolist() and rec.tolist() == want["records"].tolist()
    assert np.array_equal(lines.view(np.uint32), want["lines"].view(np.uint32))
    xy, off, poses, spec = crafted("tie")
    scans = csm.ScanTable(xy, off)
    lines, rec, stats = vectorize.vectorize_on_handle(scans, poses, product_spec(spec), max_rounds=1, check_every=1)
    scans.close()
    assert stats[1:4].tolist() == [1, 1, 1]
