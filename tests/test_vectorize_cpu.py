"""Map vectorisation without a GPU ("Map vectorisation"): the numpy reference against records worked
out by hand, the pure-host entry points of the C ABI against numpy bit for bit, the spec's accepted ranges, the workspace's
layout, the quality of the method on a synthetic bag, and the proof that the crafted cases tell four deliberate mistakes
apart."""
import ctypes as C
import math

import numpy as np
import pytest

from nautilus_amd import _lib, csm, hostside, synth, vectorize
from tests import vectorize_reference as R

W = 96  # width of the crafted windows: bin b of a horizontal line is cy + W, of a vertical one cx + W


def run_case(name, perturb=None):
    cells, spec = R.crafted()[name]
    xy, off, poses = R.scan_of_cells(cells, spec)
    return R.vectorize(xy, off, poses, spec, perturb=perturb), spec


def moments(cells):
    x, y = np.array(cells, dtype=np.int64).T
    return [len(x), x.sum(), y.sum(), (x * x).sum(), (x * y).sum(), (y * y).sum()]


def test_reference_records_worked_out_by_hand():
    """n_theta 4: row 0 is the vertical direction (C = 2^14, S = 0: b = cx + W, a = cy + W), row 2 the horizontal one
    (C = 0, S = 2^14: b = cy + W, a = W - cx)."""
    out, _ = run_case("one_line")  # y = 20, x = 10 .. 39
    assert out["records"].tolist() == [[2, 20 + W, W - 39, W - 10, 30, 735, 600, 20255, 14700, 12000]]
    assert out["stats"].tolist() == [30, 1, 1, 0, 30, 0, 2 * W + 64 + 1, 0]
    out, _ = run_case("tie")  # 20 votes each: the vertical line (row 0) has the smaller index
    assert out["records"].tolist() == [[0, 20 + W, 5 + W, 24 + W] + moments(R.vline(20, 5, 24)),
                                       [2, 40 + W, W - 69, W - 50] + moments(R.hline(40, 50, 69))]
    out, _ = run_case("dotted")  # x = 5..16, 21..32 (4 empty bins: bridged), 38..49 (5 empty bins: a run of its own)
    assert out["records"].tolist() == [[2, 12 + W, W - 49, W - 38] + moments(R.hline(12, 38, 49)),
                                       [2, 12 + W, W - 32, W - 5] + moments(R.hline(12, 5, 16) + R.hline(12, 21, 32))]
    assert out["stats"][2] == 1  # (both runs in ONE round, ascending a)
    out, _ = run_case("lengths")  # 9 cells at y = 8 retire, 10 cells at y = 50 are kept
    assert out["records"].tolist() == [[2, 50 + W, W - 12, W - 3] + moments(R.hline(50, 3, 12))]
    assert out["stats"].tolist() == [19, 1, 2, 0, 10, 9, 2 * W + 64 + 1, 0]
    out, _ = run_case("cross")  # the shared cell (40, 30) and its band neighbours go to the first line
    assert out["stats"][1] == 2 and out["records"][:, 4].sum() == 81 and out["records"][0, 4] > 41
    out, _ = run_case("diag_neg")  # row 3 (C < 0): a_q is negative for the cells with cx + cy > 135
    assert out["records"][0, 0] == 3 and out["records"][0, 2] < 0 < out["records"][0, 3] and out["records"][0, 4] == 40
    out, _ = run_case("blob")
    assert out["stats"][1] == 0 and out["stats"][5] > 0 and len(out["records"]) == 0


@pytest.mark.parametrize("perturb,case", [("tie_largest", "tie"), ("band_plus_one", "band_edge"), ("gap_le", "dotted"),
                                          ("retire_late", "stub")])
def test_crafted_cases_discriminate(perturb, case):
    """Each deliberate mistake changes the records of at least one crafted case."""
    good, _ = run_case(case)
    bad, _ = run_case(case, perturb)
    assert good["records"].shape != bad["records"].shape or not np.array_equal(good["records"], bad["records"])


def bad_specs():
    big = dict(width=8, height=8)
    yield "res", dict(big, res=0.0)
    yield "res", dict(big, res=float("nan"))
    yield "res", dict(big, res=float("inf"))
    yield "window", dict(width=0, height=8)
    yield "window", dict(width=8, height=16385)
    yield "window", dict(width=16385, height=8)
    yield "min_hits", dict(big, min_hits=0)
    yield "min_hits", dict(big, min_hits=(1 << 30) + 1)
    yield "n_theta", dict(big, n_theta=1)
    yield "n_theta", dict(big, n_theta=1025)
    yield "min_votes", dict(big, min_votes=0)
    yield "band", dict(big, band=0.49)
    yield "band", dict(big, band=float("nan"))
    yield "band", dict(big, band=float("inf"))
    yield "max_gap", dict(big, max_gap=-1)
    yield "min_length", dict(big, min_length=0)
    yield "max_segments", dict(big, max_segments=-1)


@pytest.mark.parametrize("word,fields", list(bad_specs()))
def test_bad_spec_is_an_argument_error_without_a_device(word, fields):
    lib = _lib.load()
    s = vectorize.spec(**fields)
    L = _lib.VectorizeLayout()
    stats = np.zeros(8, np.int32)
    for rc in (lib.nhip_vectorize_workspace_layout(C.byref(s), 16, C.byref(L)),
               lib.nhip_vectorize_dev(None, None, None, 0, C.byref(s), 16, 1, 1, None, _lib.ptr(stats), None, 0, None),
               lib.nhip_vectorize(None, None, C.byref(s), 16, 1, 1, None, _lib.ptr(stats)),
               lib.nhip_vectorize_endpoints(C.byref(s), None, 0, None)):
        assert rc == _lib.NHIP_ERR_ARG
        assert word in lib.nhip_last_error().decode()
    assert lib.nhip_vectorize_workspace_bytes(C.byref(s), 16) == -1


def test_bad_call_arguments_and_no_device():
    lib = _lib.load()
    s = vectorize.spec(width=8, height=8)
    stats = np.zeros(8, np.int32)
    for cells, rounds, every in ((-1, 1, 1), (1, -1, 1), (1, 1, 0)):
        assert lib.nhip_vectorize_dev(None, None, None, 0, C.byref(s), cells, rounds, every, None, _lib.ptr(stats), None, 0,
                                      None) == _lib.NHIP_ERR_ARG
    assert lib.nhip_vectorize_dev(None, None, None, -1, C.byref(s), 1, 1, 1, None, _lib.ptr(stats), None, 0, None) == _lib.NHIP_ERR_ARG
    if _lib.device_count() == 0:  # (no CPU path: the compute entry points refuse, the pure-host ones above and below work)
        assert lib.nhip_vectorize_dev(None, None, None, 0, C.byref(s), 1, 1, 1, None, _lib.ptr(stats), None, 0, None) == _lib.NHIP_ERR_NODEV
        assert lib.nhip_vectorize(None, None, C.byref(s), 1, 1, 1, None, _lib.ptr(stats)) == _lib.NHIP_ERR_NODEV


def test_default_spec():
    s = vectorize.default_spec()
    assert [getattr(s, f) for f in R.FIELDS] == [0.05, 1.5, 0, 0, 0, 0, 2, 360, 20, 4, 10, 4096, 0, 0]
    assert C.sizeof(_lib.VectorizeSpec) == 64 and C.sizeof(_lib.VectorizeLayout) == 48
    ref = R.make_spec(width=0, height=0)
    assert all(getattr(s, f) == getattr(ref, f) for f in R.FIELDS)


@pytest.mark.parametrize("n_theta", [2, 3, 360, 1024])
def test_tables_equal_numpy(n_theta):
    c, s = vectorize.tables(vectorize.spec(width=1, height=1, n_theta=n_theta))
    rc, rs = R.tables(n_theta)
    assert np.array_equal(c, rc) and np.array_equal(s, rs)
    assert c[0] == 16384 and s[0] == 0 and np.abs(c).max() <= 16384 and s.min() >= 0


def test_pose_affines_bit_equal_numpy():
    rng = np.random.default_rng(5)
    poses = np.concatenate([rng.uniform(-40, 40, (500, 3)), [[0, 0, 0], [1e-300, -1e300, math.pi], [3.1, -2.2, 1e6]]])
    got, want = vectorize.pose_affines(poses), R.pose_affines(poses)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))


_QUALITY = {}


def quality_case():
    """SynthBag(120) at its truth poses, defaults, window from map_window: computed once, shared, left unchanged."""
    if not _QUALITY:
        bag = synth.SynthBag(120)
        xy, off = csm.pack_scans(bag.scans)
        s = vectorize.window_spec(bag.truth, 30.0)
        _QUALITY.update(bag=bag, spec=s, out=R.vectorize(xy, off, bag.truth, s))
    return _QUALITY


def test_endpoints_bit_equal_reference():
    """Both sides call the same libm and round every operation on its own: no input has refused bit
    equality, so the comparison is on the bits."""
    for name in R.crafted():
        out, spec = run_case(name)
        s = vectorize.spec(**{f: getattr(spec, f) for f in R.FIELDS})
        got = vectorize.endpoints(s, out["records"])
        assert np.array_equal(got.view(np.uint32), out["lines"].view(np.uint32)), name
    q = quality_case()
    got = vectorize.endpoints(q["spec"], q["out"]["records"])
    assert len(got) > 10 and np.array_equal(got.view(np.uint32), q["out"]["lines"].view(np.uint32))
    # a hand-checked line: y = 20, x = 10 .. 39.  Along-coordinates a_lo - W = -39 and a_hi + 1 - W = -9 are x = 39 and x = 9
    # on the horizontal row; the fitted line runs through the centroid's y = 20; + 0.5 cell, times res
    out, spec = run_case("one_line")
    assert np.allclose(out["lines"], [[39.5 * 0.05, 20.5 * 0.05, 9.5 * 0.05, 20.5 * 0.05]], atol=1e-6)


GEOMETRIES = [(1, 1, 0), (16384, 1, 200), (1, 16384, 200), (7, 5, 35), (130, 67, 1000), (1500, 1513, 1 << 16)]


@pytest.mark.parametrize("w,h,cells", GEOMETRIES)
def test_workspace_layout(w, h, cells):
    s = vectorize.spec(width=w, height=h)
    L = vectorize.workspace_layout(s, cells)
    assert L.n_rho == 2 * w + h + 1 and L.n_along == w + 2 * h + 1
    parts = [(L.counts_offset, 4 * w * h), (L.cells_offset, 8 * cells), (L.votes_offset, 4 * s.n_theta * L.n_rho), (L.live_offset, cells)]
    at = 0
    for off, size in parts:  # aligned, in order, disjoint, inside the workspace
        assert off % 256 == 0 and off >= at and off > 0
        at = off + size
    assert at <= L.bytes == _lib.load().nhip_vectorize_workspace_bytes(C.byref(s), cells)
    assert vectorize.workspace_layout(s, cells + 1000).bytes >= L.bytes


def test_map_window():
    poses = np.array([[1.0, -2.0, 0.3], [4.26, 0.01, 1.0]])
    x0, y0, w, h = hostside.map_window(poses, 30.0, 0.05)
    assert (x0, y0) == (math.floor(-29.0 / 0.05), math.floor(-32.0 / 0.05))
    assert x0 + w - 1 == math.floor(34.26 / 0.05) and y0 + h - 1 == math.floor(30.01 / 0.05)
    assert hostside.map_window(np.zeros((0, 3)), 30.0, 0.05) == (0, 0, 1, 1)
    s = vectorize.window_spec(poses, 30.0, min_votes=7)
    assert (s.cell_x0, s.cell_y0, s.width, s.height, s.min_votes) == (x0, y0, w, h, 7)


def seg_dist(p, segs):
    a, d = segs[:, 0:2], segs[:, 2:4] - segs[:, 0:2]
    t = np.clip(((p[:, None, :] - a[None]) * d[None]).sum(2) / np.maximum((d * d).sum(1), 1e-30)[None], 0, 1)
    return np.sqrt(((p[:, None, :] - (a[None] + t[..., None] * d[None])) ** 2).sum(2)).min(1)


def test_quality_on_synthetic_bag():
    """Measured on the committed reference (SynthBag(120), truth poses, defaults): 5,400 cells, 20 segments in 16 rounds,
    nothing retired; the farthest endpoint lies 0.0750 m from a true wall; 92.86 % of the 1,708 samples taken every 0.1 m
    along the 16 walls lie within 0.1 m of a segment (the rest: wall pieces no scan of the 120 sees).
    Bounds: every endpoint within two cells, 0.1 m = half a cell's diagonal 0.035 + 3 sigma of range noise 0.03 + the
    along-line bin 0.05, rounded to the cell grid; coverage at least the measured value minus 2 %."""
    q = quality_case()
    bag, out = q["bag"], q["out"]
    lines = out["lines"].astype(np.float64)
    assert out["stats"][3] == 0 and out["stats"][1] == len(lines) >= 16
    far = seg_dist(np.concatenate([lines[:, :2], lines[:, 2:]]), bag.segs).max()
    samples = []
    for s in bag.segs:
        length = math.hypot(s[2] - s[0], s[3] - s[1])
        t = np.arange(int(length / 0.1) + 1) * 0.1 / length
        samples.append(np.stack([s[0] + t * (s[2] - s[0]), s[1] + t * (s[3] - s[1])], axis=1))
    cover = float((seg_dist(np.concatenate(samples), lines) <= 0.1).mean())
    print("farthest endpoint %.4f m, coverage %.4f, stats %s" % (far, cover, out["stats"].tolist()))
    assert far <= 0.1
    assert cover >= 0.9286 - 0.02
