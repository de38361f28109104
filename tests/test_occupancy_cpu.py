"""The occupancy grid without a GPU ("Occupancy grid"): the spec's accepted ranges through the C ABI,
the numpy reference against rays and sets worked out by hand, the PGM / YAML pair, and the quality of the method on a
synthetic bag."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

from nautilus_amd import _lib, csm, hostside, occupancy, synth
from tests import occupancy_reference as R


# ---------------------------------------------------------------- the spec through the C ABI
GOOD = dict(width=8, height=8)
EDGES = [  # (field, accepted edges, one step outside)
    ("res", [5e-324, 1.7976931348623157e308], [0.0, -0.05, float("nan"), float("inf")]),
    ("cell_x0", [-2 ** 31, 2 ** 31 - 1], []),
    ("cell_y0", [-2 ** 31, 2 ** 31 - 1], []),
    ("width", [1, 16384], [0, 16385]),
    ("height", [1, 16384], [0, 16385]),
    ("max_ray_cells", [1, 4096], [0, 4097]),
    ("min_obs", [1, 1 << 30], [0, (1 << 30) + 1]),
    ("occ_permille", [1, 1000], [0, 1001]),
    ("free_permille", [0, 649], [-1, 650]),
    ("flags", [0, _lib.NHIP_OCC_ACCUMULATE], [-1, 2]),
    ("reserved", [0], [-1, 1]),
]
WORD = {"width": "window", "height": "window"}


def call_dev(spec, n_scans=0):
    return _lib.load().nhip_occupancy_dev(None, None, None, n_scans, C.byref(spec), None, None, None, None, None)


def call_handle(spec):
    return _lib.load().nhip_occupancy(None, None, C.byref(spec), None, None, None, None)


def passed_the_spec_check(rc):
    """A good spec gets as far as the device (none here: NHIP_ERR_NODEV) or, with one, as the null pointers behind it."""
    if _lib.device_count() == 0:
        return rc == _lib.NHIP_ERR_NODEV
    return rc == _lib.NHIP_ERR_ARG and ("null pointer" in _lib.load().nhip_last_error().decode() or
                                        "bad arguments" in _lib.load().nhip_last_error().decode())


@pytest.mark.parametrize("field,good,bad", EDGES)
def test_spec_ranges_without_a_device(field, good, bad):
    lib = _lib.load()
    for v in good:
        fields = dict(GOOD, occ_permille=1, free_permille=0) if (field, v) == ("occ_permille", 1) else dict(GOOD)
        s = occupancy.spec(**dict(fields, **{field: v}))
        assert passed_the_spec_check(call_dev(s)), (field, v, lib.nhip_last_error().decode())
        assert passed_the_spec_check(call_handle(s)), (field, v)
    for v in bad:
        s = occupancy.spec(**dict(GOOD, **{field: v}))
        for rc in (call_dev(s), call_handle(s)):
            assert rc == _lib.NHIP_ERR_ARG
            assert WORD.get(field, field) in lib.nhip_last_error().decode(), (field, v)


def test_free_permille_follows_occ_permille():
    for occ in (1, 2, 500, 1000):
        assert passed_the_spec_check(call_dev(occupancy.spec(**dict(GOOD, occ_permille=occ, free_permille=occ - 1))))
        assert call_dev(occupancy.spec(**dict(GOOD, occ_permille=occ, free_permille=occ))) == _lib.NHIP_ERR_ARG
        assert "free_permille" in _lib.load().nhip_last_error().decode()


def test_bad_call_arguments_and_no_device():
    lib = _lib.load()
    s = occupancy.spec(**GOOD)
    assert call_dev(s, n_scans=-1) == _lib.NHIP_ERR_ARG and "n_scans" in lib.nhip_last_error().decode()
    assert lib.nhip_occupancy_dev(None, None, None, 0, None, None, None, None, None, None) == _lib.NHIP_ERR_ARG
    assert lib.nhip_occupancy_spec_default(None) == _lib.NHIP_ERR_ARG
    if _lib.device_count() == 0:  # (no CPU path: the compute entry points refuse, the spec functions work)
        assert call_dev(s) == _lib.NHIP_ERR_NODEV and call_handle(s) == _lib.NHIP_ERR_NODEV


def test_default_spec():
    s = occupancy.default_spec()
    assert [getattr(s, f) for f in R.FIELDS] == [0.05, 0, 0, 0, 0, 640, 1, 650, 196, 0, 0]
    assert C.sizeof(_lib.OccupancySpec) == 48
    ref = R.make_spec(width=0, height=0)
    assert all(getattr(s, f) == getattr(ref, f) for f in R.FIELDS)
    assert tuple(f for f, _ in _lib.OccupancySpec._fields_) == R.FIELDS
    assert synth.RANGE_MAX / s.res <= s.max_ray_cells - 1  # (600 cells and the discretisation)
    poses = np.array([[1.0, -2.0, 0.3], [4.26, 0.01, 1.0]])
    w = occupancy.window_spec(poses, 30.0, min_obs=3)
    assert (w.cell_x0, w.cell_y0, w.width, w.height) == hostside.map_window(poses, 30.0, 0.05) and w.min_obs == 3
    with pytest.raises(TypeError):
        occupancy.spec(band=1.0)


# ---------------------------------------------------------------- the reference against hand work
def test_rdiv_is_round_half_up_on_both_signs():
    for n in range(1, 13):
        for a in range(-60, 61):
            assert R.rdiv(a, n) == math.floor(Fraction(a, n) + Fraction(1, 2)), (a, n)
    assert R.rdiv(np.array([-3, -1, 1, 3]), 2).tolist() == [-1, 0, 1, 2]  # halves go UP: -1.5 -> -1, -0.5 -> 0


def test_rays_by_hand():
    assert R.ray_cells(4, 0).tolist() == [[0, 0], [1, 0], [2, 0], [3, 0]]
    assert R.ray_cells(-4, 0).tolist() == [[0, 0], [-1, 0], [-2, 0], [-3, 0]]
    assert R.ray_cells(0, 3).tolist() == [[0, 0], [0, 1], [0, 2]]
    assert R.ray_cells(0, -3).tolist() == [[0, 0], [0, -1], [0, -2]]
    assert R.ray_cells(3, -3).tolist() == [[0, 0], [1, -1], [2, -2]]
    assert R.ray_cells(-3, 3).tolist() == [[0, 0], [-1, 1], [-2, 2]]
    # slope 1/2: the halves at k = 1 and 3 go up -- on both signs, so the two rays are NOT mirror images
    assert R.ray_cells(4, 2).tolist() == [[0, 0], [1, 1], [2, 1], [3, 2]]
    assert R.ray_cells(-4, -2).tolist() == [[0, 0], [-1, 0], [-2, -1], [-3, -1]]
    assert R.ray_cells(0, 0).shape == (0, 2) and R.ray_cells(1, 0).tolist() == [[0, 0]] and R.ray_cells(-1, 1).tolist() == [[0, 0]]


def test_free_cells_are_distinct_connected_and_never_the_end():
    for dx in range(-12, 13):
        for dy in range(-12, 13):
            c = R.ray_cells(dx, dy)
            n = max(abs(dx), abs(dy))
            assert len(c) == n and len({tuple(v) for v in c.tolist()}) == n
            if n:
                assert c[0].tolist() == [0, 0] and [dx, dy] not in c.tolist()
                path = np.concatenate([c, [[dx, dy]]])
                step = np.abs(np.diff(path, axis=0))
                assert step.max() == 1 and (step.max(axis=1) == 1).all()  # 8-connected, the end cell included


def test_h_wins_and_per_scan_dedupe_by_hand():
    """One scan at world cell (10, 20), three beams, ends A = (+4, 0), B = (+4, +1), C = (+2, 0):
      A frees (0,0) (1,0) (2,0) (3,0); B (n = 4, slope 1/4) frees (0,0) (1,0) (2,1) (3,1); C frees (0,0) (1,0).
    H = {(4,0), (4,1), (2,0)}.  F = the union minus H = {(0,0), (1,0), (3,0), (2,1), (3,1)}: (2,0) stops C, so A's crossing of
    it is not a miss; (0,0) and (1,0), crossed by all three, count once."""
    spec = R.make_spec(cell_x0=8, cell_y0=19, width=9, height=4)
    xy, pose = R.scan_of_cells((10, 20), [(14, 20), (14, 21), (12, 20)], spec)
    grid, hits, misses, stats = R.occupancy(*R.pack([(xy, pose)]), spec)
    want_h, want_m = np.zeros((4, 9), np.int32), np.zeros((4, 9), np.int32)
    for x, y in ((4, 0), (4, 1), (2, 0)):
        want_h[1 + y, 2 + x] = 1
    for x, y in ((0, 0), (1, 0), (3, 0), (2, 1), (3, 1)):
        want_m[1 + y, 2 + x] = 1
    assert np.array_equal(hits, want_h) and np.array_equal(misses, want_m)
    assert stats.tolist() == [1, 0, 3, 0, 0, 3, 5, 36 - 8]
    assert (grid[want_h == 1] == 100).all() and (grid[want_m == 1] == 0).all() and (grid == -1).sum() == 28
    # the same beams as three scans: every scan observes the cells on its own
    scans = [R.scan_of_cells((10, 20), [e], spec) for e in ((14, 20), (14, 21), (12, 20))]
    grid, hits, misses, stats = R.occupancy(*R.pack(scans), spec)
    assert hits[1, 4] == 1 and misses[1, 4] == 1 and misses[1, 2] == 3 and misses[1, 3] == 3 and stats[:5].tolist() == [3, 0, 3, 0, 0]
    assert grid[1, 4] == -1  # 1 hit in 2 observations: neither >= 0.65 nor <= 0.196


def test_long_beams_dropped_points_and_scans():
    spec = R.make_spec(width=40, height=5, cell_y0=-2, max_ray_cells=8)
    xy, pose = R.scan_of_cells((3, 0), [(11, 0), (12, 0), (3, 0)], spec)  # 8 cells: kept; 9: long; the origin's cell: n = 0
    xy = np.concatenate([xy, [[np.nan, 0.0], [np.inf, 1.0], [1e30, 0.0]]]).astype(np.float32)
    poses = np.array([pose, (np.nan, 0.0, 0.0), (1e30, 0.0, 0.0), (0.0, 0.0, np.nan)])
    off = np.array([0, 6, 6, 6, 6], np.int32)
    grid, hits, misses, stats = R.occupancy(xy, off, poses, spec)
    assert stats[:5].tolist() == [2, 2, 2, 1, 3]  # (the empty scan with the NaN heading has a finite origin: traced)
    assert hits.sum() == 2 and hits[2, 11] == 1 and hits[2, 3] == 1 and misses.sum() == 7 and misses[2, 12] == 0
    assert stats[5:].sum() == 200


def test_classification_edges():
    spec = R.make_spec(width=8, height=1, occ_permille=500, free_permille=250, min_obs=4)
    hits = np.array([[2, 1, 1, 2, 3, 4, 0, 1]], np.int32)
    misses = np.array([[2, 3, 2, 3, 0, 4, 4, 4]], np.int32)
    #   obs        4  4  3  5  3  8  4  5
    assert R.classify(hits, misses, spec).tolist() == [[100, 0, -1, -1, -1, 100, 0, 0]]


# ---------------------------------------------------------------- the files
def test_pgm_yaml_round_trip(tmp_path):
    spec = occupancy.spec(cell_x0=-7, cell_y0=3, width=5, height=3, occ_permille=700, free_permille=100)
    grid = np.array([[100, 0, -1, 0, 0], [-1, -1, 100, 100, 0], [0, 10, -1, 100, -1]], np.int8)  # (10: no such value, unknown)
    stem = str(tmp_path / "map")
    pgm, yaml = hostside.write_occupancy_map(stem, grid, spec)
    raw = open(pgm, "rb").read()
    assert raw.startswith(b"P5\n5 3\n255\n") and len(raw) == 11 + 15
    assert list(raw[11:16]) == [254, 205, 205, 0, 205]  # image row 0 is the HIGHEST y
    assert list(raw[21:26]) == [0, 254, 205, 254, 254]
    text = open(yaml).read()
    assert "image: map.pgm\n" in text and "negate: 0\n" in text and "occupied_thresh: 0.7\n" in text and "free_thresh: 0.1\n" in text
    back, info = hostside.read_occupancy_map(stem)
    want = grid.copy()
    want[2, 1] = -1
    assert back.dtype == np.int8 and np.array_equal(back, want)
    assert info["resolution"] == 0.05 and info["origin"] == [-7 * 0.05, 3 * 0.05, 0.0] and info["negate"] == 0
    assert info["occupied_thresh"] == 0.7 and info["free_thresh"] == 0.1 and info["image"] == "map.pgm"
    with pytest.raises(ValueError):
        hostside.write_occupancy_map(stem, grid[:2], spec)


# ---------------------------------------------------------------- quality
def seg_dist(p, segs):
    a, d = segs[:, 0:2], segs[:, 2:4] - segs[:, 0:2]
    t = np.clip(((p[:, None, :] - a[None]) * d[None]).sum(2) / np.maximum((d * d).sum(1), 1e-30)[None], 0, 1)
    return np.sqrt(((p[:, None, :] - (a[None] + t[..., None] * d[None])) ** 2).sum(2)).min(1)


def test_quality_on_synthetic_bag():
    """Measured on the committed reference (SynthBag(120), truth poses, defaults, the window of every pose +- 30 m):
    3,201 occupied and 359,912 free cells of 2,269,500; the farthest occupied centre lies 0.0592 m from a true wall; 89.58 % of
    the 1,708 wall samples lie within 0.1 m of an occupied centre; every pose's own cell is free; 122,687 beams, none long.
    Bounds: no occupied centre farther than two cells (0.1 m) from a true wall -- half a cell's diagonal 0.035 + 3 sigma of
    range noise 0.03, rounded up to the cell grid; every pose's own cell free (every beam of its scan starts there, and no
    return lies that close); the share of the wall samples (every 0.1 m along the walls) within 0.1 m of an occupied
    centre at least the measured value minus 2 points -- the rest is wall that no scan of the 120 sees."""
    bag = synth.SynthBag(120)
    xy, off = csm.pack_scans(bag.scans)
    spec = occupancy.window_spec(bag.truth, 30.0)
    grid, hits, misses, stats = R.occupancy(xy, off, bag.truth, spec)
    cy, cx = np.nonzero(grid == 100)
    centres = np.stack([(cx + spec.cell_x0 + 0.5) * spec.res, (cy + spec.cell_y0 + 0.5) * spec.res], axis=1)
    far = seg_dist(centres, bag.segs).max()
    samples = []
    for s in bag.segs:
        length = math.hypot(s[2] - s[0], s[3] - s[1])
        t = np.arange(int(length / 0.1) + 1) * 0.1 / length
        samples.append(np.stack([s[0] + t * (s[2] - s[0]), s[1] + t * (s[3] - s[1])], axis=1))
    samples = np.concatenate(samples)
    d = np.sqrt(((samples[:, None, :] - centres[None]) ** 2).sum(2)).min(1)
    cover = float((d <= 0.1).mean())
    pose_cells = grid[np.floor(bag.truth[:, 1] / spec.res).astype(int) - spec.cell_y0,
                      np.floor(bag.truth[:, 0] / spec.res).astype(int) - spec.cell_x0]
    print("occupied %d, free %d, farthest occupied centre %.4f m, coverage %.4f of %d samples, stats %s"
          % (len(cx), int(stats[6]), far, cover, len(samples), stats.tolist()))
    assert stats[:5].tolist() == [120, 0, int(off[-1]), 0, 0] and stats[5:].sum() == spec.width * spec.height
    assert far <= 0.1
    assert (pose_cells == 0).all()
    assert cover >= QUALITY_MEASURED["cover"] - 0.02


QUALITY_MEASURED = {"cover": 0.8958}
