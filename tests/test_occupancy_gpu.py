"""The occupancy grid on the GPU (K14, nhip_occupancy.hip) against the numpy statement of the spec
(tests/occupancy_reference.py).  Everything the device computes after the cells is integer: hits, misses, grid and stats are
compared for EQUALITY.  The shapes are the smallest at which each loop can go wrong: one-beam scans in every direction, beams
at and one past max_ray_cells, boxes of one band and of more than a hundred, windows narrower than a word of the bitmap and
no multiple of one, rays that start, end or only pass inside the window."""
import ctypes as C

import numpy as np
import pytest

from nautilus_amd import _lib, csm, occupancy, synth
from tests import occupancy_reference as R

pytestmark = pytest.mark.gpu

BAD_MAP_SCAN_OFFSETS = 16384
NAMES = ("grid", "hits", "misses", "stats")


def product_spec(spec):
    return occupancy.spec(**{f: getattr(spec, f) for f in R.FIELDS})


def same(got, want, what=""):
    for g, w, name in zip(got, want, NAMES):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (name, what)


def check(xy, off, poses, spec, what=""):
    """one device call against the reference; returns the reference's (grid, hits, misses, stats)"""
    want = R.occupancy(xy, off, poses, spec)
    same(occupancy.occupancy_grid(xy, off, poses, product_spec(spec)), want, what)
    assert want[3][5:].sum() == spec.width * spec.height
    return want


def one_beam_scans(origin, ends, spec):
    return R.pack([R.scan_of_cells(origin, [e], spec) for e in ends])


# ---------------------------------------------------------------- 1
HAND = [(4, 0), (-4, 0), (0, 3), (0, -3), (3, 3), (-3, 3), (3, -3), (-3, -3), (0, 0), (1, 0), (-1, 0), (0, 1), (0, -1), (1, -1), (-1, 1)]


def test_hand_cases_9x7(gpu):
    """a horizontal, a vertical and a diagonal ray in each direction, n = 0 and n = 1, from the window's centre cell (4, 3)"""
    spec = R.make_spec(width=9, height=7)
    for dx, dy in HAND:
        grid, hits, misses, stats = check(*one_beam_scans((4, 3), [(4 + dx, 3 + dy)], spec), spec, (dx, dy))
        n = max(abs(dx), abs(dy))
        assert hits.sum() == 1 and hits[3 + dy, 4 + dx] == 1 and misses.sum() == n and stats.tolist() == [1, 0, 1, 0, 0, 1, n, 63 - 1 - n]
        for k in range(n):  # straight and diagonal rays: the cells in between
            assert misses[3 + k * dy // n, 4 + k * dx // n] == 1
    check(*R.pack([R.scan_of_cells((4, 3), [(4 + dx, 3 + dy) for dx, dy in HAND], spec)]), spec, "one scan")
    check(*one_beam_scans((4, 3), [(4 + dx, 3 + dy) for dx, dy in HAND], spec), spec, "a scan per beam")


# ---------------------------------------------------------------- 2
def test_max_ray_cells_edge_8(gpu):
    spec = R.make_spec(width=41, height=41, max_ray_cells=8)
    ends = [(20 + s * n, 20) for n in (8, 9) for s in (1, -1)] + [(20, 20 + s * n) for n in (8, 9) for s in (1, -1)]
    ends += [(28, 28), (29, 28), (12, 11), (12, 12)]
    grid, hits, misses, stats = check(*R.pack([R.scan_of_cells((20, 20), ends, spec)]), spec)
    assert stats[:5].tolist() == [1, 0, 6, 6, 0] and hits.sum() == 6
    check(*one_beam_scans((20, 20), ends, spec), spec)


def test_max_ray_cells_edge_4096_many_bands(gpu):
    """16384 x 3 window, two scans: beams of exactly 4096 and 4097 cells on each axis.  The box has 8193 rows of 257 words:
    more than a hundred bands, of which the window's three rows fall into one."""
    spec = R.make_spec(width=16384, height=3, max_ray_cells=4096)
    a = R.scan_of_cells((8192, 1), [(8192 + 4096, 1), (8192 - 4096, 1), (8192 + 4097, 1), (8192 - 4097, 1), (8192, 1 + 4096),
                                    (8192, 1 - 4096), (8192, 1 + 4097), (8192, 1 - 4097), (8192 + 4096, 2)], spec)
    b = R.scan_of_cells((5000, 4000), [(5000 + 4096, 4000 - 4096), (5000 - 4096, 4000 - 4000), (5000 - 3, 4000 - 4096),
                                       (5000 + 2000, 4000 - 4097)], spec)
    grid, hits, misses, stats = check(*R.pack([a, b]), spec)
    assert stats[:5].tolist() == [2, 0, 8, 5, 0]
    assert misses[1, 4096 + 1:8192].all() and misses[1, 8192:8192 + 4096].all() and hits[1, 4096] == 1 and hits[1, 8192 + 4096] == 1
    assert misses[:, 8192].tolist() == [1, 1, 1] and misses.sum() > 8192 + 6


# ---------------------------------------------------------------- 3
def test_every_direction_625_scans(gpu):
    """(dx, dy) over [-12, 12]^2, a scan per beam, origins 32 cells apart: every octant, both signs of the floor division,
    exact halves; no two rays share a cell, so every ray is compared on its own"""
    spec = R.make_spec(width=800, height=800)
    scans = []
    for j, dy in enumerate(range(-12, 13)):
        for i, dx in enumerate(range(-12, 13)):
            o = (16 + 32 * i, 16 + 32 * j)
            scans.append(R.scan_of_cells(o, [(o[0] + dx, o[1] + dy)], spec))
    grid, hits, misses, stats = check(*R.pack(scans), spec)
    assert stats[:5].tolist() == [625, 0, 625, 0, 0] and hits.max() == 1 and misses.max() == 1
    assert misses.sum() == sum(max(abs(dx), abs(dy)) for dx in range(-12, 13) for dy in range(-12, 13))


def test_more_scans_than_workgroups(gpu):
    """1,030 one-beam scans: the trace kernel's grid holds 1,024 workgroups along the scans, the rest come round again"""
    spec = R.make_spec(width=520, height=140)
    scans = []
    for i in range(1030):
        o = (4 + 8 * (i % 64), 4 + 8 * (i // 64))
        scans.append(R.scan_of_cells(o, [(o[0] + i % 7 - 3, o[1] + i % 5 - 2)], spec))
    grid, hits, misses, stats = check(*R.pack(scans), spec)
    assert stats[:5].tolist() == [1030, 0, 1030, 0, 0] and hits.sum() == 1030 and hits.max() == 1
    assert hits[132 + 1029 % 5 - 2, 44 + 1029 % 7 - 3] == 1  # (scan 1,029, at (44, 132))


@pytest.mark.parametrize("edge", [False, True])
def test_long_rays_in_random_directions(gpu, edge):
    """64 beams with n in 600 .. 640, a scan each from one origin: mid-cell, and on a cell edge (tx an exact multiple of res)"""
    rng = np.random.default_rng(11)
    spec = R.make_spec(width=1400, height=1400, cell_x0=-700, cell_y0=-700)
    n = rng.integers(600, 641, 64)
    minor = np.array([rng.integers(-k, k + 1) for k in n])
    sign = rng.choice([-1, 1], 64)
    swap = rng.random(64) < 0.5
    d = np.where(swap[:, None], np.stack([minor, sign * n], axis=1), np.stack([sign * n, minor], axis=1))
    pose = (3 * spec.res, -2 * spec.res, 0.0) if edge else R.cell_centre((3, -3), spec) + (0.0,)
    xy = ((d + (0.5 if edge else 0.0)) * spec.res).astype(np.float32)  # (relative to the pose: ends at cell centres)
    scans = [(xy[i:i + 1], pose) for i in range(64)]
    grid, hits, misses, stats = check(*R.pack(scans), spec)
    assert stats[0] == 64 and stats[2] + stats[3] == 64 and stats[2] >= 32 and misses.max() >= 32  # (the origin's cell: every scan)
    check(*R.pack([(xy, pose)]), spec, "one scan")


# ---------------------------------------------------------------- 4
def test_per_scan_dedupe_and_h_wins(gpu):
    spec = R.make_spec(width=12, height=6)
    o = (1, 2)
    # two beams of one scan share their first cells: once
    grid, hits, misses, stats = check(*R.pack([R.scan_of_cells(o, [(9, 2), (9, 3)], spec)]), spec)
    assert misses[2, 1] == 1 and misses[2, 2] == 1 and misses.max() == 1
    # the same two beams in two scans: twice
    grid, hits, misses, stats = check(*one_beam_scans(o, [(9, 2), (9, 3)], spec), spec)
    assert misses[2, 1] == 2 and misses[2, 2] == 2
    # beam A ends on a cell that beam B of the same scan crosses: hit 1, miss 0
    grid, hits, misses, stats = check(*R.pack([R.scan_of_cells(o, [(5, 2), (9, 2)], spec)]), spec)
    assert hits[2, 5] == 1 and misses[2, 5] == 0 and misses[2, 6] == 1 and grid[2, 5] == 100
    # across two scans: hit 1, miss 1
    grid, hits, misses, stats = check(*one_beam_scans(o, [(5, 2), (9, 2)], spec), spec)
    assert hits[2, 5] == 1 and misses[2, 5] == 1 and grid[2, 5] == -1
    # the same end cell twice in one scan: one hit
    grid, hits, misses, stats = check(*R.pack([R.scan_of_cells(o, [(5, 4), (5, 4), (5, 4)], spec)]), spec)
    assert hits[4, 5] == 1 and hits.sum() == 1 and stats[2] == 3


# ---------------------------------------------------------------- 5
@pytest.mark.parametrize("w,h", [(1, 5), (31, 5), (32, 5), (33, 5), (130, 67)])
@pytest.mark.parametrize("x0,y0", [(0, 0), (-50, -20)])
def test_window_seams(gpu, w, h, x0, y0):
    """the origin outside the window, the end outside, both outside with the ray crossing, a ray that only touches the corner
    cell (0, 0); world cells = window cells + (x0, y0)"""
    spec = R.make_spec(width=w, height=h, cell_x0=x0, cell_y0=y0)
    at = lambda c: (c[0] + x0, c[1] + y0)
    rays = [((-3, 2), (w + 2, 2)), ((w // 2, h // 2), (w + 5, h // 2 + 1)), ((-4, -4), (w // 2, h // 2)), ((-2, 2), (2, -2)),
            ((w - 1, h + 6), (w - 1, -6)), ((w + 3, h + 3), (w - 4, h - 4)), ((w + 1, 0), (w + 9, 3))]
    scans = [R.scan_of_cells(at(o), [at(e)], spec) for o, e in rays]
    grid, hits, misses, stats = check(*R.pack(scans), spec)
    assert stats[:5].tolist() == [7, 0, 7, 0, 0]
    assert misses[2, :].all() and misses[0, 0] >= 1 and misses[:, w - 1].all()
    corner = R.occupancy(*R.pack(scans[3:4]), spec)
    assert corner[2].sum() == 1 and corner[2][0, 0] == 1 and corner[1].sum() == 0
    check(*R.pack([(np.concatenate([s[0] for s in scans[:3]]), scans[0][1])]), spec, "one scan, its origin outside")


@pytest.mark.parametrize("sx,sy", [(1, -1), (-1, 1)])
def test_window_at_two_to_the_thirty(gpu, sx, sy):
    """cell_x0, cell_y0 near +-2^30: a float has 24 bits, so the cells there lie 80 apart -- both sides round alike"""
    big = 1 << 30
    spec = R.make_spec(width=700, height=700, cell_x0=sx * big - 300, cell_y0=sy * big - 300)
    pose = (sx * big * 0.05, sy * big * 0.05, 0.0)
    xy = np.array([[8.0, 0.0], [12.0, 8.0], [-8.0, -12.0], [20.0, 0.0], [0.0, 4.0], [1.0, 1.0]], np.float32)
    grid, hits, misses, stats = check(xy, np.array([0, 6], np.int32), np.array([pose]), spec)
    assert stats[:5].tolist() == [1, 0, 6, 0, 0] and hits.sum() >= 3 and misses.sum() > 300


# ---------------------------------------------------------------- 6
def test_fan_across_every_band_and_word(gpu):
    """360 rays of length 640 from one origin at the default max_ray_cells: the box is 1281 rows of 41 words, several bands;
    the fan crosses every band boundary and every word boundary of a row.  A second scan 7, 5 cells away overlaps it; the
    window cuts both boxes on all four sides."""
    spec = R.make_spec(width=1270, height=1250, cell_x0=-630, cell_y0=-620)
    a = np.radians(np.arange(360))
    d = np.stack([np.cos(a), np.sin(a)], axis=1)
    ends = np.rint(d * (640.0 / np.abs(d).max(axis=1))[:, None]).astype(int)
    assert (np.abs(ends).max(axis=1) == 640).all()
    scans = [R.scan_of_cells((0, 0), ends, spec), R.scan_of_cells((7, 5), ends + [7, 5], spec)]
    grid, hits, misses, stats = check(*R.pack(scans), spec)
    assert stats[:5].tolist() == [2, 0, 720, 0, 0] and misses.max() == 2 and misses.sum() > 100000
    # the whole box inside a window: every end cell is there
    spec = R.make_spec(width=1300, height=1290, cell_x0=-650, cell_y0=-645)
    grid, hits, misses, stats = check(*R.pack(scans[:1]), spec)
    assert hits.sum() == len({tuple(e) for e in ends.tolist()})


# ---------------------------------------------------------------- 7
def bad_input_case():
    spec = R.make_spec(width=40, height=9, cell_y0=-4, max_ray_cells=16)
    good, pose = R.scan_of_cells((3, 0), [(11, 0), (12, 2), (3, 0), (30, 0)], spec)
    dirty = np.concatenate([good[:2], [[np.nan, 0.0], [np.inf, 1.0], [0.0, -np.inf], [1e30, 0.0]], good[2:]]).astype(np.float32)
    return spec, good, dirty, pose


def test_bad_points_and_poses(gpu):
    spec, good, dirty, pose = bad_input_case()
    empty = np.zeros((0, 2), np.float32)
    scans = [(good, pose), (empty, pose), (dirty, pose), (good, (np.nan, 0.0, 0.0)), (good, (0.0, 1e30, 0.0)),
             (good, (0.1, 0.1, np.nan)), (good, (np.inf, 0.0, 0.0))]
    grid, hits, misses, stats = check(*R.pack(scans), spec)
    assert stats[:5].tolist() == [4, 3, 6, 2, 8]  # (a NaN heading: a finite origin, every point dropped)
    assert hits[4, 11] == 2 and hits[4, 3] == 2 and hits[4, 30] == 0


def test_bad_scan_offsets_are_an_empty_scan(gpu):
    """scan 1's end lies before its start: NhipError of kind 16384; the other scans are traced as ever"""
    import torch
    spec, good, dirty, pose = bad_input_case()
    xy = np.concatenate([good, dirty, good])
    poses = np.array([pose, pose, (0.5, 0.1, 0.3)])
    off = np.array([0, 4, 2, len(xy)], np.int32)
    s = product_spec(spec)
    with pytest.raises(_lib.NhipError, match="scan offset"):
        occupancy.occupancy_grid(xy, off, poses, s)
    # the raw call: the planes of the other scans, the record of the first bad offset
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_hits, d_misses = (torch.full((spec.height, spec.width), 77, dtype=torch.int32, device=dev) for _ in range(2))
    d_grid = torch.zeros((spec.height, spec.width), dtype=torch.int8, device=dev)
    d_stats = torch.zeros(8, dtype=torch.int64, device=dev)
    lib = _lib.load()
    d_xy, d_off, d_aff = t(xy), t(off), t(occupancy.pose_affines(poses))  # (named: they live until the stream has drained)
    rc = lib.nhip_occupancy_dev(d_xy.data_ptr(), d_off.data_ptr(), d_aff.data_ptr(), 3, C.byref(s),
                                d_hits.data_ptr(), d_misses.data_ptr(), d_grid.data_ptr(), d_stats.data_ptr(), None)
    info = (C.c_int32 * 4)()
    rc_status = lib.nhip_dev_status(None, info)
    assert rc == 0 and rc_status == _lib.NHIP_ERR_ARG and b"nhip_occupancy_dev" in lib.nhip_last_error(), lib.nhip_last_error()
    assert list(info) == [BAD_MAP_SCAN_OFFSETS, BAD_MAP_SCAN_OFFSETS, 2, 2]
    want = R.occupancy(xy, off, poses, spec)
    assert want[3][:2].tolist() == [2, 1]
    same((d_grid.cpu().numpy(), d_hits.cpu().numpy(), d_misses.cpu().numpy(), d_stats.cpu().numpy()), want)
    # a second call without that scan: the same planes
    keep = np.concatenate([xy[0:4], xy[2:]])
    again = check(keep, np.array([0, 4, 4 + len(xy) - 2], np.int32), poses[[0, 2]], spec)
    assert np.array_equal(again[1], want[1]) and np.array_equal(again[2], want[2])
    with pytest.raises(_lib.NhipError, match="scan offset"):
        occupancy.occupancy_grid(xy, np.array([-1, 4, len(xy)], np.int32), poses[:2], s)


def test_no_scans(gpu):
    spec = R.make_spec(width=33, height=5)
    grid, hits, misses, stats = check(np.zeros((0, 2), np.float32), np.array([0], np.int32), np.zeros((0, 3)), spec)
    assert (grid == -1).all() and not hits.any() and not misses.any() and stats.tolist() == [0, 0, 0, 0, 0, 0, 0, 165]


# ---------------------------------------------------------------- 8
@pytest.mark.parametrize("w,h", [(8, 1), (7, 3), (64, 5), (130, 67)])
def test_classification_edges(gpu, w, h):
    """planes preset through the accumulate form, no scans: 1000 hits == occ_permille obs and one hit less, 1000 hits ==
    free_permille obs and one more, obs == min_obs - 1 and min_obs; occ 500 / free 250, so small counts hit equality.  The
    widths exercise the 16-byte groups of the classification and the cells behind the last whole group."""
    import torch
    edges_h = np.array([2, 1, 1, 2, 3, 4, 0, 1, 1, 2, 50, 49, 25, 26, 2 ** 30, 0, 3, 2], np.int32)
    edges_m = np.array([2, 3, 2, 3, 0, 4, 4, 4, 3, 6, 50, 51, 75, 74, 2 ** 30, 2 ** 31 - 1, 0, 1], np.int32)
    rng = np.random.default_rng(w * 1000 + h)
    hits = rng.integers(0, 6, (h, w)).astype(np.int32)
    misses = rng.integers(0, 9, (h, w)).astype(np.int32)
    k = min(len(edges_h), w * h)
    hits.reshape(-1)[:k], misses.reshape(-1)[:k] = edges_h[:k], edges_m[:k]
    hits.reshape(-1)[-1], misses.reshape(-1)[-1] = 2, 2
    for min_obs in (1, 3, 5, 4):
        spec = R.make_spec(width=w, height=h, occ_permille=500, free_permille=250, min_obs=min_obs, flags=R.ACCUMULATE)
        want = R.occupancy(np.zeros((0, 2), np.float32), np.array([0], np.int32), np.zeros((0, 3)), spec, planes=(hits, misses))
        planes = tuple(torch.from_numpy(p.copy()).to("cuda:0") for p in (hits, misses))
        got = occupancy.occupancy_grid(np.zeros((0, 2), np.float32), np.array([0], np.int32), np.zeros((0, 3)), product_spec(spec),
                                       planes=planes)
        same(got, want, min_obs)
        assert np.array_equal(planes[0].cpu().numpy(), hits) and np.array_equal(planes[1].cpu().numpy(), misses)
    if (w, h) == (8, 1):
        assert want[0].tolist() == [[100, 0, -1, -1, -1, 100, 0, 100]]  # min_obs 4; the last cell was set to 2, 2


# ---------------------------------------------------------------- 9, 10
@pytest.fixture(scope="module")
def bag40():
    """SynthBag(40) at its odometry poses, defaults, the window of every pose +- 30 m; the reference once"""
    bag = synth.SynthBag(40)
    xy, off = csm.pack_scans(bag.scans)
    s = occupancy.window_spec(bag.odom, 30.0)
    return xy, off, bag.odom, s, R.occupancy(xy, off, bag.odom, s)


def test_accumulate(gpu, bag40):
    """scans 0 .. 19, then 20 .. 39 onto the same planes: the map of 0 .. 39; without the flag the second call forgets the first"""
    import torch
    xy, off, poses, s, want = bag40
    first = (xy[:off[20]], off[:21], poses[:20])
    second = (xy[off[20]:], off[20:] - off[20], poses[20:])
    planes = tuple(torch.full((s.height, s.width), 99, dtype=torch.int32, device="cuda:0") for _ in range(2))
    a = occupancy.occupancy_grid(*first, s, planes=planes)  # (no flag: the 99s are cleared)
    same(a, R.occupancy(*first, s), "first half")
    acc = occupancy.spec(**dict({f: getattr(s, f) for f in R.FIELDS}, flags=_lib.NHIP_OCC_ACCUMULATE))
    b = occupancy.occupancy_grid(*second, acc, planes=planes)
    for k in (0, 1, 2):
        assert np.array_equal(b[k], want[k]), NAMES[k]
    assert b[3][5:].tolist() == want[3][5:].tolist() and (a[3][:5] + b[3][:5]).tolist() == want[3][:5].tolist()
    assert np.array_equal(planes[0].cpu().numpy(), want[1])
    c = occupancy.occupancy_grid(*second, s, planes=planes)
    same(c, R.occupancy(*second, s), "second half alone")
    assert not np.array_equal(c[1], want[1])


def test_three_entry_points_agree_and_repeat(gpu, bag40):
    import torch
    xy, off, poses, s, want = bag40
    assert want[3][:5].tolist() == [40, 0, int(off[-1]), 0, 0] and want[3][5] > 1000 and want[3][6] > 100000
    runs = [occupancy.occupancy_grid(xy, off, poses, s), occupancy.occupancy_grid(xy, off, poses, s)]
    d_xy, d_off = torch.from_numpy(xy).to("cuda:0"), torch.from_numpy(off).to("cuda:0")
    runs.append(occupancy.occupancy_grid_on_device(d_xy, d_off, 40, poses, s))
    scans = csm.ScanTable(xy, off)
    runs.append(occupancy.occupancy_grid_on_handle(scans, poses, s))
    scans.close()
    for r in runs:
        same(r, want)
        for k in range(4):
            assert r[k].tobytes() == runs[0][k].tobytes()
