"""Map windows on the GPU (K20): cells, windows, offsets and stats bit-equal to the per-cell statement of the spec
(tests/localize_reference.py) on every crafted map, the two capacity rules, buffers at the least alignment the header promises,
the host form, the tables built on device windows, and HipBackend.localize end to end against the host route."""
import ctypes as C
import math

import numpy as np
import pytest

from nautilus_amd import _lib, csm, hostside, localize, synth
from tests import localize_reference as R

pytestmark = pytest.mark.gpu

CASES = R.shared_cases()
DEV = "cuda:0"


def product_spec(spec):
    s = localize.default_spec()
    for f in R.FIELDS:
        setattr(s, f, getattr(spec, f))
    return s


def status(lib, torch):
    info = (C.c_int32 * 4)()
    rc = lib.nhip_dev_status(C.c_void_p(torch.cuda.current_stream().cuda_stream), info)
    return rc, list(info)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_cells_and_windows_equal_reference(gpu, case):
    name, grid, spec, origins = case
    mw = product_spec(spec)
    want_cells, want = R.shared_results()[name]
    row_ptr, cols, stats = localize.map_cells(grid, mw, DEV)
    R.same_cells((row_ptr, cols), want_cells, name)
    assert stats.tolist() == [want_cells[2], 0, 0, 0, 0, 0, 0, 0]
    got = localize.windows(grid, mw, origins, DEV)
    R.same(got, want, name)
    R.same(localize.windows(grid, mw, origins, DEV), got, name + " (again: the same bits)")
    R.same(localize.windows_host_form(grid, mw, origins, int(want[1][-1])), want, name + " (host form)")


def test_query_counts_and_duplicates(gpu):
    name, grid, spec, origins = R.many_queries_case()
    mw = product_spec(spec)
    for n in (0, 1, 2500):
        want = R.map_windows(grid, spec, origins[:n])
        R.same(localize.windows(grid, mw, origins[:n], DEV), want, "%s, %d" % (name, n))
        R.same(localize.windows_host_form(grid, mw, origins[:n], int(want[1][-1])), want, "%s, %d (host form)" % (name, n))
    assert len(np.unique(origins, axis=0)) < 400  # (duplicates: equal windows at different offsets)


def test_capacities_exact_and_one_short(gpu):
    import torch
    lib = _lib.load()
    name, grid, spec, origins = R.many_queries_case()
    mw = product_spec(spec)
    want = R.map_windows(grid, spec, origins)
    n_occ, total, n = int(want[2][0]), int(want[2][2]), len(origins)
    d_grid = torch.from_numpy(grid).to(DEV)
    d_org = torch.from_numpy(origins).to(DEV)

    def run(max_cells, capacity):
        d_row_ptr, d_cols, d_stats = localize.map_cells_on_device(d_grid, mw, max_cells)
        d_cols.fill_(-7)
        lib.nhip_mapwin_cells_dev(d_grid.data_ptr(), C.byref(mw), max_cells, d_row_ptr.data_ptr(), d_cols.data_ptr(), d_stats.data_ptr(),
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
        d_xy, d_off, d_stats = localize.windows_on_device(d_row_ptr, d_cols, mw, d_org, n, capacity, d_stats)
        rc, info = status(lib, torch)
        off = d_off.cpu().numpy()
        return rc, info, d_row_ptr.cpu().numpy(), d_cols.cpu().numpy(), d_xy[:int(off[-1])].cpu().numpy(), off, d_stats.cpu().numpy()

    rc, info, row_ptr, cols, xy, off, stats = run(n_occ, total)  # exactly enough
    assert rc == _lib.NHIP_OK and info[0] == 0
    R.same((xy, off, stats), want, name)
    rc, info, row_ptr, cols, xy, off, stats = run(n_occ - 1, total)  # one cell short: nothing packed, an empty map downstream
    assert rc == _lib.NHIP_ERR_ARG and info[:4] == [localize.KIND_CELLS, localize.KIND_CELLS, n_occ, spec.height]
    assert b"max_cells" in lib.nhip_last_error()
    assert not row_ptr.any() and (cols == -7).all() and not off.any() and stats.tolist() == [n_occ, n, 0, n, 0, 1, 0, 0]
    R.same((xy, off, stats), R.map_windows(grid, spec, origins, max_cells=n_occ - 1), name + " (cells short)")
    rc, info, row_ptr, cols, xy, off, stats = run(n_occ, total - 1)  # one point short: nothing stored
    assert rc == _lib.NHIP_ERR_ARG and info[:4] == [localize.KIND_POINTS, localize.KIND_POINTS, total, n]
    assert b"out_capacity" in lib.nhip_last_error()
    R.same_cells((row_ptr, cols), R.map_cells(grid, spec), name)
    R.same((xy, off, stats), R.map_windows(grid, spec, origins, capacity=total - 1), name + " (points short)")
    rc, info, row_ptr, cols, xy, off, stats = run(n_occ, 0)
    assert rc == _lib.NHIP_ERR_ARG and info[2] == total and not off.any() and stats[6] == 1
    with pytest.raises(_lib.NhipError, match="out_capacity"):
        localize.windows(grid, mw, origins, DEV, capacity=total - 1)
    rc, info, row_ptr, cols, xy, off, stats = run(n_occ + 5, total + 11)  # later calls are not affected
    assert rc == _lib.NHIP_OK and info[0] == 0
    R.same((xy, off, stats), want, name + " (after the refusals)")
    # the host form sizes the cell list itself; only the points can fail to fit
    hxy, hoff, hstats = np.zeros((total, 2), np.float32), np.zeros(n + 1, np.int32), np.zeros(8, np.int64)
    assert lib.nhip_map_windows(_lib.ptr(grid), C.byref(mw), _lib.ptr(origins), n, _lib.ptr(hxy), total - 1, _lib.ptr(hoff),
                                _lib.ptr(hstats)) == _lib.NHIP_OK
    assert not hoff.any() and hstats[6] == 1 and not hxy.any() and lib.nhip_dev_status(None, None) == _lib.NHIP_ERR_ARG


def test_buffers_at_the_least_alignment(gpu):
    """d_grid at an odd address, the int32 arrays and the workspace on 4 bytes, out_xy and the stats on 8"""
    import torch
    lib = _lib.load()
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for name, grid, spec, origins in [CASES[k] for k in (10, 21, 22, 46)] + [c for c in CASES if c[0].startswith("counted rows side 300")]:
        mw = product_spec(spec)
        want_cells, want = R.shared_results()[name]
        n_occ, total, n, cells = want_cells[2], int(want[1][-1]), len(origins), grid.size
        for shift in (1, 3, 13):
            raw = torch.zeros(cells + 64, dtype=torch.int8, device=DEV)
            d_grid = raw[shift:shift + cells]
            d_grid.copy_(torch.from_numpy(grid.reshape(-1)))
            ints = torch.full((spec.height + 1 + max(n_occ, 1) + 2 * n + n + 1 + 64,), -9, dtype=torch.int32, device=DEV)
            a = 1
            d_row_ptr = ints[a:a + spec.height + 1]
            a += spec.height + 1 + 2
            d_cols = ints[a:a + max(n_occ, 1)]
            a += max(n_occ, 1) + 2
            d_org = ints[a:a + 2 * n]
            d_org.copy_(torch.from_numpy(origins.reshape(-1)))
            a += 2 * n + 1
            d_off = ints[a:a + n + 1]
            words = torch.zeros(8 + 1, dtype=torch.int64, device=DEV)
            d_stats = words[1:]
            pts = torch.zeros((total + 2, 2), dtype=torch.float32, device=DEV)
            d_xy = pts[1:]
            ws = lib.nhip_mapwin_workspace_bytes(n)
            wsb = torch.zeros(ws + 8, dtype=torch.uint8, device=DEV)
            d_ws = wsb[4:]
            assert d_grid.data_ptr() % 2 == 1 and d_row_ptr.data_ptr() % 8 == 4 and d_xy.data_ptr() % 16 == 8 and d_stats.data_ptr() % 16 == 8
            _lib.check(lib.nhip_mapwin_cells_dev(d_grid.data_ptr(), C.byref(mw), n_occ, d_row_ptr.data_ptr(), d_cols.data_ptr(),
                                                 d_stats.data_ptr(), sp))
            _lib.check(lib.nhip_mapwin_gather_dev(d_row_ptr.data_ptr(), d_cols.data_ptr(), C.byref(mw), d_org.data_ptr(), n, d_xy.data_ptr(),
                                                  total, d_off.data_ptr(), d_stats.data_ptr(), d_ws.data_ptr(), ws, sp))
            _lib.check(lib.nhip_dev_status(sp, None))
            R.same_cells((d_row_ptr.cpu().numpy(), d_cols[:n_occ].cpu().numpy()), want_cells, name)
            R.same((d_xy[:total].cpu().numpy(), d_off.cpu().numpy(), d_stats.cpu().numpy()), want, "%s, shift %d" % (name, shift))
            assert (ints[0] == -9).all() and (pts[0] == 0).all() and (pts[total + 1:] == 0).all() and int(words[0]) == 0
    # a misaligned out_xy or stats block is refused
    assert lib.nhip_mapwin_cells_dev(d_grid.data_ptr(), C.byref(mw), n_occ, d_row_ptr.data_ptr(), d_cols.data_ptr(), d_stats.data_ptr() + 4,
                                     sp) == _lib.NHIP_ERR_ARG
    assert lib.nhip_mapwin_gather_dev(d_row_ptr.data_ptr(), d_cols.data_ptr(), C.byref(mw), d_org.data_ptr(), n, d_xy.data_ptr() + 4, total,
                                      d_off.data_ptr(), d_stats.data_ptr(), d_ws.data_ptr(), ws, sp) == _lib.NHIP_ERR_ARG


def test_row_ptr_entries_are_checked(gpu):
    """a row_ptr whose entries are not rows of the cell list: those rows are empty, reported, and nothing is read past the list"""
    import torch
    lib = _lib.load()
    spec = R.make_spec(cell_x0=0, cell_y0=0, width=16, height=4, side=8)
    mw = product_spec(spec)
    grid = np.full((4, 16), 100, np.int8)
    d_row_ptr, d_cols, d_stats = localize.map_cells_on_device(torch.from_numpy(grid).to(DEV), mw)
    bad = d_row_ptr.clone()
    bad[2] = 10 ** 9  # row 1 ends and row 2 starts far beyond the 64 cells
    d_org = torch.tensor([[4, 2]], dtype=torch.int32, device=DEV)
    d_xy, d_off, d_stats = localize.windows_on_device(bad, d_cols, mw, d_org, 1, 64, d_stats)
    rc, info = status(lib, torch)
    assert rc == _lib.NHIP_ERR_ARG and info[1] == localize.KIND_CELLS and info[2] == 10 ** 9 and info[3] in (1, 2)
    assert d_off.cpu().numpy().tolist() == [0, 16]  # rows 0 and 3 of the map: 8 cells each
    d_xy, d_off, d_stats = localize.windows_on_device(d_row_ptr, d_cols, mw, d_org, 1, 64, d_stats)
    assert status(lib, torch)[0] == _lib.NHIP_OK and d_off.cpu().numpy().tolist() == [0, 32]


def test_tables_of_device_windows(gpu):
    """the tables built on device windows are those built on host windows, and their hit raster is the crop of the map"""
    name, grid, spec, origins = next(c for c in CASES if c[0].startswith("values 130x130 occ_min 100"))
    gs = csm.grid_spec(2.0, 0.05, 2.0, 1e-10, 8)  # side 80
    side = csm.grid_layout(gs).side
    occ = R.make_spec(res=0.05, cell_x0=spec.cell_x0, cell_y0=spec.cell_y0, width=spec.width, height=spec.height)
    mw = localize.spec(occ, gs)
    org = np.array([[spec.cell_x0 + 65, spec.cell_y0 + 65], [spec.cell_x0 + 3, spec.cell_y0 + 120], [spec.cell_x0 + 129, spec.cell_y0],
                    [spec.cell_x0 - 500, spec.cell_y0]], np.int32)
    dxy, doff, _ = localize.windows(grid, mw, org, DEV)
    hxy, hoff, _ = hostside.map_windows(grid, mw, org)
    assert dxy.tobytes() == hxy.tobytes() and np.array_equal(doff, hoff) and doff[-1] > 500
    ids = np.arange(len(org), dtype=np.int32)
    gd, gh = csm.LikelihoodGrids(csm.ScanTable(dxy, doff), ids, gs), csm.LikelihoodGrids(csm.ScanTable(hxy, hoff), ids, gs)
    world = np.zeros((spec.height + 2 * side, spec.width + 2 * side), bool)  # the map's occupied cells with a margin of a window
    world[side:side + spec.height, side:side + spec.width] = grid >= 100
    for k, (ox, oy) in enumerate(org.tolist()):
        assert gd.download(k).tobytes() == gh.download(k).tobytes()
        hits = gd.hits(k)
        assert np.array_equal(hits, gh.hits(k))
        y, x = oy - side // 2 - spec.cell_y0 + side, ox - side // 2 - spec.cell_x0 + side
        crop = world[y:y + side, x:x + side] if 0 <= x and 0 <= y and x < world.shape[1] else np.zeros((side, side), bool)
        assert np.array_equal(hits.astype(bool), crop), k
        assert hits.sum() == doff[k + 1] - doff[k]


# ---------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def mapped_bag(gpu):
    """SynthBag(120), the map of its 60 even scans at their truth poses (HipBackend.occupancy_grid, the defaults), eight queries"""
    from nautilus_amd import occupancy, posegraph
    bag = synth.SynthBag(120)
    even = list(range(0, 120, 2))
    xy, off = csm.pack_scans([bag.scans[i] for i in even])
    occ = occupancy.window_spec(bag.truth, 30.0)
    be = posegraph.HipBackend(DEV)
    grid = be.occupancy_grid(bag.truth[even], spec=occ, xy=xy, offsets=off)[0]
    q = [1, 17, 33, 49, 65, 81, 97, 113]
    qxy, qoff = csm.pack_scans([bag.scans[i] for i in q])
    return bag, be, grid, occ, q, qxy, qoff


def test_localize_small_spec_equals_host_route(mapped_bag):
    bag, be, grid, occ, q, qxy, qoff = mapped_bag
    gs, srch = csm.grid_spec(6.0, 0.05, 2.0, 1e-10, 8), csm.search_spec(21, 17, 17, math.radians(1.0))
    d = np.linspace(0.0, 2.0 * math.pi, len(q), endpoint=False)
    priors = bag.truth[q] + np.stack([0.21 * np.cos(d), 0.21 * np.sin(d), np.full(len(q), math.radians(4.3))], axis=1)
    priors = np.concatenate([priors, priors[:3] + [0.001, 0.002, 0.0]])  # (three queries share their origin cell with another)
    xy2, off2 = csm.pack_scans([bag.scans[i] for i in q + q[:3]])
    got = be.localize(xy2, off2, priors, grid, occ, grid_spec=gs, search=srch)
    want = hostside.localize(be, xy2, off2, priors, grid, occ, grid_spec=gs, search=srch)
    assert len(np.unique(got["origins"], axis=0)) < len(priors)
    assert got["records"].tobytes() == want["records"].tobytes() and got["poses"].tobytes() == want["poses"].tobytes()
    assert np.array_equal(got["origins"], want["origins"]) and np.array_equal(got["points_per_window"], want["points_per_window"])
    assert not got["rejected"].any() and got["points_per_window"].min() > 50
    # (no bound against the truth here: a 6 m table sees the nearest walls only, and a scan slides along a single wall -- the
    #  full-spec test holds the poses to the truth.  What must hold: every pose is a pose of its prior's lattice)
    e = got["poses"] - priors
    assert np.abs(e[:, :2]).max() <= (8 + 1) * 0.05 and np.degrees(np.abs(csm.angle_mod(e[:, 2]))).max() <= 10.0 + 1e-9
    # one slot at a time gives the same records: the batches are independent
    one = be.localize(xy2, off2, priors, grid, occ, grid_spec=gs, search=srch, max_slots=1)
    assert one["records"].tobytes() == got["records"].tobytes()
    # the gated call rejects what the ungated score says it should, and keeps the other records as they are
    score = got["records"]["score"]
    gate = float(np.sort(score)[len(score) // 2]) + 1e-4
    gated = be.localize(xy2, off2, priors, grid, occ, grid_spec=gs, search=srch, min_score=gate)
    assert np.array_equal(gated["rejected"], score < gate) and 0 < gated["rejected"].sum() < len(score)
    keep = ~gated["rejected"]
    assert gated["records"][keep].tobytes() == got["records"][keep].tobytes() and gated["poses"][keep].tobytes() == got["poses"][keep].tobytes()
    assert np.isnan(gated["poses"][~keep]).all() and (gated["records"]["itheta"][~keep] == -1).all()


def test_localize_full_spec(mapped_bag):
    """eight queries on config #2's table and lattice, priors 1 m and 10.4 degrees off: the device path equals the host route
    bit for bit and the poses are within the CPU test's bounds of the truth"""
    bag, be, grid, occ, q, qxy, qoff = mapped_bag
    d = np.random.default_rng(3).uniform(0.0, 2.0 * math.pi, len(q))
    priors = bag.truth[q] + np.stack([np.cos(d), np.sin(d), np.full(len(q), math.radians(10.4))], axis=1)
    got = be.localize(qxy, qoff, priors, grid, occ)
    want = hostside.localize(be, qxy, qoff, priors, grid, occ)
    assert got["records"].tobytes() == want["records"].tobytes() and got["poses"].tobytes() == want["poses"].tobytes()
    assert np.array_equal(got["points_per_window"], want["points_per_window"]) and got["points_per_window"].min() > 2000
    e = got["poses"] - bag.truth[q]
    pos, ang = np.hypot(e[:, 0], e[:, 1]), np.degrees(np.abs(csm.angle_mod(e[:, 2])))
    print("full spec: position error max %.3f m, heading error max %.2f deg, scores %.2f .. %.2f"
          % (pos.max(), ang.max(), got["records"]["score"].min(), got["records"]["score"].max()))
    assert pos.max() <= 0.15 and ang.max() <= 1.0 and not got["rejected"].any()
