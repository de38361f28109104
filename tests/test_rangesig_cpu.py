"""Range signatures without a GPU: the numpy statement (hostside.range_signatures / scan_signatures / signature_candidates) held
to the slow statement of the spec (tests/rangesig_reference.py) on every crafted case, what the crafted cases are for, the
library's tables and refusals (pure host), and the quality of the proposals on a ray-traced map of the synthetic world."""
import ctypes as C
import math

import numpy as np
import pytest

from nautilus_amd import _lib, csm, hostside, rangesig
from tests import rangesig_reference as R
from tests import relocalize_cases as cases

MAP_CASES, MATCH_CASES = R.map_cases(), R.match_cases()


def product_spec(spec):
    s = rangesig.default_spec()
    for f in R.FIELDS:
        setattr(s, f, getattr(spec, f))
    return s


# ---------------------------------------------------------------- the three statements
@pytest.mark.parametrize("case", MAP_CASES, ids=[c[0] for c in MAP_CASES])
def test_hostside_map_signatures_equal_reference(case):
    name, grid, spec, rays = case
    want_a, want_sig, want_stats = R.map_results()[name]
    a, sig, stats = hostside.range_signatures(grid, product_spec(spec), rays)
    assert np.array_equal(a, want_a) and a.shape == want_a.shape and a.dtype == np.int32
    assert sig.tobytes() == want_sig.tobytes() and stats.tolist() == want_stats.tolist()
    assert stats[3:6].sum() == 64 * spec.rays_per_sector * len(a)
    if rays is None:  # the library's table is the reference's
        assert [tuple(r) for r in rangesig.tables(product_spec(spec))[0].tolist()] == R.ray_table(spec)


def test_hostside_scan_signatures_equal_reference():
    xy, off, spec = R.scan_case()
    want = R.scan_result()
    assert hostside.scan_signatures(xy, off, product_spec(spec)).tobytes() == want.tobytes()
    assert [float(v) for v in rangesig.tables(product_spec(spec))[1]] == [float(v) for v in R.edge_table(spec)]
    assert want[7, 31] == 0 and want[7, 32] == 8  # the origin in sector 31; (-1, +-0) in sector 32, 1 m = 8 units
    assert (want[0] == 255).all() and (want[1] != 255).sum() == 1 and (want[6] != 255).all()
    # r2 on both sides of edge2[1] and of edge2[254], the edge itself among them
    e2 = R.edge_table(spec)
    p = xy[off[8]:off[9]]
    r2 = (p[:, 0] * p[:, 0]).astype(np.float32) + (p[:, 1] * p[:, 1]).astype(np.float32)
    for k in (1, 254):
        T = e2[k]
        assert (r2 == T).any() and (r2 == np.nextafter(T, np.float32(0))).any() and (r2 == np.nextafter(T, np.float32(np.inf))).any(), k


@pytest.mark.parametrize("case", MATCH_CASES, ids=[c[0] for c in MATCH_CASES])
def test_hostside_candidates_equal_reference(case):
    name, qs, ms, an, spec = case
    want, (none, written) = R.match_results()[name]
    rec, stats = hostside.signature_candidates(qs, ms, an, product_spec(spec))
    assert np.array_equal(rec, want) and rec.dtype == np.int32 and stats[6:].tolist() == [none, written]


def test_map_cases_hold_what_they_are_for():
    """edges and corners of the window, a wall at k = 1 and at k = n, 254 reached, unknown before a wall, no node, no anchor"""
    res = R.map_results()
    a, sig, stats = res["rooms 37x29 stride 1 m 1 L 7"]
    assert (a[:, 0] == 0).any() and (a[:, 0] == 36).any() and (a[:, 1] == 0).any() and (a[:, 1] == 28).any()
    assert stats[4] > 0 and stats[3] > 0 and stats[5] > 0
    a, sig, _ = res["wall at k = 1 .. n"]
    row = {int(r[0]): s for r, s in zip(a, sig) if r[1] == 1}
    # sector 0 looks along +x: the wall at x = 9 is k = 9 - x cells of 0.05 m away, in units of 0.125 m; k = 8 is beyond n = 7
    assert [int(row[x][0]) for x in range(1, 9)] == [255] + [(k * 26214) >> 16 for k in range(7, 0, -1)]
    a, sig, _ = res["saturating unit"]
    assert int(sig[[i for i, r in enumerate(a) if tuple(r[:2]) == (2, 1)][0]][0]) == 254
    assert res["no free cell"][0].shape == (0, 4) and res["no free cell"][2][0] == 99
    assert res["rooms 37x29 stride 64 m 4 L 600"][2][0] == 0
    # an unknown cell before a wall: 255 by default, its range under NHIP_RANGESIG_UNKNOWN_STOPS
    plain, stops = res["rooms 37x29 stride 3 m 4 L 600"], res["rooms 37x29 unknown stops stride 3 m 4 L 600"]
    assert np.array_equal(plain[0], stops[0]) and (stops[1] <= plain[1]).all() and (stops[1] < plain[1]).sum() > 100
    # rdiv's halves: the rays to (4, 2) and to (-4, -2) are not mirror images
    assert R.ray_table(R.make_spec(max_ray_cells=4, rays_per_sector=1))[0][:3] == (4, 0, 4)
    assert [((2 * k * 2 + 4) // 8, (2 * k * -2 + 4) // 8) for k in (1, 2, 3, 4)] == [(1, 0), (1, -1), (2, -1), (2, -2)]


def test_match_cases_hold_what_they_are_for():
    res = R.match_results()
    rec = res["ties among shifts and anchors"][0]
    assert rec[0, 0].tolist() == [0, 0, 2 * 64, 64] and rec[0, 1, 0] == 1  # shift 0 of 64 equal ones; anchor 0 before anchor 1
    rec = res["valid around min_sectors"][0]
    assert (rec[0] == -1).all() and (rec[1] == -1).all() and rec[2, 0, 3] == 8
    assert res["bytes 0 254 255"][0][0, :, 2].tolist() == [0, 64 * 254, 16320]
    rec = res["suppression min_sep 2"][0][0, :, 0]
    assert rec[:5].tolist() == [0, 3, 6, 9, 30]  # 3 steps apart in i; anchor 10 = (0, 1) is 1 step from anchor 0, anchor 30 = (0, 3) is 3
    assert res["suppression min_sep 0"][0][0, :, 0].tolist() == list(range(16))
    rec = res["fewer anchors than K"][0][0]
    assert rec[:4, 0].tolist() == [0, 2, 3, 5] and (rec[4:] == -1).all()
    rec = res["turned by 5 and by 63 sectors"][0]
    assert rec[0, 0, :3].tolist() == [7, 5, 0] and rec[1, 0, :3].tolist() == [3, 63, 0]
    # the sign of item 5: shift 5 is a heading of +5 sectors, shift 63 one of -1
    th = rangesig.priors(rec[:, :1], R.lattice_anchors(12), product_spec(R.make_spec(res=0.5, cell_x0=-3, cell_y0=4)))[:, 0]
    assert np.allclose(th[:, 2], [5 * 2 * math.pi / 64, -2 * math.pi / 64]) and th[0, :2].tolist() == [(-3 + 7 + 0.5) * 0.5, (4 + 0 + 0.5) * 0.5]
    assert np.isnan(rangesig.priors(np.full((1, 2, 4), -1), R.lattice_anchors(12), product_spec(R.make_spec()))).all()


# ---------------------------------------------------------------- the library without a device
def test_tables_at_the_longest_ray():
    """n >= 1 and k scale < 2^31 for every ray of L = 4096, every m"""
    for m in (1, 2, 4, 8):
        rays, edge2 = rangesig.tables(rangesig.spec(max_ray_cells=4096, rays_per_sector=m, width=8, height=8))
        assert rays.shape == (64 * m, 4) and rays[:, 2].min() >= 1 and rays[:, 2].max() <= 4096
        assert (rays[:, 2] == np.abs(rays[:, :2]).max(axis=1)).all()
        assert (rays[:, 2].astype(np.int64) * rays[:, 3].astype(np.int64)).max() < 2 ** 31 and rays[:, 3].min() > 0
        assert np.all(np.diff(edge2) > 0) and edge2[0] == 0 and edge2[254] == np.float32(31.75) ** 2
    # the half offset of phi: no ray ends on an axis at (L, 0) exactly by symmetry, and the table has the rotational symmetry
    rays = rangesig.tables(rangesig.spec(max_ray_cells=600, width=8, height=8))[0]
    assert np.array_equal(rays[64:128, 0], -rays[:64, 1]) and np.array_equal(rays[64:128, 1], rays[:64, 0])


@pytest.mark.parametrize("field,bad", [("res", 0.0), ("res", math.inf), ("unit", 0.0), ("unit", math.nan), ("width", 0), ("width", 16385),
                                       ("height", 0), ("occ_min", 0), ("occ_min", 128), ("free_max", -1), ("free_max", 100), ("stride", 0),
                                       ("stride", 1025), ("max_ray_cells", 0), ("max_ray_cells", 4097), ("rays_per_sector", 3),
                                       ("rays_per_sector", 16), ("top_k", 0), ("top_k", 17), ("min_sep", -1), ("min_sep", 65),
                                       ("min_sectors", 0), ("min_sectors", 65), ("flags", 2), ("reserved", 1), ("unit", 1e-7)])
def test_spec_and_table_errors_without_a_device(field, bad):
    """NHIP_ERR_ARG with a message from every entry point, before a device is looked for (unit 1e-7: n scale >= 2^31)"""
    lib = _lib.load()
    s = rangesig.spec(width=8, height=8)
    setattr(s, field, bad)
    calls = [lambda: lib.nhip_rangesig_tables(C.byref(s), None, None),
             lambda: lib.nhip_rangesig_anchors_dev(None, C.byref(s), 0, None, None, None, 1 << 20, None),
             lambda: lib.nhip_rangesig_map_dev(None, C.byref(s), None, None, 0, None, None, None),
             lambda: lib.nhip_rangesig_scans_dev(None, None, 0, C.byref(s), None, None),
             lambda: lib.nhip_rangesig_match_dev(None, 0, None, None, 0, C.byref(s), None, None, None, 0, None),
             lambda: lib.nhip_rangesig_candidates(None, C.byref(s), None, None, 0, 0, None, None, None, None, None, None)]
    for call in calls:
        assert call() == _lib.NHIP_ERR_ARG and len(lib.nhip_last_error()) > 0
    if field != "unit" or bad != 1e-7:
        assert lib.nhip_rangesig_workspace_bytes(C.byref(s), 1, 1) == -1
        with pytest.raises(ValueError):
            hostside.rangesig_spec_check(s)


def test_defaults_counts_and_no_device():
    lib = _lib.load()
    s = rangesig.default_spec()
    assert (s.res, s.unit, s.occ_min, s.free_max, s.stride, s.max_ray_cells, s.rays_per_sector, s.top_k, s.min_sep, s.min_sectors, s.flags,
            s.reserved) == (0.05, 0.125, 100, 0, 10, 600, 4, 5, 2, 8, 0, 0)
    assert C.sizeof(_lib.RangesigSpec) == 72
    s = rangesig.spec(width=8, height=8)
    assert lib.nhip_rangesig_match_dev(None, -1, None, None, 0, C.byref(s), None, None, None, 0, None) == _lib.NHIP_ERR_ARG
    assert lib.nhip_rangesig_map_dev(None, C.byref(s), None, None, (1 << 20) + 1, None, None, None) == _lib.NHIP_ERR_ARG
    assert lib.nhip_rangesig_anchors_dev(None, C.byref(s), 0, None, None, None, 100, None) == _lib.NHIP_ERR_ARG  # (the workspace)
    assert lib.nhip_rangesig_workspace_bytes(C.byref(s), -1, 1) == -1 and lib.nhip_rangesig_workspace_bytes(C.byref(s), 1, -1) == -1
    # one row of keys per query, rows of 64 keys; never below the anchors' row counts; capped, one row excepted
    w = lambda a, q: lib.nhip_rangesig_workspace_bytes(C.byref(s), a, q)
    assert w(0, 0) == w(1, 1) == w(64, 64) == 65792 and w(65, 1000) == 128 * 4 * 1000 and w(4000, 10 ** 6) == (64 << 20) // 16128 * 16128
    assert w(1 << 20, 5) == 5 * 4 * (1 << 20) and w(1 << 20, 100) == (64 << 20)
    if _lib.device_count() == 0:  # no fall-back: the compute entry points refuse
        for rc in (lib.nhip_rangesig_anchors_dev(None, C.byref(s), 0, None, None, None, 1 << 20, None),
                   lib.nhip_rangesig_map_dev(None, C.byref(s), None, None, 0, None, None, None),
                   lib.nhip_rangesig_scans_dev(None, None, 0, C.byref(s), None, None),
                   lib.nhip_rangesig_match_dev(None, 0, None, None, 0, C.byref(s), None, None, None, 0, None),
                   lib.nhip_rangesig_candidates(None, C.byref(s), None, None, 0, 0, None, None, None, None, None, None)):
            assert rc == _lib.NHIP_ERR_NODEV


# ---------------------------------------------------------------- quality, on the numpy statement alone
MAP_SCANS = 400
TOP1_MEASURED, TOPK_MEASURED = 99, 100  # of 100 queries (test_recall_on_the_mapped_lap's docstring)




def test_recall_on_the_mapped_lap():
    """The setup: SynthBag(400), the 40 m x 25 m world's lap; the map from the 200 even scans at their truth poses through
    tests/occupancy_reference.occupancy with the defaults -- 1843 x 1544 cells, 3,451 occupied; the defaults of the spec with
    NHIP_RANGESIG_UNKNOWN_STOPS: 28,336 lattice nodes, 3,992 anchors; the queries are the 100 scans 1, 5, ..., 397, no priors.
    A query is recalled at rank k when proposal k lies within 1 m and 15 degrees of the truth (well inside the matcher's +-2 m /
    +-30 degrees).  Measured here, on the numpy statement alone (held equal to the slow reference on every crafted case): top-1
    99 of 100, top-5 100 of 100; the floors are those less two queries.  This guards the sign of the heading (item 5) and the
    spec, as test_recall_of_the_descriptor_on_a_perturbed_lap does for the place descriptor.
    Without the flag (not a condition; measured once on the 50 scans 1, 9, ..., 393): top-1 1 of 50, top-5 2 of 50 -- 772,681 of
    the 1,021,952 rays end in an unknown cell, because in a map ray-traced from scans the 2,900 cells in front of the walls
    that some scans hit and others saw through are neither free nor occupied; with those cells taken as walls 49 and 50 of 50.
    That is why the flag exists and why global_localize sets it."""
    bag, grid, occ = cases.mapped_lap()
    assert grid.shape == (1544, 1843) and int((grid == 100).sum()) == 3451
    spec = rangesig.spec(occ, flags=_lib.NHIP_RANGESIG_UNKNOWN_STOPS)
    anchors, sig, stats = hostside.range_signatures(grid, spec)
    assert stats[:3].tolist() == [28336, 3992, 0] and stats[3:6].sum() == 256 * 3992
    q = list(range(1, MAP_SCANS, 4))
    qxy, qoff = csm.pack_scans([bag.scans[i] for i in q])
    rec, s2 = hostside.signature_candidates(hostside.scan_signatures(qxy, qoff, spec), sig, anchors, spec)
    ok = cases.near_truth(rangesig.priors(rec, anchors, spec), bag.truth[q])
    top1, topk = int(ok[:, 0].sum()), int(ok.any(axis=1).sum())
    print("rays ended on a wall %d, in unknown %d, outside or at n %d; %d queries: top-1 %d, top-%d %d; valid sectors %d .. %d"
          % (stats[3], stats[4], stats[5], len(q), top1, spec.top_k, topk, rec[:, 0, 3].min(), rec[:, 0, 3].max()))
    assert s2[6] == 0 and s2[7] == len(q) * spec.top_k
    assert top1 >= TOP1_MEASURED - 2 and topk >= TOPK_MEASURED - 2

