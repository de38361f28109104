"""The kernels' loops on their second trip (tests/loop_trips.py): K8's carries beyond 1024 scans, K16's and K21's grid-stride
over scans beyond 4096, K20's row steps beyond 1024 rows, its queries beyond 16384 and its windows of 255 .. 257 rows, K21's
lattice rows beyond 1024 and node steps at 64 and 128, the cost kernel's tiles in chunks that are no multiple of eight, and
the sector count of K16 and K21 on every sector boundary.  Device bytes against hostside (K8) and the references, for
equality; tests/test_loop_trips_cpu.py proves that the cases cross the seams they are named after."""
import ctypes as C

import numpy as np
import pytest

from nautilus_amd import _lib, localize, place, rangesig
from tests import localize_reference as LR
from tests import loop_trips as T
from tests import place_reference as PR
from tests import rangesig_reference as RR
from tests.test_hitl_gpu import _select_raw
from tests.test_localize_gpu import product_spec as mapwin_spec
from tests.test_localize_gpu import status as mapwin_status
from tests.test_rangesig_gpu import device_map, product_spec as rangesig_spec, status as rangesig_status

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def clean(torch):
    return _lib.load().nhip_dev_status(C.c_void_p(torch.cuda.current_stream().cuda_stream), None) == _lib.NHIP_OK


# ---------------------------------------------------------------- K8
@pytest.mark.parametrize("name,n", T.HITL_CASES)
def test_hitl_offsets_beyond_1024_scans(gpu, name, n):
    """hitl_offsets_kernel takes 1024 scans a step and carries four sums; its second pass adds n_a and pts_a to the b-nodes"""
    import torch
    table = T.hitl_table(name, n)
    want = T.hitl_expected(table)
    config = (T.HITL["line_a"], T.HITL["line_b"], T.HITL["width"], T.HITL["threshold"])
    got, _, _, n_scans, n_pts = _select_raw(config, table=table)
    assert n_scans == n and clean(torch)
    sizes, sentinels = (n_pts, 2 * n, n, n, 3), (77, -99, -99, -99, -99)
    for g, w, size, sentinel, what in zip(got, want, sizes, sentinels, ("class", "counts", "scan_block", "scan_offset", "totals")):
        assert np.array_equal(g[:size], w), (what, np.nonzero(g[:size] != w)[0][:8])
        assert len(g) == size + 64 and (g[size:] == sentinel).all(), what  # nothing written behind the output


# ---------------------------------------------------------------- K16 and K21: scans beyond 4096, the sector boundaries
@pytest.mark.parametrize("n", T.N_MANY_SCANS)
def test_describe_beyond_4096_scans(gpu, n):
    import torch
    xy, off = T.many_scans()
    want_D, want_bits = T.many_scans_descriptors()
    d_xy, d_off = torch.from_numpy(xy).to(DEV), torch.from_numpy(off).to(DEV)
    d_desc, d_bits = place.describe_on_device(d_xy, d_off, n, place.default_spec())
    assert clean(torch)
    assert np.array_equal(d_desc.cpu().numpy().view(np.uint64), want_D[:n]) and np.array_equal(d_bits.cpu().numpy(), want_bits[:n])


@pytest.mark.parametrize("n", T.N_MANY_SCANS)
def test_scan_signatures_beyond_4096_scans(gpu, n):
    import torch
    xy, off = T.many_scans()
    want = T.many_scans_signatures()
    d_xy, d_off = torch.from_numpy(xy).to(DEV), torch.from_numpy(off).to(DEV)
    got = rangesig.scan_signatures_on_device(d_xy, d_off, n, rangesig_spec(RR.make_spec())).cpu().numpy()
    assert rangesig_status(torch)[0] == _lib.NHIP_OK
    assert got.tobytes() == want[:n].tobytes(), np.argwhere(got != want[:n])[:5]


def test_sector_boundaries_through_both_kernels(gpu):
    """p = 2^e DIRS[j]: both products of the comparison are equal, the difference is exactly 0 and `>=` puts the point into
    sector j -- a contracted multiply-add or a `>` would not; the floats beside it fall as the reference's rounding says"""
    import torch
    xy, off = T.boundary_scans()
    n = len(off) - 1
    d_xy, d_off = torch.from_numpy(xy).to(DEV), torch.from_numpy(off).to(DEV)
    want = RR.scan_signatures(xy, off, RR.make_spec())
    got = rangesig.scan_signatures_on_device(d_xy, d_off, n, rangesig_spec(RR.make_spec())).cpu().numpy()
    assert rangesig_status(torch)[0] == _lib.NHIP_OK and got.tobytes() == want.tobytes(), np.argwhere(got != want)[:5]
    want_D, want_bits = PR.describe(xy, off, *PR.make_tables(8, 64.0))
    d_desc, d_bits = place.describe_on_device(d_xy, d_off, n, place.spec(n_rings=8, range_max=64.0))
    assert clean(torch)
    assert np.array_equal(d_desc.cpu().numpy().view(np.uint64), want_D) and np.array_equal(d_bits.cpu().numpy(), want_bits)
    for i, (x, y, j, kind) in enumerate(T.boundary_points()):  # the same sector through both
        if kind == 0:
            sector = j + (32 if (y < 0 or (y == 0 and x < 0)) else 0)
            assert got[i, sector] != 255 and want_D[i].sum() == np.uint64(1) << np.uint64(sector)


# ---------------------------------------------------------------- K20
@pytest.mark.parametrize("width,height", T.TALL_MAPS)
def test_map_cells_and_windows_beyond_1024_rows(gpu, width, height):
    """mapwin_row_scan_kernel takes 1024 rows a step: cells and windows (sides 8 and 41, rows on both sides of the steps), and
    max_cells one short, a total that only a later step than the first reaches: everything zero, the report raised"""
    import torch
    lib = _lib.load()
    grid, spec, origins = T.tall_map(width, height)
    mw = mapwin_spec(spec)
    want_cells = LR.map_cells(grid, spec)
    row_ptr, cols, stats = localize.map_cells(grid, mw, DEV)
    LR.same_cells((row_ptr, cols), want_cells, "cells")
    assert stats.tolist() == [want_cells[2], 0, 0, 0, 0, 0, 0, 0]
    for side in (8, 41):
        sp = T.with_side(spec, side)
        want = LR.map_windows(grid, sp, origins)
        LR.same(localize.windows(grid, mapwin_spec(sp), origins, DEV), want, "side %d" % side)
        LR.same(localize.windows_host_form(grid, mapwin_spec(sp), origins, int(want[1][-1])), want, "side %d (host form)" % side)
    if height > 1024:
        n_occ, n = want_cells[2], len(origins)
        d_grid, d_org = torch.from_numpy(grid).to(DEV), torch.from_numpy(origins).to(DEV)
        d_row_ptr, d_cols, d_stats = localize.map_cells_on_device(d_grid, mw, n_occ - 1)
        d_cols.fill_(-7)
        lib.nhip_mapwin_cells_dev(d_grid.data_ptr(), C.byref(mw), n_occ - 1, d_row_ptr.data_ptr(), d_cols.data_ptr(), d_stats.data_ptr(),
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
        d_xy, d_off, d_stats = localize.windows_on_device(d_row_ptr, d_cols, mw, d_org, n, 64 * n, d_stats)
        rc, info = mapwin_status(lib, torch)
        assert rc == _lib.NHIP_ERR_ARG and info[:4] == [localize.KIND_CELLS, localize.KIND_CELLS, n_occ, height]
        assert not d_row_ptr.cpu().numpy().any() and (d_cols.cpu().numpy() == -7).all() and not d_off.cpu().numpy().any()
        assert d_stats.cpu().numpy().tolist() == [n_occ, n, 0, n, 0, 1, 0, 0]
        assert mapwin_status(lib, torch)[0] == _lib.NHIP_OK  # (the record was consumed)


@pytest.mark.parametrize("n", T.N_MANY_QUERIES)
def test_windows_beyond_16384_queries(gpu, n):
    grid, spec, origins = T.many_queries()
    xy, off, stats = T.many_queries_windows()
    counts = np.diff(off[:n + 1])
    want = (xy[:off[n]], off[:n + 1], np.array([stats[0], n, off[n], (counts == 0).sum(), counts.max(), 0, 0, 0], np.int64))
    mw = mapwin_spec(spec)
    LR.same(localize.windows(grid, mw, origins[:n], DEV), want, "device form")
    LR.same(localize.windows_host_form(grid, mw, origins[:n], int(off[n])), want, "host form")


@pytest.mark.parametrize("side", (255, 256, 257))
def test_windows_of_256_rows_and_one_more(gpu, side):
    grid, spec, origins = T.wide_window_map()
    sp = T.with_side(spec, side)
    want = LR.map_windows(grid, sp, origins)
    LR.same(localize.windows(grid, mapwin_spec(sp), origins, DEV), want, "device form")
    LR.same(localize.windows_host_form(grid, mapwin_spec(sp), origins, int(want[1][-1])), want, "host form")


# ---------------------------------------------------------------- K21: the lattice
@pytest.mark.parametrize("name", [c[0] for c in T.lattice_cases()])
def test_anchors_beyond_1024_lattice_rows_and_64_nodes(gpu, name):
    """rs_row_scan_kernel takes 1024 lattice rows a step, rs_row_count_kernel and rs_row_pack_kernel 64 nodes: anchors, map
    signatures and stats; the capacity exact, and one short with the cut in a later step than the first"""
    import torch
    _, grid, spec = next(c for c in T.lattice_cases() if c[0] == name)
    ps = rangesig_spec(spec)
    want_a, want_sig, want_stats = T.lattice_results()[name]
    n_all = len(want_a)
    for cap in (None, n_all, n_all - 1):
        a, sig, stats, st = device_map(torch, grid, ps, max_anchors=cap)
        if cap == n_all - 1:
            assert st[0] == _lib.NHIP_ERR_ARG and st[1][1] == rangesig.KIND_ANCHORS and st[1][2] == n_all and st[1][3] == cap
            short_a, short_sig, short_stats = RR.anchors_and_signatures(grid, spec, None, max_anchors=cap)
            assert np.array_equal(a, short_a) and sig.tobytes() == short_sig.tobytes() and stats.tolist() == short_stats.tolist()
            assert stats[2] == 1 and np.array_equal(short_a, want_a[:cap])
        else:
            assert st[0] == _lib.NHIP_OK, st
            assert np.array_equal(a, want_a) and sig.tobytes() == want_sig.tobytes() and stats.tolist() == want_stats.tolist()


# ---------------------------------------------------------------- K21: the match
@pytest.mark.parametrize("Q", T.MATCH_QUERIES)
def test_match_in_chunks_that_are_no_multiple_of_eight(gpu, Q):
    """rs_cost_kernel takes eight queries a tile: Q in {7, 8, 9, 16, 25} in one chunk, and in chunks of 3, 8, 9 and 12 rows"""
    import torch
    qs, ms, an, spec, records = T.match_case()
    ps = rangesig_spec(spec)
    want = records[:Q]
    none, written = int((want[:, 0, 0] < 0).sum()), int((want[:, :, 0] >= 0).sum())
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    d_q, d_m, d_a = t(qs[:Q]), t(ms), t(an)
    for rows in (None,) + T.MATCH_CHUNK_ROWS:
        ws = None if rows is None else rows * T.key_row_bytes(T.MATCH_A)
        rec, stats = rangesig.match_on_device(d_q, Q, d_m, d_a, T.MATCH_A, ps, workspace=ws)
        assert rangesig_status(torch)[0] == _lib.NHIP_OK
        assert np.array_equal(rec.cpu().numpy(), want), (Q, rows)
        assert stats.cpu().numpy()[6:].tolist() == [none, written], (Q, rows)
