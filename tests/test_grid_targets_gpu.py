"""The likelihood-table build (nhip_grid.h and its units) on targets chosen to break it, every plane of every slot against
its definition (tests/grid_reference.py; tests/test_grid_targets_cpu.py ties the definitions to the CPU oracle and holds the
inputs' preconditions).  Hits in the grid's corners and on its rim, on both sides of tile seams and where four tiles meet,
in the partial last tile; tile neighbourhoods with every cell a hit (blur radius 16: the build's LDS lists at capacity); a
density ramp (thousands of distinct 16-bit values, blur sums from 1 upwards at sigma 0.7); points on cell edges; piles;
floors of 1e-3 and 1e-30; then the other ways to the same bytes: builds in chunks, rebuilds over another build's tiles,
the band kernels, slots without the image -- and one pass through the matcher, which reads all of it.

Every comparison is exact equality of integers or bytes."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from nautilus_amd import _lib, csm
from oracle import oracle as O
from tests import grid_reference as G

pytestmark = pytest.mark.gpu

DEG = math.radians(1.0)


def _assert_every_slot(grids, names, expected, what):
    """assert_slot on every slot; the failure names every scan whose slot differs, not only the first."""
    failures = []
    for slot, name in enumerate(names):
        try:
            G.assert_slot(grids, slot, expected[slot], "%s, %s:" % (what, name))
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("combination", G.COMBINATIONS, ids=G.combination_id)
def test_every_plane_of_every_slot_is_its_definition(gpu, combination):
    geometry, bits, floor_p = combination
    spec, ospec, L = G.specs(geometry, bits, floor_p)
    names, clouds, _ = G.geometry_targets(geometry)
    expected = G.expected_slots(geometry, bits, floor_p)
    assert G.has_map(spec, L) and L.grid_bytes > 0, "the matrix checks every plane: image and skip map included"
    st = csm.ScanTable.from_list(clouds)
    grids = csm.LikelihoodGrids(st, np.arange(len(clouds), dtype=np.int32), spec)
    try:
        _assert_every_slot(grids, names, expected, G.combination_id(combination))
    finally:
        grids.close()
        st.close()


@pytest.mark.parametrize("geometry,bits", [("A", 8), ("A", 16), ("C", 8), ("C", 16)])
def test_slots_without_the_image(gpu, geometry, bits):
    """no_image=True: the pooled tables come from the tiled copies of the cells; every plane such a slot has."""
    spec, _, L = G.specs(geometry, bits, no_image=True)
    names, clouds, _ = G.geometry_targets(geometry)
    expected = G.expected_slots(geometry, bits)
    assert L.grid_bytes == 0 and not G.has_map(spec, L)
    st = csm.ScanTable.from_list(clouds)
    grids = csm.LikelihoodGrids(st, np.arange(len(clouds), dtype=np.int32), spec)
    try:
        _assert_every_slot(grids, names, expected, "%s %d bits, no image" % (geometry, bits))
    finally:
        grids.close()
        st.close()


# ------------------------------------------------------------------------------------------------ build paths
N_DEV = 6  # targets of the device-pointer builds: rim, seams, both filled scans, ramp, edges


@pytest.mark.parametrize("geometry,bits,skip_map", [("A", 8, True), ("A", 16, True), ("A", 16, False),
                                                    ("B", 8, True), ("B", 16, True), ("B", 16, False)])
def test_chunked_builds_rebuilds_and_band_kernels_give_the_same_bytes(gpu, small_bag, geometry, bits, skip_map):
    """nhip_grid_build_dev / nhip_grid_rebuild_dev on caller-owned buffers.  The one-pass build into zeroed memory is held
    to the definitions plane by plane; every other path must leave its bytes: builds in chunks of 1 and of 4 targets
    (workspaces smaller than the call: passes that start at a later target, a ragged last one) into a buffer of 0xFF,
    a rebuild over a chunked build (no tag: everything is cleared), a rebuild over the tables of other, sparser scans
    whose tiles lie elsewhere, a rebuild in reverse slot order, and NHIP_GRID_POOL=bands.  A has a border of 48 cells
    (line masks are written and read), B one of 36 (the dword path); 16-bit cells with and without a skip map (without:
    the pooled tables are cleared and rebuilt tile by tile)."""
    import torch
    dev = torch.device("cuda:0")
    lib = _lib.load()
    spec, _, L = G.specs(geometry, bits, skip_map=skip_map)
    assert (L.pad % 16 == 0) == (geometry == "A") and {G.specs(g, 8)[2].pad % 16 == 0 for g in G.GEOMETRIES} == {True, False}
    names, clouds, _ = G.geometry_targets(geometry)
    expected = G.expected_slots(geometry, bits)
    walls = [small_bag.scans[i] for i in (3, 8, 17, 25, 33, 40)]
    xy, off = csm.pack_scans(list(clouds) + walls)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_xy, d_off = t(xy), t(off)
    n = N_DEV
    nbytes = lib.nhip_grids_bytes(C.byref(spec), n)
    ws_full = lib.nhip_grid_workspace_bytes(C.byref(spec), n)
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    zeros = lambda k: torch.zeros(k, dtype=torch.uint8, device=dev)
    ones = lambda k: torch.full((k,), 255, dtype=torch.uint8, device=dev)

    def call(fn, ids, d_grids, d_ws):
        d_ids = t(np.asarray(ids, dtype=np.int32))
        _lib.check(fn(d_xy.data_ptr(), d_off.data_ptr(), d_off.numel() - 1, d_ids.data_ptr(), n, C.byref(spec), d_grids.data_ptr(),
                      d_ws.data_ptr(), d_ws.numel(), sp))
        torch.cuda.synchronize()
        return d_grids[:n * L.slot_bytes].cpu().numpy().reshape(n, L.slot_bytes).copy()

    ids = list(range(n))
    fresh = call(lib.nhip_grid_build_dev, ids, zeros(nbytes), zeros(ws_full))
    for slot in ids:
        G.assert_raw_slot(fresh[slot], spec, L, expected[slot], "%s %d bits, one-pass build, %s:" % (geometry, bits, names[slot]))
    # in chunks
    for chunk in (1, 4):
        Gc = ones(nbytes)
        ws = lib.nhip_grid_workspace_bytes(C.byref(spec), chunk)
        assert ws < ws_full
        assert np.array_equal(call(lib.nhip_grid_build_dev, ids, Gc, ones(ws)), fresh), "build in chunks of %d" % chunk
    assert np.array_equal(call(lib.nhip_grid_rebuild_dev, ids, Gc, ones(ws_full)), fresh), "rebuild over a chunked build, new workspace"
    Gc, Wc = ones(nbytes), ones(ws_full)
    assert np.array_equal(call(lib.nhip_grid_build_dev, ids, Gc, Wc[:lib.nhip_grid_workspace_bytes(C.byref(spec), 4)]), fresh)
    assert np.array_equal(call(lib.nhip_grid_rebuild_dev, ids, Gc, Wc), fresh), "rebuild over a chunked build, the same workspace"
    # over the tables of other scans, then in reverse slot order
    Gr, Wr = ones(nbytes), ones(ws_full)
    sparse = call(lib.nhip_grid_build_dev, [len(clouds) + i for i in range(n)], Gr, Wr)
    assert sparse.any() and not np.array_equal(sparse, fresh)
    assert np.array_equal(call(lib.nhip_grid_rebuild_dev, ids, Gr, Wr), fresh), "rebuild over sparser tables"
    assert np.array_equal(call(lib.nhip_grid_rebuild_dev, ids[::-1], Gr, Wr), fresh[::-1]), "rebuild in reverse slot order"
    assert np.array_equal(call(lib.nhip_grid_rebuild_dev, ids, Gr, Wr), fresh), "... and back"
    # the band kernels
    os.environ["NHIP_GRID_POOL"] = "bands"
    try:
        bands = call(lib.nhip_grid_build_dev, ids, ones(nbytes), ones(ws_full))
        Gb, Wb = ones(nbytes), ones(ws_full)
        call(lib.nhip_grid_build_dev, ids[::-1], Gb, Wb)
        bands_rebuilt = call(lib.nhip_grid_rebuild_dev, ids, Gb, Wb)
    finally:
        os.environ.pop("NHIP_GRID_POOL", None)
    assert np.array_equal(bands, fresh), "NHIP_GRID_POOL=bands"
    assert np.array_equal(bands_rebuilt, fresh), "NHIP_GRID_POOL=bands, rebuild"


# ------------------------------------------------------------------------------------------------ more than one z-slice
N_SLICED = 65537  # a launch's z dimension holds 65,535 targets: two slices, the second of two targets


def test_more_targets_than_one_z_slice_in_one_pass(gpu):
    """65,537 targets in one pass of nhip_grid_build_dev: the kernels launched in z-slices (skip map, level 1 from level
    2, and with NHIP_GRID_POOL=bands the band kernel) run a second slice, whose slots are t_base + blockIdx.z.  The
    smallest geometry with a tile and a blur: side 4 (one tile), border 16, blur radius 2, 8-bit cells with the skip
    map -- under 16 KB a slot, so the buffer stays under 1 GB.  Target ids cycle through five scans of a few points (one
    empty): every slot i must equal slot i mod 5 (compared on the device), and slots 0 .. 4, 65,535 and 65,536 are held
    to the definitions plane by plane."""
    import torch
    dev = torch.device("cuda:0")
    lib = _lib.load()
    range_m, res, sigma = 0.1, 0.05, 0.5
    spec = csm.grid_spec(range_m, res, sigma, 1e-10, 0, 8)
    ospec, L = O.grid_spec(range_m, res, sigma, 1e-10, 8), csm.grid_layout(spec)
    S = L.side
    assert S == 4 and L.blur_radius == 2 and L.pad == 16 and L.cell_bytes == 1 and G.has_map(spec, L)
    assert L.slot_bytes < 16384 and L.slot_bytes % 8 == 0, "a slot of the geometry the test is sized for"
    every_cell = [(c, r) for r in range(S) for c in range(S)]
    clouds = [G.cell_centres(cells, S, res) for cells in ([(0, 0)], [(3, 3), (0, 3), (2, 1)], every_cell)]
    clouds += [np.zeros((0, 2), np.float32), G.cell_centres([(3, 0), (1, 2)], S, res)]
    k = len(clouds)
    expected = [G.expected_slot(c, spec, ospec, L) for c in clouds]
    n = N_SLICED
    xy, off = csm.pack_scans(clouds)
    ids = (np.arange(n) % k).astype(np.int32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_xy, d_off, d_ids = t(xy), t(off), t(ids)
    nbytes = lib.nhip_grids_bytes(C.byref(spec), n)
    ws = lib.nhip_grid_workspace_bytes(C.byref(spec), n)
    assert nbytes < (1 << 30) and ws < (2 << 20)
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    d_grids = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    d_ws = torch.empty(ws, dtype=torch.uint8, device=dev)
    held = list(range(k)) + [n - 2, n - 1]

    def build_and_check(what):
        d_grids.fill_(255)
        d_ws.fill_(255)
        _lib.check(lib.nhip_grid_build_dev(d_xy.data_ptr(), d_off.data_ptr(), k, d_ids.data_ptr(), n, C.byref(spec),
                                           d_grids.data_ptr(), d_ws.data_ptr(), ws, sp))
        torch.cuda.synchronize()
        slots = d_grids[:n * L.slot_bytes].view(torch.int64).view(n, L.slot_bytes // 8)
        for j in range(k):
            same = (slots[j::k] == slots[j]).all(dim=1)
            assert bool(same.all()), "%s: slot %d differs from slot %d" % (what, j + k * int((~same).nonzero()[0]), j)
        for slot in held:
            raw = slots[slot].view(torch.uint8).cpu().numpy()
            G.assert_raw_slot(raw, spec, L, expected[slot % k], "%s, slot %d:" % (what, slot))

    build_and_check("one pass of %d targets" % n)
    os.environ["NHIP_GRID_POOL"] = "bands"
    try:
        build_and_check("one pass of %d targets, NHIP_GRID_POOL=bands" % n)
    finally:
        os.environ.pop("NHIP_GRID_POOL", None)


# ------------------------------------------------------------------------------------------------ the consumer
@pytest.mark.parametrize("bits", [16, 8])
def test_the_matcher_on_filled_ramp_and_seam_tables(gpu, small_bag, bits):
    """Wall scans and the ramp scan itself against the filled, ramp and seam tables of geometry A: best-pose indices and
    integer sums of the default form, the single kernel, the split form and the kernels that perform every add equal the
    oracle's."""
    spec, ospec, _ = G.specs("A", bits)
    names, clouds, _ = G.geometry_targets("A")
    # (the targets lie around cells 40 .. 230 of 480, the wall scans around the middle: the walls once as they are -- most
    #  of their points then read zeros -- and once moved onto the targets)
    onto = np.array([[-7.3, -7.3], [-6.9, -7.6]], dtype=np.float32)
    scans = list(clouds) + [small_bag.scans[8], small_bag.scans[9], small_bag.scans[8] + onto[0], small_bag.scans[9] + onto[1]]
    xy, off = csm.pack_scans(scans)
    slots = [names.index(s) for s in ("filled_corner", "filled_tile", "ramp", "seams")]
    sources = [len(clouds), len(clouds) + 1, len(clouds) + 2, len(clouds) + 3, names.index("ramp")]
    src = np.repeat(sources, len(slots)).astype(np.int32)
    slot = np.tile(np.arange(len(slots)), len(sources)).astype(np.int32)
    th0 = np.linspace(-0.03, 0.03, len(src))
    st = csm.ScanTable(xy, off)
    grids = csm.LikelihoodGrids(st, np.asarray(slots, dtype=np.int32), spec)
    try:
        ogr = O.grid_build_batch(xy, off, slots, ospec)
        want = O.csm_match_batch(xy, off, ogr, ospec, src, slot, th0, O.search_spec(5, 25, 25, DEG))
        assert (want["sum"] > 0).sum() >= len(src) // 2, "most pairs overlap"
        forms = [({}, False), ({"NHIP_BNB_KERNELS": "1"}, False), ({"NHIP_BNB_SPLIT": "1"}, False), ({}, True)]
        for env, exhaustive in forms:
            os.environ.update(env)
            try:
                got, sums = csm.match_pairs(st, grids, src, slot, th0, csm.search_spec(5, 25, 25, DEG, exhaustive=exhaustive))
            finally:
                for k in env:
                    os.environ.pop(k, None)
            for f in ("itheta", "ix", "iy"):
                assert np.array_equal(got[f], want[f]), (env, exhaustive, f, got[f], want[f])
            assert np.array_equal(sums, want["sum"]), (env, exhaustive)
    finally:
        grids.close()
        st.close()
