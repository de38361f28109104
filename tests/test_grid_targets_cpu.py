"""The definitions of tests/grid_reference.py against the CPU oracle, and the preconditions of its target scans; no GPU.

For every (geometry, cell width, floor) of the matrix and every target scan: the numpy restatement -- hit raster, exact
integer blur, quantisation by nhip_grid_tables' threshold table -- equals oracle.grid_build (libm log in double) cell for
cell.  That pins the host tables (make_thresholds) at sigma 0.7 / 5.3 and the floors 1e-3 / 1e-30, and it is what lets
tests/test_grid_targets_gpu.py trust the definitions.  The preconditions make sure an input cannot quietly stop covering
its case: they are computed from the oracle, numpy and nhip_grid_tables only."""
import numpy as np
import pytest

from tests import grid_reference as G
from oracle import oracle as O


def _tables_and_images(geometry, bits, floor_p):
    spec, ospec, L = G.specs(geometry, bits, floor_p)
    names, clouds, facts = G.geometry_targets(geometry)
    taps, thr = G.grid_tables(spec)
    sums = [G.blur_sums(G.hit_raster(c, L.side, spec.res), taps) for c in clouds]
    images = [O.grid_build(c, ospec) for c in clouds]
    return spec, L, names, facts, taps, thr, sums, images


@pytest.mark.parametrize("combination", G.COMBINATIONS, ids=G.combination_id)
def test_definitions_equal_the_oracle_and_the_targets_cover_their_cases(combination):
    geometry, bits, floor_p = combination
    spec, L, names, facts, taps, thr, sums, images = _tables_and_images(*combination)
    S, R, levels = L.side, L.blur_radius, 255 if bits == 8 else 65535
    assert (S, R) == (facts["side"], facts["R"]) == G.geometry_of(*G.GEOMETRIES[geometry][:3])
    assert taps.sum() == L.tap_sum and np.all(np.diff(thr.astype(np.int64)) >= 0)
    for name, V, img in zip(names, sums, images):
        assert np.array_equal(G.quantise_by_table(V, thr), img), name
    at = dict(zip(names, range(len(names))))
    # filled: the top of the table, and a tile neighbourhood with every cell a hit
    for name in ("filled_corner", "filled_tile"):
        assert images[at[name]].max() == levels and sums[at[name]].max() == int(L.tap_sum) ** 2, name
    assert facts["filled_tile_inside"] and facts["filled_tile_cells"] == (64 + 2 * R) ** 2
    if geometry == "C":
        assert R == 16 and facts["filled_tile_cells"] == 9216
    # rim: the corner cells are written; -range is cell 0 and +range no cell where the raster ends on the range (at B,
    # 666 cells of 0.03 m, it ends inside: -range is outside too, and the scan carries points on the raster's own ends)
    rim = images[at["rim"]]
    if floor_p < 0.5:  # (under the floor of 0.999 a single hit stays at 0 everywhere: that case is about filled blocks)
        assert min(rim[0, 0], rim[0, S - 1], rim[S - 1, 0], rim[S - 1, S - 1]) > 0
    hits = G.hit_raster(G.geometry_targets(geometry)[1][at["rim"]], S, spec.res)
    assert hits[:, 0].any() and hits[:, S - 1].any() and hits[0].any() and hits[S - 1].any()
    if geometry == "B":
        assert facts["rim"]["minus_range_cell"] == (-1, -1) and facts["rim"]["plus_range_cell"][0] >= S
    else:
        assert facts["rim"] == {"minus_range_cell": (0, 0), "plus_range_cell": (S, S), "below_plus_range_cell": (S - 1, S - 1)}
    # edges: the points fall on both sides of their cell edge
    assert min(facts["edges_at_k"]) >= 0.25 and min(facts["edges_at_k_minus_1"]) >= 0.25
    ramp = images[at["ramp"]]
    figures = {"ramp distinct values": len(np.unique(ramp))}
    if bits == 16 and floor_p == 1e-10:
        assert figures["ramp distinct values"] >= 3000
    if (geometry, bits, floor_p) == ("D", 16, 1e-10):
        # blur sums from 1 upwards: the low end of the 16-bit table, where the quantiser's first guess is poor
        nz = np.concatenate([img[img > 0] for img in images])
        figures["smallest non-zero cell"] = int(nz.min())
        figures["ramp cells below 16384"] = int(((ramp > 0) & (ramp < 16384)).sum())
        assert sums[at["ramp"]][sums[at["ramp"]] > 0].min() == 1
        assert nz.min() < 16384 and figures["ramp cells below 16384"] >= 100
    if floor_p == 1e-3:
        # many non-zero blur sums quantise to 0 (the build's "nothing to store" path on sums that are not zero)
        figures["edges cells with a sum and value 0"] = int(((sums[at["edges"]] > 0) & (images[at["edges"]] == 0)).sum())
        assert figures["edges cells with a sum and value 0"] >= 1000
    if bits == 16:
        # cells whose blur sum lies right at a threshold of the table: the first sum of its level or the last
        t = thr.astype(np.int64)
        n_at = 0
        for V, img in zip(sums, images):
            q = img.astype(np.int64)
            nxt = np.where(q < 65535, t[np.minimum(q + 1, 65535)], np.int64(1) << 40)
            n_at += int(((V > 0) & ((V == t[q]) | (V == nxt - 1))).sum())
        figures["cells at a threshold"] = n_at
        if geometry == "D":
            assert n_at > 0
        # cells the quantiser's first guess misses by more than the 12 table steps it may walk, above the middle of the
        # table: settled by the binary search over all 16 bits
        off = [np.abs(G.first_guess(V[img > 0], thr) - img[img > 0].astype(np.int64)) for V, img in zip(sums, images)]
        mids = [(img[img > 0] >= 32768) & (img[img > 0] < 65535) for img in images]
        figures["largest miss of the first guess"] = int(max(o.max() for o in off if len(o)))
        figures["cells missed by > 12 levels, value in [32768, 65535)"] = int(sum(((o > 12) & m).sum() for o, m in zip(off, mids)))
        if floor_p == 0.999:
            assert figures["cells missed by > 12 levels, value in [32768, 65535)"] >= 100
            assert figures["largest miss of the first guess"] >= 48
    print("%s: %s" % (G.combination_id(combination), figures))


@pytest.mark.parametrize("bits", [8, 16])
def test_vectorised_pool_is_the_looped_definition(bits):
    """pool_definition (what expected_slot uses) against _pool_numpy, the definition as test_csm_gpu.py spells it, on a
    stored image whose side (666 + 2 * 36) is no multiple of either stride."""
    spec, ospec, L = G.specs("B", bits)
    names, clouds, _ = G.geometry_targets("B")
    for name in ("seams", "rim", "ramp"):
        e = G.expected_slot(clouds[names.index(name)], spec, ospec, L)
        stored = e["image"][:, :L.rows]
        for stride in (8, 4):
            assert np.array_equal(G.pool_definition(stored, bits, stride), G._pool_numpy(stored, bits, stride)), (name, stride)


def test_both_kinds_of_border_occur():
    """Borders that are a multiple of 16 cells (the build writes line masks for the next rebuild) and that are not."""
    pads = {g: G.specs(g, 8)[2].pad for g in G.GEOMETRIES}
    assert pads["A"] % 16 == 0 and pads["B"] % 16 != 0, pads
    assert any(p % 16 == 0 for p in pads.values()) and any(p % 16 != 0 for p in pads.values())


def test_a_weakened_input_is_noticed():
    """The preconditions are not vacuous: half of the filled corner block no longer reaches the table's top."""
    spec, ospec, L = G.specs("A", 16)
    names, clouds, _ = G.geometry_targets("A")
    block = clouds[names.index("filled_corner")]
    assert O.grid_build(block, ospec).max() == 65535
    assert O.grid_build(block[:len(block) // 2], ospec).max() < 65535
