"""The statement and the inputs of tests/test_zero_chunks_gpu.py hold what they claim (tests/zero_chunks.py), by numpy and the
oracle alone: on the oracle's table, for every input, rotation and sub-block, the chunks the rule visits contain every chunk
that holds a cell that is not 0 -- for single sub-blocks, for the two of a pair and for a block's four; the placed entries
sit in the chunks they name; the fall-backs are fall-backs; every input has one expected record, the first maximum of the
oracle's volume; and the switch is where the statement says."""
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import lattice_edge as L
from tests import saturated_cases as S
from tests import zero_chunks as M

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nautilus_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_constants_and_switch_are_the_sources():
    params, host, bnb = _src("nhip_bnb_params.h"), _src("nhip_bnb_host.hip"), _src("nhip_bnb.hip")
    assert "constexpr int RUN_CHUNKS = %d;" % (M.RUN_WAVE // M.CHUNK) in params
    assert 'tunable("NHIP_BNB_ZERO_CHUNKS")' in host and "((int32_t)p.zero_chunks << 3)" in host
    assert host.count("NHIP_BNB_ZERO_CHUNKS") == 1          # bnb_plan alone reads it
    assert "w > 257u" in _src("nhip_bnb_origin.h") and M.FIELD_POINTS == 257
    # the kernel that works a pair from start to end keeps no run list and takes every chunk
    assert "rotation_pass<CB, false, false>(" in bnb and bnb.count("rotation_pass<CB, true, true, true>(") == 2
    assert "P.zero_chunks != 0 && P.levels >= 2 ? nrc : 0" in bnb   # (no strip bounds, no notes: every chunk)
    assert list(M.OFF) == ["NHIP_BNB_ZERO_CHUNKS"] and M.PAD == L.PAD
    names = set(M.variants())
    assert len(names) == 18 and {"split_levels1", "hand_over_levels1"} <= names and all(("NHIP_BNB_ZERO_CHUNKS" in e) == v.endswith("_off") for v, e in M.variants().items())


@pytest.fixture(scope="module", params=[8, 16], ids=["8bit", "16bit"])
def tables(request):
    bits = request.param
    gs = O.grid_spec(M.RANGE, M.RES, M.SIGMA, M.FLOOR_P, bits)
    assert O.grid_side(gs) == M.SIDE
    out = {}
    for t in M.TARGETS:
        img = O.grid_build(M.target(t), gs)
        big = M.padded(img)
        out[t] = (img, big, M.level2(big), M.window_max(big, 4, 1))
    return bits, gs, out


def test_the_table_is_what_the_inputs_assume(tables):
    bits, _, T = tables
    img = np.asarray(T["square"][0]).astype(np.int64)
    nz = np.argwhere(img > 0)
    assert nz.min() >= M.SQ0 - M.R - 1 and nz.max() <= M.SQ1 + M.R, (nz.min(), nz.max())
    assert img[M.PEAK, M.PEAK] == img.max() > 0
    assert np.asarray(T["nothing"][0])[:300, :300].max() == 0


@pytest.mark.parametrize("lattice", M.LATTICES, ids=lambda v: "%dx%dx%d" % v)
def test_visited_chunks_hold_every_cell_that_is_not_zero(tables, lattice):
    bits, _, T = tables
    nx, ny, n_theta = lattice
    nbx, nby = L.n_blocks(nx), L.n_blocks(ny)
    left_out = 0
    for name, t, cells in M.sources(nx, ny, bits):
        _, big, P4, M4 = T[t]
        pts = M.scan(cells)
        for k in range(n_theta):
            row, col = M.stored_origins(pts, k, n_theta, nx, ny)
            assert row.min() >= 0 and col.min() >= 0 and row.max() + ny + 8 < big.shape[0] and col.max() + nx + 8 < big.shape[1]
            nch = int(M.cell_list(row, col)[-1]) // M.CHUNK + 1
            assert nch <= 17
            for Y in range(nby):
                for X in range(nbx):
                    block = [(Y, X, sy, sx) for sy in (0, 1) for sx in (0, 1)]
                    passes = [[s] for s in block] + [[block[0], block[1]], [block[2], block[3]], block]
                    for subs in passes:
                        v, need = M.visited(row, col, P4, subs), M.needed(row, col, M4, subs)
                        assert need <= v <= set(range(nch)), (name, k, subs, need, v)
                        left_out += nch - len(v)
    assert left_out > 0


def test_placed_entries_sit_where_they_claim(tables):
    bits, _, T = tables
    for nx, ny, n_theta in M.LATTICES:
        H = M.live(nx, ny)
        srcs = {name: (t, cells) for name, t, cells in M.sources(nx, ny, bits)}
        _, big, P4, _ = T["square"]
        all_subs = [(Y, X, sy, sx) for Y in range(L.n_blocks(ny)) for X in range(L.n_blocks(nx)) for sy in (0, 1) for sx in (0, 1)]

        def lists(name):
            row, col = M.stored_origins(M.scan(srcs[name][1]), (n_theta - 1) // 2, n_theta, nx, ny)
            return row, col, M.cell_list(row, col), M.run_list(row, col)

        # (a) the live entry on either side of a chunk boundary; every other chunk is left out by every pass
        for n in (128, 1088):
            for where, entry in (("last", n - 1), ("first", 0), ("e63", 63), ("e64", 64)):
                row, col, ce, ru = lists("live_%s/%d" % (where, n))
                at = srcs["live_%s/%d" % (where, n)][1].index(H)
                assert ce[at] == entry and ce[-1] == n - 1 and M.has_run_list(row, col)
                assert M.visited(row, col, P4, all_subs) == {entry // M.CHUNK}
        # (b) one run, from the last entry of chunk 0 into chunk 1
        for r in (2, 5, 64):
            row, col, ce, ru = lists("across/%d" % r)
            assert len(row) == 64 + r and ce[-1] == 64 and ce[-2] == 63 and ru[-1] == ru[64] and (ru == ru[-1]).sum() == r
            assert M.visited(row, col, P4, all_subs) == {0, 1}
        # (c) no chunk without an entry of H
        for n in (128, 512):
            row, col, ce, ru = lists("alternate/%d" % n)
            assert ce[-1] == n - 1 and M.has_run_list(row, col)
            hrow, hcol = M.stored_origins(M.point(H)[None], (n_theta - 1) // 2, n_theta, nx, ny)
            for c in range(n // M.CHUNK):
                assert ((row == hrow[0]) & (col == hcol[0]) & (ce // M.CHUNK == c)).any()
        # (d) nothing to visit
        _, _, P4n, _ = T["nothing"]
        row, col, ce, ru = lists("nothing/1088")
        assert M.visited(row, col, P4n, all_subs) == set()
        # (f) the fall-backs
        row, col, ce, ru = lists("runs_full")
        assert ru[-1] + 1 == 1088 > M.RUN_WAVE and M.group8_points(ce) <= M.FIELD_POINTS and not M.has_run_list(row, col)
        row, col, ce, ru = lists("field")
        assert M.group8_points(ce) > M.FIELD_POINTS and not M.has_run_list(row, col)
        assert M.visited(row, col, P4, all_subs[:1]) == set(range(int(ce[-1]) // M.CHUNK + 1))
    # (h) one field of block (1, 1) for E, at least three for H, in different chunks
    srcs = {name: cells for name, _, cells in M.sources(17, 17, bits)}
    cells = srcs["one_field"]
    E = M.one_field_cell(bits)
    row, col = M.stored_origins(M.scan(cells), 0, 1, 17, 17)
    ce = M.cell_list(row, col)
    bytes_of = lambda i: [int(P4[(row[i] >> 2) + 2 + sy, (col[i] >> 2) + 2 + sx] > 0) for sy in (0, 1) for sx in (0, 1)]
    assert cells[0] == M.live(17, 17) and cells[64] == E and ce[64] // M.CHUNK == 1 and ce[0] == 0
    assert sum(bytes_of(0)) >= L.WHOLE_MIN and sum(bytes_of(64)) == 1
    assert M.visited(row, col, P4, [(1, 1, sy, sx) for sy in (0, 1) for sx in (0, 1)]) == {0, 1}


@pytest.mark.parametrize("lattice", M.LATTICES, ids=lambda v: "%dx%dx%d" % v)
def test_every_input_has_one_expected_record(tables, lattice):
    bits, gs, T = tables
    nx, ny, n_theta = lattice
    ss = O.search_spec(n_theta, nx, ny, M.THETA_STEP)
    names = [name for name, _, _ in M.sources(nx, ny, bits)]
    assert len(names) == len(set(names)) and [n for n in names if n.startswith("len/")] == ["len/%d" % n for n in M.LENGTHS]
    for name, t, cells in M.sources(nx, ny, bits):
        vol = np.asarray(O.csm_scores(M.scan(cells), T[t][0], gs, 0.0, ss)).astype(np.int64)
        pose, best = S.first_maximum(vol)
        assert vol.shape == (n_theta, nx, ny) and 0 <= best
        if t == "nothing":
            assert (pose, best) == ((0, 0, 0), 0), name
        else:
            assert best > 0, name
        # the statement's sums: every pose's sum over the visited chunks alone is the volume's
        if nx <= 17:
            _, big, P4, _ = T[t]
            for k in range(n_theta):
                row, col = M.stored_origins(M.scan(cells), k, n_theta, nx, ny)
                ce = M.cell_list(row, col)
                for Y in range(L.n_blocks(ny)):
                    for X in range(L.n_blocks(nx)):
                        for sy in (0, 1):
                            for sx in (0, 1):
                                keep = np.isin(ce // M.CHUNK, list(M.visited(row, col, P4, [(Y, X, sy, sx)])))
                                for dy in range(4):
                                    for dx in range(4):
                                        ix, iy = 8 * X + 4 * sx + dx, 8 * Y + 4 * sy + dy
                                        if ix < nx and iy < ny:
                                            assert int(big[row[keep] + iy, col[keep] + ix].sum()) == vol[k, ix, iy], (name, k, ix, iy)
