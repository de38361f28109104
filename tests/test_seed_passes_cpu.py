"""The statement and the inputs of tests/test_seed_passes_gpu.py hold what they claim (tests/seed_passes.py), by numpy and the
oracle alone: the constants are the sources', a seed pass with and without bounds evaluates the same poses wherever no bound
is 0, a superset with the same argmax where only one sub-block is alive, an edge block never goes whole either way, and the
two added placements sit where they claim."""
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import lattice_edge as L
from tests import saturated_cases as S
from tests import seed_passes as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nautilus_amd", "csrc")


def _src(name, at=CSRC):
    with open(os.path.join(at, name)) as f:
        return f.read()


def _images(bits):
    return {t: O.grid_build(L.target(t), O.grid_spec(L.RANGE, L.RES, L.SIGMA, L.FLOOR_P, bits)) for t in M.TARGETS}


@pytest.fixture(scope="module", params=[8, 16], ids=["8bit", "16bit"])
def images(request):
    return request.param, _images(request.param)


def test_constants_are_the_sources():
    bnb, host, params = _src("nhip_bnb.hip"), _src("nhip_bnb_host.hip"), _src("nhip_bnb_params.h")
    assert "constexpr int WHOLE_MIN = %d;" % L.WHOLE_MIN in bnb
    # bnb_plan alone reads the switch, the launch reports it in bit 4
    assert 'p.seed_bounds = is(tunable("NHIP_BNB_SEED_BOUNDS"), \'1\');' in host and host.count("NHIP_BNB_SEED_BOUNDS") == 1
    assert "((int32_t)p.seed_bounds << 4)" in host and "P.seed_bounds = plan.seed_bounds;" in host
    assert "NHIP_BNB_SEED_BOUNDS" not in bnb.replace("(NHIP_BNB_SEED_BOUNDS=1)", "")  # (named in one comment, read nowhere)
    assert list(M.BOUNDS) == ["NHIP_BNB_SEED_BOUNDS"] and "int32_t seed_bounds;" in params
    # a seed pass is the one with `done`; it reads the best sum once, and only a sum of 0 with the switch off leaves the bounds out
    assert "const bool seed_best0 = done != nullptr && best_sum<GLOBAL>(best) == 0u;" in bnb
    assert "const bool unbounded = seed_best0 && P.seed_bounds == 0;" in bnb and "if (P.levels >= 2 && !unbounded) {" in bnb
    # the candidates' kernels pass no `done`, the kernel that takes a pair's bounds does
    assert bnb.count("lane, best, nullptr, org, n_work, clk, runs, note, span);") == 1
    assert bnb.count("&P.keys[pair], nullptr, org, n, clk, runs, note, span);") == 1
    assert "lane, s_best, done, org, n_work, clk);" in bnb
    assert "constexpr int BNB_MAX_NB = %d;" % M.NB in _src("nhip_common.h")
    assert '"seed_bounds": bool(out[6] & 16)' in _src("csm.py", os.path.join(ROOT, "nautilus_amd"))
    assert set(M.SEED_FORMS) <= set(M.FORMS) and M.FORMS["hand_over"][0].get("NHIP_BNB_KERNELS") == "2"
    assert len(M.variants()) == 12 and all(("NHIP_BNB_SEED_BOUNDS" in e) == v.endswith("_bounds") for v, e in M.variants().items())


def test_seed_block_is_the_highest_bound_ties_to_the_largest_index():
    assert M.seed_block(np.zeros((2, 2))) is None
    assert M.seed_block([[1, 5], [5, 2]]) == (1, 0) and M.seed_block([[7, 5], [5, 2]]) == (0, 0)
    assert M.seed_block(np.full((11, 11), 3)) == (10, 10)


@pytest.mark.parametrize("lattice", M.STATED + M.LATTICES, ids=lambda v: "%dx%d" % v)
def test_both_paths_evaluate_the_same_poses_where_no_bound_is_zero(lattice):
    """... whatever the bounds are, as long as none is 0 and the best sum is: every block of the lattice as the seed."""
    nx, ny = lattice
    rng = np.random.default_rng(19)
    for Y, X, vy, vx in L.blocks(nx, ny):
        sub = rng.integers(1, 1000, (2, 2))
        with_b, whole_b = M.seed_poses(nx, ny, Y, X, sub, 0, switch=True)
        without, whole = M.seed_poses(nx, ny, Y, X, sub, 0, switch=False)
        assert with_b == without and whole_b == whole
        n_valid = sum(L.sub_valid(vy, vx, sy, sx) for sy in (0, 1) for sx in (0, 1))
        assert whole == (n_valid >= L.WHOLE_MIN) and len(without) == min(vx, L.B) * min(vy, L.B)
        assert all(ix < nx and iy < ny for ix, iy in without)
        if min(vx, vy) <= L.B4:
            assert not whole  # an edge block with at most 4 pose columns or rows: at most two sub-blocks hold a pose
        # a best sum above 0 (a gate's floor) keeps the bounds whatever the switch says
        assert M.seed_poses(nx, ny, Y, X, sub, 500, switch=False) == M.seed_poses(nx, ny, Y, X, sub, 500, switch=True)


@pytest.mark.parametrize("lattice", M.STATED + M.LATTICES, ids=lambda v: "%dx%d" % v)
def test_zero_bounds_make_the_path_without_bounds_a_superset(lattice):
    nx, ny = lattice
    rng = np.random.default_rng(23)
    for Y, X, vy, vx in L.blocks(nx, ny):
        for _ in range(8):
            sub = rng.integers(1, 1000, (2, 2)) * (rng.random((2, 2)) < 0.5)
            with_b, _ = M.seed_poses(nx, ny, Y, X, sub, 0, switch=True)
            without, _ = M.seed_poses(nx, ny, Y, X, sub, 0, switch=False)
            assert with_b <= without
            # what is added lies in sub-blocks whose bound is 0: poses that sum to 0
            for ix, iy in without - with_b:
                assert sub[(iy - L.B * Y) // L.B4][(ix - L.B * X) // L.B4] == 0


def test_one_live_sub_block_gives_the_same_argmax(images):
    """`one_sub` on every lattice: in the seed block of the centre rotation exactly one sub-block holds a pose that does not
    sum to 0; the pass without bounds evaluates the whole block's poses (or the edge block's sub-blocks), a superset of the
    pass with the tightest bounds, and the best key over either set is the same -- and, the seed block holding the
    lattice's optimum, the first maximum of the oracle's volume."""
    bits, img = images
    seen_whole = 0
    for nx, ny in M.LATTICES:
        t, cell, _ = M.placements(nx, ny, bits)["one_sub"]
        for n in M.LENGTHS:
            vol = L.volume(img[t], cell, n, nx, ny, 1)
            blocks, sub = M.tight_bounds(vol[0], nx, ny)
            Y, X = M.seed_block(blocks)
            assert (Y, X) == (L.n_blocks(ny) - 1, L.n_blocks(nx) - 1), (nx, ny, n)
            assert np.count_nonzero(sub[Y, X]) == 1, (nx, ny, n, sub[Y, X])
            c0, r0 = M.one_sub_pose(nx, ny)
            assert vol[0, c0, r0] > 0 and vol[0, :c0, :].max() == 0 and vol[0, :, :r0].max() == 0, (nx, ny, n)
            with_b, whole_b = M.seed_poses(nx, ny, Y, X, sub[Y, X], 0, switch=True)
            without, whole = M.seed_poses(nx, ny, Y, X, sub[Y, X], 0, switch=False)
            assert with_b <= without and not whole_b
            n_valid = len(M.alive_sub_blocks(nx, ny, Y, X, sub[Y, X], 0, take_bounds=False))
            assert (with_b < without) == (n_valid > 1) and whole == (n_valid >= L.WHOLE_MIN)
            seen_whole += whole
            key = lambda p: (int(vol[0, p[0], p[1]]), -(p[0] * ny + p[1]))
            best_b, best = max(with_b, key=key), max(without, key=key)
            assert best_b == best and all(vol[0, ix, iy] == 0 for ix, iy in without - with_b)
            pose, top = S.first_maximum(vol)
            assert pose == (0,) + best and top == vol[0, best[0], best[1]] > 0
    assert seen_whole  # (7 x 7 and 13 x 13: the pass without bounds takes the block whole)


def test_nothing_scores_nothing_and_every_other_placement_scores(images):
    bits, img = images
    for nx, ny, n_theta in M.groups():
        for name, (t, cell, claim) in M.placements(nx, ny, bits).items():
            vol = L.volume(img[t], cell, 3, nx, ny, n_theta)
            if name == "nothing":
                assert vol.max() == 0 and S.first_maximum(vol) == ((0, 0, 0), 0)
            else:
                assert vol.max() > 0, (nx, ny, n_theta, name)


def test_lattices_cover_the_seams():
    ext = {(L.extent(nx, L.n_blocks(nx) - 1), L.extent(ny, L.n_blocks(ny) - 1)) for nx, ny in M.LATTICES}
    assert {(7, 7), (1, 1), (3, 3), (5, 5), (1, 5), (5, 1)} <= ext
    # sub-blocks of 1 x 4 and 4 x 1 poses on the last block column and row
    assert (4, 1) in {(nr, nc) for _, X, _, _, nr, nc in L.valid_sub_blocks(9, 13) if X == 1}
    assert (1, 4) in {(nr, nc) for Y, _, _, _, nr, nc in L.valid_sub_blocks(13, 9) if Y == 1}
    assert all(nx % 2 == 1 and ny % 2 == 1 for nx, ny in M.LATTICES) and (8, 8) in M.STATED and (12, 12) in M.STATED
    assert M.N_THETAS == (1, 3, 9) and M.LENGTHS == (1, 63, 64, 65, 193)
    assert len(M.groups()) == 3 * (len(M.LATTICES) - 1) + 1
