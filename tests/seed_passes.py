"""The seeds without their strip bounds (nhip_bnb.hip rotation_pass, the pass with `done` set): the numpy statement of which
sub-blocks a seed evaluates with and without bounds, the lattices and placed scans at its seams, and the child process that
runs them in every form with the switch on and off.  tests/test_seed_passes_cpu.py checks the statement and the placements;
tests/test_seed_passes_gpu.py starts the child and compares.

THE STATEMENT.  Every wave of csm_bnb_kernel evaluates its highest-bound block (ties: the largest (rotation, block index))
exactly before anything is pruned.  A sub-block (sy, sx) of that block is ALIVE iff it holds a pose of the lattice
(tests/lattice_edge.py sub_valid), its bound is not 0 and its bound reaches the pair's best sum; a block with at least
WHOLE_MIN = 3 alive sub-blocks is evaluated whole, otherwise its alive sub-blocks one by one.  A seed that begins while the
best sum is still 0 -- no score gate, no other wave's seed landed -- takes NO bounds: every sub-block that holds a pose is
alive.  That is the set the bounds give wherever no bound is 0, and a superset of it where one is; the added poses read only
empty cells, sum to 0, and a key of sum 0 never beats the floor key (pose 0 with sum 0).  NHIP_BNB_SEED_BOUNDS=1 takes the
bounds always; a best sum above 0 (a gate's floor) keeps them too.

THE GEOMETRY, targets and placed scans are those of tests/lattice_edge.py, with two added:
  one_sub    `corner` placed so that the first pose that reads a cell that is not 0 is the first pose of ONE sub-block of the
             lattice's last block (its sub-block (1, 1) where the block has more than 4 pose columns and rows, its only
             sub-block with a pose otherwise): the seed block's other sub-blocks hold poses that sum to 0
  nothing    `xhi` read 50 cells to the left of its first cell: every pose sums to 0, the record is pose 0 with sum 0 (no
             bound reaches above 0: no seed at all)
THE LATTICES.  A search has odd sides (the library refuses an even one), so tests/lattice_edge.py's 8 x 8 (no edge block) and
12 x 12 (an edge block of 4 pose columns) stay in the numpy statement (STATED) and their odd neighbours run: 7 x 7 (one block,
7 x 7 poses: all four sub-blocks), 9 x 9 (the last block 1 x 1), 11 x 11 (3 x 3), 13 x 13 (5 x 5: sub-blocks of 4 x 4, 4 x 1,
1 x 4, 1 x 1 poses), 9 x 13 and 13 x 9 (a last block column / row of sub-blocks with 1 x 4 and 4 x 1 poses: an even 1 x 4
lattice block needs a side of 8 m + 4), and the bench's 81 x 81 at one rotation.  Rotations 1, 3 and 9: nine give wave 0 two
rotations and so a choice of seed.

    python -m tests.seed_passes CELL_BITS OUT.npz     (in a process started with NHIP_TUNABLES=1)"""
import functools
import json
import os
import sys

import numpy as np

from tests import lattice_edge as L
from tests import saturated_cases as S
from tests.point_prefetch import EVERY_ADD, FORMS, INSTR

NB = 11                                     # blocks per row of a rotation's bounds (nhip_common.h)
STATED = ((8, 8), (9, 9), (12, 12), (9, 12), (12, 9))
LATTICES = ((7, 7), (9, 9), (11, 11), (13, 13), (9, 13), (13, 9), (81, 81))
N_THETAS = (1, 3, 9)
LENGTHS = (1, 63, 64, 65, 193)
TARGETS = L.TARGETS
SEED_FORMS = ("fused", "split", "hand_over")
BOUNDS = {"NHIP_BNB_SEED_BOUNDS": "1"}      # the switch: the seeds take their bounds whatever the best sum
MIN_SCORE = -22.0                           # a gate whose floor is above 0 for every length (the child asserts it)
COUNTED = L.COUNTED
SEED_COUNTED = ("seed_passes", "seed_passes_best0", "seed_passes_without_bounds", "seed_blocks_zero_sub")


def groups():
    return [(nx, ny, nt) for nx, ny in LATTICES for nt in N_THETAS if (nx, ny) != (81, 81) or nt == 1]


# ---- the statement ------------------------------------------------------------------------------------------------------
def seed_block(block_bounds):
    """(Y, X) of a rotation's seed: the highest bound of block_bounds[Y][X], ties to the largest block index NB * Y + X; None
    where no bound is above 0."""
    b = np.asarray(block_bounds)
    if b.max() <= 0:
        return None
    return max(((int(b[Y, X]), NB * Y + X, (Y, X)) for Y in range(b.shape[0]) for X in range(b.shape[1])))[2]


def alive_sub_blocks(nx, ny, Y, X, sub_bounds, best_sum, take_bounds):
    """[(sy, sx)] alive in block (Y, X): sub_bounds[sy][sx] are its sub-block bounds, take_bounds whether the pass takes them."""
    vy, vx = L.extent(ny, Y), L.extent(nx, X)
    valid = [(sy, sx) for sy in (0, 1) for sx in (0, 1) if L.sub_valid(vy, vx, sy, sx)]
    if not take_bounds:
        assert best_sum == 0  # (only such a pass leaves them out)
        return valid
    return [(sy, sx) for sy, sx in valid if sub_bounds[sy][sx] != 0 and sub_bounds[sy][sx] >= best_sum]


def seed_poses(nx, ny, Y, X, sub_bounds, best_sum=0, switch=False):
    """(poses (ix, iy) the seed pass of block (Y, X) evaluates, whole?).  switch: NHIP_BNB_SEED_BOUNDS=1."""
    vy, vx = L.extent(ny, Y), L.extent(nx, X)
    alive = alive_sub_blocks(nx, ny, Y, X, sub_bounds, best_sum, take_bounds=switch or best_sum != 0)
    whole = len(alive) >= L.WHOLE_MIN
    subs = [(sy, sx) for sy in (0, 1) for sx in (0, 1) if L.sub_valid(vy, vx, sy, sx)] if whole else alive
    poses = set()
    for sy, sx in subs:
        nr, nc = L.sub_extent(vy, vx, sy, sx)
        poses |= {(L.B * X + L.B4 * sx + dx, L.B * Y + L.B4 * sy + dy) for dy in range(nr) for dx in range(nc)}
    return poses, whole


def tight_bounds(plane, nx, ny):
    """(block bounds [Y][X], sub-block bounds [Y][X][sy][sx]) of one rotation's plane[ix][iy]: the maxima themselves -- the
    tightest bounds there are; the kernels' pooled ones are looser, never 0 where these are not."""
    nbx, nby = L.n_blocks(nx), L.n_blocks(ny)
    sub = np.zeros((nby, nbx, 2, 2), np.int64)
    for Y, X, sy, sx, nr, nc in L.valid_sub_blocks(nx, ny):
        x0, y0 = L.B * X + L.B4 * sx, L.B * Y + L.B4 * sy
        sub[Y, X, sy, sx] = plane[x0:x0 + nc, y0:y0 + nr].max()
    return sub.max(axis=(2, 3)), sub


# ---- the placed scans ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def corner_image(bits):
    from oracle import oracle as O
    return np.asarray(O.grid_build(L.target("corner"), O.grid_spec(L.RANGE, L.RES, L.SIGMA, L.FLOOR_P, bits)))


def first_cell(bits):
    """The first column (= row: the target is symmetric) of `corner`'s table that holds a cell that is not 0."""
    return int(np.nonzero(corner_image(bits).any(axis=0))[0][0])


def one_sub_pose(nx, ny):
    """The first pose (ix, iy) of the one sub-block of the last block that reads cells that are not 0."""
    lx, ly = L.n_blocks(nx) - 1, L.n_blocks(ny) - 1
    return (L.B * lx + (L.B4 if L.extent(nx, lx) > L.B4 else 0), L.B * ly + (L.B4 if L.extent(ny, ly) > L.B4 else 0))


def placements(nx, ny, bits):
    """tests/lattice_edge.py's, `one_sub` and `nothing`."""
    out = dict(L.placements(nx, ny, bits))
    Z, (c0, r0) = first_cell(bits), one_sub_pose(nx, ny)
    out["one_sub"] = ("corner", (Z - c0 + L.half(nx), Z - r0 + L.half(ny)), None)
    out["nothing"] = ("xhi", (L.CENTRE - 50, L.CENTRE), (0, 0))
    return out


def sources(nx, ny, bits):
    return [("%s/%d" % (name, n), t, cell, n) for name, (t, cell, _) in sorted(placements(nx, ny, bits).items()) for n in LENGTHS]


# ---- the child process --------------------------------------------------------------------------------------------------
def variants():
    """name -> environment: every form, its instrumented build, each with the seeds' bounds left out (the default) and with
    NHIP_BNB_SEED_BOUNDS=1 (`_bounds`)."""
    out = {}
    for name in SEED_FORMS:
        env = FORMS[name][0]
        for v, e in ((name, env), (name + "_instr", dict(env, **INSTR))):
            out[v] = e
            out[v + "_bounds"] = dict(e, **BOUNDS)
    return out


def run(bits, out_path):
    from nautilus_amd import csm
    assert os.environ.get("NHIP_TUNABLES") == "1", "the forms are chosen through switches a process reads only then"
    targets = [L.target(t) for t in TARGETS]
    arrays, meta = {}, {}
    spec = L.spec_of(csm, bits)
    meta["floors"] = {str(n): int(csm.gate_floor(spec, MIN_SCORE, n)) for n in LENGTHS}
    for nx, ny, n_theta in groups():
        g = "%dx%dx%d" % (n_theta, nx, ny)
        srcs = sources(nx, ny, bits)
        st = csm.ScanTable.from_list(targets + [S.cluster(cell, n) for _, _, cell, n in srcs])
        grids = csm.LikelihoodGrids(st, np.arange(len(TARGETS), dtype=np.int32), spec)
        n = len(srcs)
        src = np.arange(len(TARGETS), len(TARGETS) + n, dtype=np.int32)
        slot, th0 = np.array([TARGETS.index(t) for _, t, _, _ in srcs], np.int32), np.zeros(n)
        meta[g] = {"n_pairs": n, "side": int(grids.layout.side), "pool_bytes": int(grids.layout.pool_bytes)}

        def once(search, env, src=src, slot=slot, th0=th0, min_score=None):
            os.environ.update(env)
            try:
                csm.bnb_stats_levels()  # (reset)
                csm.bnb_stats_seeds()
                rec, sums = csm.match_pairs(st, grids, src, slot, th0, search, min_score=min_score)
                launch = csm.last_launch()
                stats = None
                if "NHIP_BNB_STATS" in env:
                    stats = {k: int(v) for k, v in csm.bnb_stats_levels().items() if k in COUNTED}
                    stats.update({k: int(v) for k, v in csm.bnb_stats_seeds().items() if k in SEED_COUNTED})
            finally:
                for k in env:
                    os.environ.pop(k, None)
            return np.frombuffer(rec.tobytes(), np.uint8), sums, launch, stats

        bnb = csm.search_spec(n_theta, nx, ny, L.THETA_STEP)
        flat = [i for i, (name, _, _, _) in enumerate(srcs) if name.startswith("flat/")]
        for v, env in variants().items():
            arrays["rec_%s_%s" % (g, v)], arrays["sum_%s_%s" % (g, v)], meta[g][v], meta[g][v + "_stats"] = once(bnb, env)
            # ... under a gate whose floor is above 0: the best starts there and every seed keeps its bounds
            arrays["rec_%s_%s_gated" % (g, v)], arrays["sum_%s_%s_gated" % (g, v)], _, meta[g][v + "_gated_stats"] = once(
                bnb, env, min_score=MIN_SCORE)
            if "_instr" in v:  # the saturated pairs alone, one at a time, counted
                meta[g][v + "_counts"] = [once(bnb, env, src[i:i + 1], slot[i:i + 1], th0[i:i + 1])[3] for i in flat]
        ex = csm.search_spec(n_theta, nx, ny, L.THETA_STEP, exhaustive=True)
        for name, env in EVERY_ADD.items():
            arrays["rec_%s_%s" % (g, name)], arrays["sum_%s_%s" % (g, name)], _, _ = once(ex, env)
        grids.close()
        st.close()
    np.savez(out_path, meta=np.array(json.dumps(meta)), **arrays)


if __name__ == "__main__":
    run(int(sys.argv[1]), sys.argv[2])
