"""The lattice's edge inside the branch-and-bound matcher's blocks (nhip_bnb.hip process_candidate_c / process_candidate,
nhip_bnb_exact.h block_extent / sub_valid): the numpy statement, the lattices and placed scans at its seams, and the child
process that runs them in every form.  tests/test_lattice_edge_cpu.py checks the statement and the placements;
tests/test_lattice_edge_gpu.py starts the child and compares.

THE STATEMENT.  A plane of nx x ny translations is cut into 8 x 8 blocks (Y, X), each into four 4 x 4 sub-blocks (sy, sx).
Block column X holds vx = clamp(nx - 8 X, 0, 8) pose columns, block row Y holds vy = clamp(ny - 8 Y, 0, 8) pose rows; a
lattice side that is no multiple of 8 has one EDGE block column or row (v < 8).  Sub-block (sy, sx) holds a pose iff
4 sx < vx and 4 sy < vy, and then nc = min(4, vx - 4 sx) columns and nr = min(4, vy - 4 sy) rows of it are poses.  The matcher
counts and evaluates only sub-blocks that hold a pose, and a block goes whole (one pass over all 64 poses) when at least
WHOLE_MIN = 3 of them are alive -- so an edge block with at most 4 pose columns or rows (the bench's 81 = 8 * 10 + 1), which
has at most two, never does; one with 5 .. 7 of both has a pose in all four and is a block like any other.

THE GEOMETRY is that of tests/saturated_cases.py (240 cells of 0.05 m, sigma 2; the pooled table stays in LDS) with
max_shift 40, which admits the bench's 81 x 81 translations.  THE TARGETS have one point per hit cell: `plateau` (every
lookup at the top level: bound == sum, everything stays alive, the counts are deterministic), half planes `xhi` (x >= X0:
top level from column T on, a ramp of 2 R cells before it), `yhi`, their mirror images `xlo`, `ylo` (top level up to
column TL), and `corner` (the block x >= X0, y >= X0: (TC, TC) is its first top-level cell; at 8 bits the quantiser rounds
a half plane's ramp to the top level earlier than a corner's, so T < TC there).  THE SOURCES are n COINCIDENT
points in one cell; pose (ix, iy) of the centre rotation reads cell (c.x + ix - hx, c.y + iy - hy), so the cell chooses
which pose sees column T:
  x_last, y_last, corner     the optimum at ix = nx - 1, at iy = ny - 1, in the corner (the other axis ties: index 0)
  x_beyond<d>, y_beyond<d>,  the top level d = 1, 4, 8 cells BEYOND the upper edge: the sums keep rising past the last
  corner_beyond4             pose, so the sub-blocks without a pose carry the block's largest bounds and sums
  x_tie                      columns nx - 2 and nx - 1 both at the top level: the smaller linear index must win
  x_first, y_first           the optimum at index 0 of the mirror images (no edge blocks there: the unchanged path)
  flat                       the centre cell on `plateau`: every pose ties at n * levels, pose (0, 0, 0) wins
Rotations other than the centre one move a cluster into a neighbouring cell; volume() follows them.

    python -m tests.lattice_edge CELL_BITS OUT.npz     (in a process started with NHIP_TUNABLES=1)"""
import json
import math
import os
import sys

import numpy as np

from tests import saturated_cases as S
from tests.point_prefetch import EVERY_ADD, FORMS, INSTR

B, B4, WHOLE_MIN = 8, 4, 3          # BNB_B, BNB_B4 (nhip_common.h); WHOLE_MIN (nhip_bnb.hip)
RANGE, RES, SIGMA, FLOOR_P, MAX_SHIFT = S.RANGE, S.RES, S.SIGMA, S.FLOOR_P, 40
SIDE, R, CENTRE = S.SIDE, S.R, S.CENTRE
PAD = ((2 * MAX_SHIFT + 16) + 3) & ~3
X0, X1 = CENTRE + 6, CENTRE - 7     # the half planes x >= X0 and x <= X1
THETA_STEP = math.radians(1.0)
# (nx, ny): every residue that matters mod 8 and mod 4, and the bench's lattice.  A search has odd sides (nhip_csm_match
# refuses an even one, and the drop-in call searches 2 h + 1 translations), so the lattices with an even side -- a multiple
# of 8 among them -- cannot reach the kernel: they stay in the list, the child records that the library refuses them, the
# numpy statement covers them (tests/test_lattice_edge_cpu.py), and ODD_NEIGHBOURS, the odd sides on either side of each
# even one, run in their place: block extents 1, 3, 5 and 7 in either direction, edge blocks with a pose in one, two and all
# four sub-blocks.
LATTICES = ((1, 1), (4, 4), (5, 4), (8, 8), (9, 9), (12, 9), (13, 16), (17, 1), (81, 81))
ODD_NEIGHBOURS = ((3, 3), (5, 5), (5, 3), (7, 7), (11, 9), (13, 9), (13, 15), (13, 17))
N_THETAS = (1, 3)
LENGTHS = (1, 63, 64, 65, 193)
TARGETS = ("plateau", "xhi", "yhi", "corner", "xlo", "ylo")
BEYOND = (1, 4, 8)


def groups():
    """(nx, ny, n_theta) of every list the GPU test runs: the bench's lattice at one rotation only."""
    return [(nx, ny, nt) for nx, ny in LATTICES + ODD_NEIGHBOURS for nt in N_THETAS if (nx, ny) != (81, 81) or nt == 1]


def admitted(nx, ny):
    return nx % 2 == 1 and ny % 2 == 1


# ---- the statement ------------------------------------------------------------------------------------------------------
def extent(n, b):
    """Pose columns (rows) of block column (row) b of a lattice of n columns (rows)."""
    return min(max(n - B * b, 0), B)


def n_blocks(n):
    return (n + B - 1) // B


def sub_valid(vy, vx, sy, sx):
    return B4 * sx < vx and B4 * sy < vy


def sub_extent(vy, vx, sy, sx):
    """(nr, nc) of a valid sub-block."""
    return min(B4, vy - B4 * sy), min(B4, vx - B4 * sx)


def blocks(nx, ny):
    """[(Y, X, vy, vx)] of the lattice's blocks."""
    return [(Y, X, extent(ny, Y), extent(nx, X)) for Y in range(n_blocks(ny)) for X in range(n_blocks(nx))]


def valid_sub_blocks(nx, ny):
    """[(Y, X, sy, sx, nr, nc)] of the sub-blocks that hold a pose."""
    return [(Y, X, sy, sx) + sub_extent(vy, vx, sy, sx) for Y, X, vy, vx in blocks(nx, ny) for sy in (0, 1) for sx in (0, 1)
            if sub_valid(vy, vx, sy, sx)]


def covered(nx, ny):
    """The poses (ix, iy) the valid sub-blocks hold, as a list (a pose held twice appears twice)."""
    return [(B * X + B4 * sx + dx, B * Y + B4 * sy + dy) for Y, X, sy, sx, nr, nc in valid_sub_blocks(nx, ny)
            for dy in range(nr) for dx in range(nc)]


def counts(nx, ny):
    """Per rotation: blocks, edge blocks, sub-blocks in all, without a pose, valid ones of edge blocks."""
    bl = blocks(nx, ny)
    edge = [(vy, vx) for _, _, vy, vx in bl if vy < B or vx < B]
    valid_edge = sum(sub_valid(vy, vx, sy, sx) for vy, vx in edge for sy in (0, 1) for sx in (0, 1))
    return {"blocks": len(bl), "edge_blocks": len(edge), "sub_blocks": 4 * len(bl),
            "without_pose": 4 * len(bl) - len(valid_sub_blocks(nx, ny)), "valid_edge": valid_edge}


def saturated_counts(nx, ny, n_theta):
    """What the instrumented build counts where every bound equals every sum (everything stays alive, each block is taken
    once): a block with all four sub-blocks goes whole, an edge block's valid sub-blocks are evaluated one by one."""
    c = counts(nx, ny)
    n_valid = [(vy < B or vx < B, sum(sub_valid(vy, vx, sy, sx) for sy in (0, 1) for sx in (0, 1))) for _, _, vy, vx in blocks(nx, ny)]
    whole = sum(v >= WHOLE_MIN for _, v in n_valid)
    # (an edge block with 5 .. 7 pose columns and more than 4 rows, or the reverse, has a pose in all four sub-blocks and
    #  goes whole like any other; with 1 .. 4 -- the bench's 81 = 80 + 1 -- it has at most two and cannot)
    return {"blocks_whole": n_theta * whole, "sub_blocks": n_theta * sum(v for _, v in n_valid if v < WHOLE_MIN),
            "candidates_refined": n_theta * c["blocks"], "edge_blocks_refined": n_theta * c["edge_blocks"],
            "sub_blocks_without_pose": 0, "edge_blocks_whole": n_theta * sum(e and v >= WHOLE_MIN for e, v in n_valid),
            "blocks_total": n_theta * c["blocks"]}


# ---- targets and sources ------------------------------------------------------------------------------------------------
def reach_half(bits):
    """The most columns a blur window may lack (all its rows hit) and still round to the top level: 0 at 16 bits."""
    return max(m for m in range(R) if S.level_of(m, 0, bits) == S.levels(bits))


def top_column(bits):
    """T: the first top-level column of `xhi` (row of `yhi`)."""
    return X0 + R - reach_half(bits)


def top_diagonal(bits):
    """TC: (TC, TC) is the first top-level cell of `corner`, and the only one of the rectangle up to it."""
    return X0 + R - S.reach(bits)


def top_column_lo(bits):
    """TL: the last top-level column of `xlo` (row of `ylo`)."""
    return X1 - R + reach_half(bits)


def target_cells(name):
    a = np.arange(SIDE)
    if name == "plateau":
        return S.target_cells("plateau", 16)
    if name == "xhi":
        return S._cells(np.arange(X0, SIDE), a)
    if name == "yhi":
        return S._cells(a, np.arange(X0, SIDE))
    if name == "xlo":
        return S._cells(np.arange(0, X1 + 1), a)
    if name == "ylo":
        return S._cells(a, np.arange(0, X1 + 1))
    if name == "corner":
        return S.G._block(X0, SIDE, SIDE)
    raise KeyError(name)


def target(name):
    return S.G.cell_centres(target_cells(name), SIDE, RES)


def half(n):
    return (n - 1) // 2


def placements(nx, ny, bits):
    """{name: (target, source cell (column, row), claimed (ix, iy) of the centre rotation's first maximum | None)}."""
    T, TC, TL, hx, hy = top_column(bits), top_diagonal(bits), top_column_lo(bits), half(nx), half(ny)
    at_x = lambda d, T=T: T - d - (nx - 1) + hx   # the source column that puts pose column nx - 1 + d on column T
    at_y = lambda d, T=T: T - d - (ny - 1) + hy
    out = {"x_last": ("xhi", (at_x(0), CENTRE), (nx - 1, 0)), "y_last": ("yhi", (CENTRE, at_y(0)), (0, ny - 1)),
           "corner": ("corner", (at_x(0, TC), at_y(0, TC)), (nx - 1, ny - 1)),
           "x_tie": ("xhi", (at_x(-1), CENTRE), (max(nx - 2, 0), 0)),
           "x_first": ("xlo", (TL + hx, CENTRE), (0, 0)), "y_first": ("ylo", (CENTRE, TL + hy), (0, 0)),
           "flat": ("plateau", (CENTRE, CENTRE), (0, 0)),
           "corner_beyond4": ("corner", (at_x(4, TC), at_y(4, TC)), (nx - 1, ny - 1))}
    for d in BEYOND:
        out["x_beyond%d" % d] = ("xhi", (at_x(d), CENTRE), (nx - 1, 0))
        out["y_beyond%d" % d] = ("yhi", (CENTRE, at_y(d)), (0, ny - 1))
    return out


def sources(nx, ny, bits):
    """[(name, target, cell, n points)] of a lattice's list: every placement at every length."""
    return [("%s/%d" % (name, n), t, cell, n) for name, (t, cell, _) in sorted(placements(nx, ny, bits).items()) for n in LENGTHS]


def lookup_origin(point, k, n_theta, hx, hy):
    """(row, column) of the image cell that pose (0, 0) of rotation k reads for `point`: the kernels' float32 rotation and
    the definition's floor (tests/saturated_cases.py origins, without the border)."""
    cf, sf = S.rotation(0.0, k, n_theta, THETA_STEP)
    x, y = np.float32(point[0]), np.float32(point[1])
    xr = np.float32(cf * x) - np.float32(sf * y)
    yr = np.float32(sf * x) + np.float32(cf * y)
    col = SIDE // 2 + int(math.floor(float(xr) / RES)) - hx
    row = SIDE // 2 + int(math.floor(float(yr) / RES)) - hy
    return row, col


def volume(image, cell, n, nx, ny, n_theta):
    """volume[k, ix, iy]: the sums of n coincident points in `cell` on the (SIDE x SIDE, [row][column]) image."""
    out = np.zeros((n_theta, nx, ny), np.int64)
    for k in range(n_theta):
        row, col = lookup_origin(S.cluster_point(cell), k, n_theta, half(nx), half(ny))
        assert row >= 0 and col >= 0 and row + ny <= SIDE and col + nx <= SIDE
        out[k] = np.asarray(image)[row:row + ny, col:col + nx].T.astype(np.int64) * n
    return out


def spec_of(csm, bits):
    return csm.grid_spec(RANGE, RES, SIGMA, FLOOR_P, MAX_SHIFT, bits, skip_map=bits == 16)


# ---- the child process --------------------------------------------------------------------------------------------------
COUNTED = ("blocks_whole", "sub_blocks", "candidates_refined", "blocks_total", "edge_blocks_refined", "sub_blocks_without_pose",
           "edge_blocks_whole")


def run(bits, out_path):
    from nautilus_amd import csm
    assert os.environ.get("NHIP_TUNABLES") == "1", "the forms are chosen through switches a process reads only then"
    targets = [target(t) for t in TARGETS]
    arrays, meta = {}, {}
    for nx, ny, n_theta in groups():
        g = "%dx%dx%d" % (n_theta, nx, ny)
        srcs = sources(nx, ny, bits)
        st = csm.ScanTable.from_list(targets + [S.cluster(cell, n) for _, _, cell, n in srcs])
        grids = csm.LikelihoodGrids(st, np.arange(len(TARGETS), dtype=np.int32), spec_of(csm, bits))
        n = len(srcs)
        src = np.arange(len(TARGETS), len(TARGETS) + n, dtype=np.int32)
        slot, th0 = np.array([TARGETS.index(t) for _, t, _, _ in srcs], np.int32), np.zeros(n)
        meta[g] = {"n_pairs": n, "side": int(grids.layout.side), "pool_bytes": int(grids.layout.pool_bytes)}
        if not admitted(nx, ny):  # (refused: what the library says goes to the parent)
            for flags in ({}, {"exhaustive": True}):
                try:
                    csm.match_pairs(st, grids, src, slot, th0, csm.search_spec(n_theta, nx, ny, THETA_STEP, **flags))
                    meta[g]["refused"] = None
                except Exception as e:  # (NhipError)
                    meta[g].setdefault("refused", str(e))
            grids.close()
            st.close()
            continue

        def once(name, search, env, src=src, slot=slot, th0=th0):
            os.environ.update(env)
            try:
                csm.bnb_stats_levels()  # (reset)
                rec, sums = csm.match_pairs(st, grids, src, slot, th0, search)
                launch = csm.last_launch()
                stats = {k: int(v) for k, v in csm.bnb_stats_levels().items() if k in COUNTED} if "NHIP_BNB_STATS" in env else None
            finally:
                for k in env:
                    os.environ.pop(k, None)
            return np.frombuffer(rec.tobytes(), np.uint8), sums, launch, stats

        bnb = csm.search_spec(n_theta, nx, ny, THETA_STEP)
        flat = [i for i, (name, _, _, _) in enumerate(srcs) if name.startswith("flat/")]
        for name, (env, _) in FORMS.items():
            for v, e in ((name, env), (name + "_instr", dict(env, **INSTR))):
                arrays["rec_%s_%s" % (g, v)], arrays["sum_%s_%s" % (g, v)], launch, _ = once(v, bnb, e)
                meta[g][v] = launch
            # the saturated pairs alone, one at a time, counted
            meta[g][name + "_counts"] = [once(name, bnb, dict(env, **INSTR), src[i:i + 1], slot[i:i + 1], th0[i:i + 1])[3] for i in flat]
        ex = csm.search_spec(n_theta, nx, ny, THETA_STEP, exhaustive=True)
        for name, env in EVERY_ADD.items():
            arrays["rec_%s_%s" % (g, name)], arrays["sum_%s_%s" % (g, name)], _, _ = once(name, ex, env)
        grids.close()
        st.close()
    np.savez(out_path, meta=np.array(json.dumps(meta)), **arrays)


if __name__ == "__main__":
    run(int(sys.argv[1]), sys.argv[2])
