"""Two live sub-blocks side by side in one pass of exact sums (nhip_bnb.hip strip_sub_blocks, nhip_bnb_exact.h pair_sums8): the
numpy statement of the pairing, the lattices and placed scans at its seams, and the child process that runs them in every
form with the switch on and off.  tests/test_pair_passes_cpu.py checks the statement and the placements;
tests/test_pair_passes_gpu.py starts the child and compares.

THE STATEMENT.  The candidates' kernels (csm_bnb_cand_kernel of the split form, csm_bnb_rot_kernel of the hand-over) take a
rotation's live blocks in block order, in STRIPS of up to three neighbours in X.  A block of the strip with at least WHOLE_MIN
live valid sub-blocks goes whole; the live valid sub-blocks (sy, sx) of the others are noted per sy as bit 2 t + sx of a mask
over the strip's six sub-block columns (t: the block's place in the strip).  Each mask is then walked from the left: a set
bit and its set right neighbour are ONE pass -- a pair -- when they are the two sub-blocks of one block (the left bit is
even); a pair `across` a block boundary (the left bit odd) is taken only by a library built with NHIP_BNB_PAIR_CROSS=1, which
is not the one that ships (ACROSS below); every other set bit is a pass of its own.  The kernel that works a pair from start
to end (csm_bnb_kernel: the seeds of every form, and all of the fused form) does not pair.  Every wave's seed is its highest bound, ties to the largest (rotation, block index):
where every bound is the same and each rotation has a wave of its own (n_theta <= 8) that is the rotation's LAST block, which
is taken alone before the candidates' kernels see the rest.

THE GEOMETRY, targets and placed scans are those of tests/lattice_edge.py, with three ties added, each of which the smaller
linear index (k * nx + ix) * ny + iy must win:
  tie_halves       `xhi` with the top level from pose column 2 on: columns 2, 3 (a pair's left half), 4 .. 7 (its right half)
                   and every later one tie
  tie_rows         `yhi` with the top level from pose row 1 on: rows 1 .. 3 of one half tie (and every column)
  tie_pair_single  `xhi` with the top level from pose column nx - 4 on: at nx = 8 m + 1 the columns 8 m - 3 .. 8 m - 1 of the
                   last full block (a pair) tie with the single column of the edge block (a pass of its own)

    python -m tests.pair_passes CELL_BITS OUT.npz     (in a process started with NHIP_TUNABLES=1)"""
import json
import os
import sys

import numpy as np

from tests import lattice_edge as L
from tests import saturated_cases as S
from tests.point_prefetch import EVERY_ADD, FORMS, INSTR

STRIP = 3                                   # blocks per strip (nhip_bnb.hip rotation_pass)
ACROSS = False                              # NHIP_BNB_PAIR_CROSS (nhip_bnb.hip): pairs across a block boundary
LATTICES = ((9, 9), (13, 9), (17, 3), (21, 3), (19, 5), (81, 81))
N_THETAS = (1, 3)
LENGTHS = (1, 63, 64, 65, 129, 193)
TARGETS = L.TARGETS
OFF = {"NHIP_BNB_PAIR_SUBS": "0"}
PAIRING_FORMS = ("hand_over", "split", "split_rounds")   # the forms whose candidates run in the kernels that pair
COUNTED = L.COUNTED + ("pair_passes", "pair_passes_across_blocks")


def groups():
    return [(nx, ny, nt) for nx, ny in LATTICES for nt in N_THETAS if (nx, ny) != (81, 81) or nt == 1]


# ---- the statement ------------------------------------------------------------------------------------------------------
def strips(xs):
    """The strips of a block row whose live blocks are `xs` (ascending): runs of neighbours, cut at STRIP blocks."""
    out = []
    for x in xs:
        if out and out[-1][-1] == x - 1 and len(out[-1]) < STRIP:
            out[-1].append(x)
        else:
            out.append([x])
    return out


def walk(mask, across_blocks=ACROSS):
    """(pairs, pairs across a block boundary, singles) of one mask over a strip's sub-block columns, walked from the left."""
    pairs = across = singles = 0
    c = 0
    while mask >> c:
        if (mask >> c) & 1:
            if (mask >> (c + 1)) & 1 and (across_blocks or c % 2 == 0):
                pairs += 1
                across += c & 1
                c += 1
            else:
                singles += 1
        c += 1
    return pairs, across, singles


def strip_passes(nx, ny, Y, xs, live=lambda Y, X, sy, sx: True, across_blocks=ACROSS):
    """{whole, pairs, across, singles} of one strip (blocks `xs` of block row Y) whose live sub-blocks `live` names."""
    out = {"whole": 0, "pairs": 0, "across": 0, "singles": 0}
    masks = [0, 0]
    for t, X in enumerate(xs):
        vy, vx = L.extent(ny, Y), L.extent(nx, X)
        alive = [(sy, sx) for sy in (0, 1) for sx in (0, 1) if L.sub_valid(vy, vx, sy, sx) and live(Y, X, sy, sx)]
        if len(alive) >= L.WHOLE_MIN:
            out["whole"] += 1
        else:
            for sy, sx in alive:
                masks[sy] |= 1 << (2 * t + sx)
    for m in masks:
        p, a, s = walk(m, across_blocks)
        out["pairs"] += p
        out["across"] += a
        out["singles"] += s
    return out


def saturated_pairs(nx, ny, n_theta, form, switch=True):
    """What the instrumented build counts where every bound equals every sum: {pair_passes, pair_passes_across_blocks}, and
    `passes`, the passes over sub-blocks in all (each pair saves one of lattice_edge.saturated_counts' sub_blocks)."""
    assert n_theta <= 8
    nbx, nby = L.n_blocks(nx), L.n_blocks(ny)
    pairs = across = 0
    if switch and form in PAIRING_FORMS:
        for Y in range(nby):
            xs = [X for X in range(nbx) if (Y, X) != (nby - 1, nbx - 1)]  # (the rotation's last block: its wave's seed)
            for s in strips(xs):
                got = strip_passes(nx, ny, Y, s)
                pairs += got["pairs"]
                across += got["across"]
    sub = L.saturated_counts(nx, ny, n_theta)["sub_blocks"]
    return {"pair_passes": n_theta * pairs, "pair_passes_across_blocks": n_theta * across, "passes": sub - n_theta * pairs}


# ---- the placed scans ---------------------------------------------------------------------------------------------------
def placements(nx, ny, bits):
    """tests/lattice_edge.py's, and the three ties."""
    T, hx, hy = L.top_column(bits), L.half(nx), L.half(ny)
    out = dict(L.placements(nx, ny, bits))
    first_top = lambda c, h: T - c + h   # the source column (row) that puts pose column (row) c on column (row) T
    cx, cy = min(2, nx - 1), min(1, ny - 1)
    out["tie_halves"] = ("xhi", (first_top(cx, hx), L.CENTRE), (cx, 0))
    out["tie_rows"] = ("yhi", (L.CENTRE, first_top(cy, hy)), (0, cy))
    out["tie_pair_single"] = ("xhi", (first_top(max(nx - 4, 0), hx), L.CENTRE), (max(nx - 4, 0), 0))
    return out


def sources(nx, ny, bits):
    return [("%s/%d" % (name, n), t, cell, n) for name, (t, cell, _) in sorted(placements(nx, ny, bits).items()) for n in LENGTHS]


# ---- the child process --------------------------------------------------------------------------------------------------
def variants():
    """name -> environment: every form, its instrumented build, each with the switch on and off."""
    out = {}
    for name, (env, _) in FORMS.items():
        for v, e in ((name, env), (name + "_instr", dict(env, **INSTR))):
            out[v] = e
            out[v + "_off"] = dict(e, **OFF)
    return out


def run(bits, out_path):
    from nautilus_amd import csm
    assert os.environ.get("NHIP_TUNABLES") == "1", "the forms are chosen through switches a process reads only then"
    targets = [L.target(t) for t in TARGETS]
    arrays, meta = {}, {}
    for nx, ny, n_theta in groups():
        g = "%dx%dx%d" % (n_theta, nx, ny)
        srcs = sources(nx, ny, bits)
        st = csm.ScanTable.from_list(targets + [S.cluster(cell, n) for _, _, cell, n in srcs])
        grids = csm.LikelihoodGrids(st, np.arange(len(TARGETS), dtype=np.int32), L.spec_of(csm, bits))
        n = len(srcs)
        src = np.arange(len(TARGETS), len(TARGETS) + n, dtype=np.int32)
        slot, th0 = np.array([TARGETS.index(t) for _, t, _, _ in srcs], np.int32), np.zeros(n)
        meta[g] = {"n_pairs": n, "side": int(grids.layout.side), "pool_bytes": int(grids.layout.pool_bytes)}

        def once(search, env, src=src, slot=slot, th0=th0):
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

        bnb = csm.search_spec(n_theta, nx, ny, L.THETA_STEP)
        flat = [i for i, (name, _, _, _) in enumerate(srcs) if name.startswith("flat/")]
        for v, env in variants().items():
            arrays["rec_%s_%s" % (g, v)], arrays["sum_%s_%s" % (g, v)], meta[g][v], _ = once(bnb, env)
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
