"""Exact sums that leave out the chunks of the cell list whose windows hold only empty cells (nhip_bnb.hip chunk_mask,
nhip_bnb_exact.h *_masked, nhip_bnb_bounds.h strip_sums NOTE, nhip_bnb_origin.h cache_origins run_span): the numpy statement
of the rule, inputs placed where a mask can go wrong, and the child process that runs them in every form with the switch on
and off.  tests/test_zero_chunks_cpu.py checks the statement against the oracle's table and volumes;
tests/test_zero_chunks_gpu.py starts the child and compares.

THE STATEMENT.  A rotation's points become the CELL LIST: consecutive points with one window origin (stored row, column) are
one entry, cut at every 64th point; entries are taken in CHUNKS of 64.  Beside it the RUN LIST: consecutive points whose
origins share one 4 x 4 level-2 entry (row >> 2, column >> 2) are one run, cut at every 64th point too, so a run's cells lie
in the chunk of its first cell or that and the next.  The level-2 table holds, per 4 x 4 entry (i, j), the maximum P4[i][j]
of the 7 x 7 cells from (4 i, 4 j) on -- every cell a 4 x 4 sub-block of poses reads from any origin of the entry.  A pass
of exact sums over sub-blocks F = {(Y, X, sy, sx)} of rotation k visits chunk c iff some run with a cell in c has
P4[(row >> 2) + 2 Y + sy][(column >> 2) + 2 X + sx] > 0 for some member of F.  Every entry of a chunk that is left out
reads only cells that are 0 for every pose of F, so the pass's sums are those over all chunks.  A rotation without a usable
run list (more than RUN_WAVE runs; an aligned group of 8 lanes of either list with more than 257 points) visits every chunk,
and so does a search without sub-block bounds (NHIP_BNB_LEVELS=1), in which nothing loads the level-2 bytes.

THE GEOMETRY: range 8.0 m, res 0.05 (S = 320), sigma 2 (R = 6), max_shift 40 (pad 96).  THE TARGETS: `square`, the hit cells
[224, 237)^2 -- the table is 0 outside [218, 243)^2, rises to its largest value at (230, 230), the square's centre -- and
`nothing` (hits in [317, 320)^2 only: every cell any pose of any source reads is 0).  THE SOURCES are lists of points 0.3 cells
inside chosen cells:
  dead cells D_i   (20 + i % 100, 20 + i // 100): nothing they read on any lattice is ever hit; consecutive ones are
                   neighbours, so about four share a level-2 entry; `sparse` ones (20 + 4 (i % 40), 20 + 4 (i // 40)) never do
  the live cell H  (230 - (nx - 1) + hx, 230 - (ny - 1) + hy): the LAST pose reads the table's maximum, alone
  (a) live_<where>/<n>   n = 128, 1088 points, all dead but one: the last, the first, entry 63, entry 64
  (b) across/<r>   two coincident dead points, 62 dead cells, then a run of r points that starts in chunk 0 and ends in
                   chunk 1: r - 1 points in H's neighbour inside H's level-2 entry (one entry, number 63), then H (entry 64)
  (c) alternate/<n>  H, D_0, H, D_1, ... (n = 128, 512): every chunk holds an entry of H, no chunk can be left out
  (d) nothing/<n>  dead cells against `nothing`: every bound is 0, no pass is made, the record is pose (0, 0, 0) with sum 0
  (e) len/<n>      n - 1 dead cells, then H: 1, 63, 64, 65, 128, 129, 1081, 1088
  (f) runs_full    1088 points, sparse dead cells and H last: 1088 runs, more than the run list holds
      field        300 points in H, then 200 dead cells: five entries of H in one group of 8 lanes hold 300 > 257 points
  (h) one_field    H in chunk 0 and, 64 entries later, a cell E found by search: for block (1, 1) of the 17 x 17 lattice E's
                   run has exactly one level-2 byte that is not 0 while H's has at least three (the block can go whole, and
                   the whole pass must keep E's chunk)
  (g) the lattice's edge: the inputs of tests/lattice_edge.py on their own geometry, lattice 9 x 9 (group `edge`)

    python -m tests.zero_chunks CELL_BITS OUT.npz     (in a process started with NHIP_TUNABLES=1)"""
import json
import math
import os
import sys

import numpy as np

from tests import grid_reference as G
from tests import lattice_edge as L
from tests import saturated_cases as S
from tests.point_prefetch import EVERY_ADD, FORMS, INSTR

RANGE, RES, SIGMA, FLOOR_P, MAX_SHIFT = 8.0, 0.05, 2.0, 1e-10, 40
SIDE, R, CENTRE, PAD = 320, 6, 160, 96
SQ0, SQ1, PEAK = 224, 237, 230
THETA_STEP = math.radians(1.0)
CHUNK, RUN_WAVE, FIELD_POINTS = 64, 512, 257   # nhip_bnb_params.h RUN_WAVE; nhip_bnb_origin.h cache_origins
LATTICES = ((9, 9, 1), (17, 17, 3), (81, 81, 1))
LENGTHS = (1, 63, 64, 65, 128, 129, 1081, 1088)
TARGETS = ("square", "nothing")
OFF = {"NHIP_BNB_ZERO_CHUNKS": "0"}
MASKING_FORMS = ("hand_over", "split", "split_rounds")   # the forms whose candidates run in the kernels that keep a run list
COUNTED_CASES = ("live_", "alternate/", "nothing/", "runs_full", "field")


# ---- targets and sources ------------------------------------------------------------------------------------------------
def target(name):
    cells = G._block(SQ0, SQ1, SIDE) if name == "square" else G._block(SIDE - 3, SIDE, SIDE)
    return G.cell_centres(cells, SIDE, RES)


def point(cell):
    return np.array([(cell[0] - CENTRE + 0.3) * RES, (cell[1] - CENTRE + 0.3) * RES], np.float32)


def dead(i, sparse=False):
    return (20 + 4 * (i % 40), 20 + 4 * (i // 40)) if sparse else (20 + i % 100, 20 + i // 100)


def live(nx, ny):
    return (PEAK - (nx - 1) + (nx - 1) // 2, PEAK - (ny - 1) + (ny - 1) // 2)


def stored_origins(pts, k, n_theta, nx, ny):
    """Stored (row, column) of the window origin of every point under rotation k: the kernels' float32 rotation, the
    definition's floor, the border of PAD cells."""
    cf, sf = S.rotation(0.0, k, n_theta, THETA_STEP)
    x, y = pts[:, 0].astype(np.float32), pts[:, 1].astype(np.float32)
    xr = (cf * x).astype(np.float32) - (sf * y).astype(np.float32)
    yr = (sf * x).astype(np.float32) + (cf * y).astype(np.float32)
    col = SIDE // 2 + np.floor(xr.astype(np.float64) / RES).astype(np.int64) - (nx - 1) // 2 + PAD
    row = SIDE // 2 + np.floor(yr.astype(np.float64) / RES).astype(np.int64) - (ny - 1) // 2 + PAD
    return row, col


def _neighbour_in_entry(nx, ny):
    """H's neighbour in x that shares H's level-2 entry under the centre rotation of an odd n_theta."""
    H = live(nx, ny)
    _, col = stored_origins(point(H)[None], 0, 1, nx, ny)
    return (H[0] - 1, H[1]) if (int(col[0]) & 3) != 0 else (H[0] + 1, H[1])


def sources(nx, ny, bits):
    """[(name, target, cells of the scan's points in order)]"""
    H = live(nx, ny)
    out = []
    for n in (128, 1088):
        for where, at in (("last", n - 1), ("first", 0), ("e63", 63), ("e64", 64)):
            cells = [dead(i) for i in range(n)]
            cells[at] = H
            out.append(("live_%s/%d" % (where, n), "square", cells))
    A = _neighbour_in_entry(nx, ny)
    for r in (2, 5, 64):
        out.append(("across/%d" % r, "square", [dead(0), dead(0)] + [dead(i) for i in range(1, 63)] + [A] * (r - 1) + [H]))
    for n in (128, 512):  # (every point a run of its own: 512 are what the run list holds)
        out.append(("alternate/%d" % n, "square", [H if i % 2 == 0 else dead(i // 2) for i in range(n)]))
    for n in (128, 1088):
        out.append(("nothing/%d" % n, "nothing", [dead(i) for i in range(n)]))
    for n in LENGTHS:
        out.append(("len/%d" % n, "square", [dead(i) for i in range(n - 1)] + [H]))
    out.append(("runs_full", "square", [dead(i, True) for i in range(1087)] + [H]))
    out.append(("field", "square", [H] * 300 + [dead(i) for i in range(200)]))
    if (nx, ny) == (17, 17):
        E = one_field_cell(bits)
        out.append(("one_field", "square", [H] + [dead(i) for i in range(63)] + [E] + [dead(63 + i) for i in range(20)]))
    return out


def scan(cells):
    return np.stack([point(c) for c in cells]).astype(np.float32)


# ---- the statement ------------------------------------------------------------------------------------------------------
def cell_list(row, col):
    """Per point the index of its entry of the cell list."""
    n = len(row)
    head = np.ones(n, bool)
    head[1:] = (row[1:] != row[:-1]) | (col[1:] != col[:-1])
    head[np.arange(n) % CHUNK == 0] = True
    return np.cumsum(head) - 1


def run_list(row, col):
    """Per point the index of its run."""
    n = len(row)
    head = np.ones(n, bool)
    head[1:] = ((row[1:] >> 2) != (row[:-1] >> 2)) | ((col[1:] >> 2) != (col[:-1] >> 2))
    head[np.arange(n) % CHUNK == 0] = True
    return np.cumsum(head) - 1


def group8_points(index):
    """The most points any aligned group of 8 lanes of a list holds (entry e sits in lane e % 64)."""
    w = np.bincount(index % CHUNK, minlength=CHUNK)
    return int(w.reshape(8, 8).sum(axis=1).max())


def list_chunks(row, col):
    """Chunks of the cell list as the kernels keep it: a list whose group of 8 lanes would hold more than 257 points is built
    again with one point per entry."""
    ce = cell_list(row, col)
    return (len(row) + CHUNK - 1) // CHUNK if group8_points(ce) > FIELD_POINTS else int(ce[-1]) // CHUNK + 1


def has_run_list(row, col):
    ce, ru = cell_list(row, col), run_list(row, col)
    return ru[-1] + 1 <= RUN_WAVE and group8_points(ce) <= FIELD_POINTS and group8_points(ru) <= FIELD_POINTS


def padded(image):
    big = np.zeros((SIDE + 2 * PAD + 16, SIDE + 2 * PAD + 16), np.int64)
    big[PAD:PAD + SIDE, PAD:PAD + SIDE] = image
    return big


def window_max(big, size, stride):
    n = (big.shape[0] - size) // stride
    out = np.zeros((n, n), np.int64)
    for dy in range(size):
        for dx in range(size):
            np.maximum(out, big[dy:dy + n * stride:stride, dx:dx + n * stride:stride], out=out)
    return out


def level2(big):
    return window_max(big, 7, 4)


def visited(row, col, P4, subs):
    """The chunks of the cell list a pass over sub-blocks `subs` = [(Y, X, sy, sx)] visits."""
    ce, ru = cell_list(row, col), run_list(row, col)
    nch = int(ce[-1]) // CHUNK + 1
    if not has_run_list(row, col):
        return set(range(nch))
    hit = np.zeros(len(row), bool)
    for Y, X, sy, sx in subs:
        hit |= P4[(row >> 2) + 2 * Y + sy, (col >> 2) + 2 * X + sx] > 0
    runs_hit = np.unique(ru[hit])
    return {int(c) for r in runs_hit for c in np.unique(ce[ru == r] // CHUNK)}


def needed(row, col, M4, subs):
    """The chunks that hold an entry with a cell that is not 0 for some pose of `subs` (M4: 4 x 4 window maxima)."""
    ce = cell_list(row, col)
    hit = np.zeros(len(row), bool)
    for Y, X, sy, sx in subs:
        hit |= M4[row + 8 * Y + 4 * sy, col + 8 * X + 4 * sx] > 0
    return {int(c) for c in np.unique(ce[hit] // CHUNK)}


def one_field_cell(bits):
    """(h): a cell E whose run has exactly one level-2 byte that is not 0 for block (1, 1) of the 17 x 17 lattice, and reads a
    cell that is not 0 at the lattice's last pose -- the first such cell in raster order."""
    from oracle import oracle as O
    big = padded(O.grid_build(target("square"), O.grid_spec(RANGE, RES, SIGMA, FLOOR_P, bits)))
    P4 = level2(big)
    for cy in range(190, 225):
        for cx in range(190, 225):
            row, col = stored_origins(point((cx, cy))[None], 0, 1, 17, 17)
            f = [int(P4[(row[0] >> 2) + 2 + sy, (col[0] >> 2) + 2 + sx] > 0) for sy in (0, 1) for sx in (0, 1)]
            if sum(f) == 1 and big[row[0] + 16, col[0] + 16] > 0:
                return (cx, cy)
    raise AssertionError("no such cell")


# ---- the child process --------------------------------------------------------------------------------------------------
def variants():
    out = {}
    for name, (env, _) in FORMS.items():
        for v, e in ((name, env), (name + "_instr", dict(env, **INSTR))):
            out[v] = e
            out[v + "_off"] = dict(e, **OFF)
    # without the sub-block bounds (NHIP_BNB_LEVELS=1) nothing writes the runs' notes: every chunk is visited
    out["split_levels1"] = dict(FORMS["split"][0], NHIP_BNB_LEVELS="1")
    out["hand_over_levels1"] = dict(FORMS["hand_over"][0], NHIP_BNB_LEVELS="1")
    return out


def counted(name):
    return name.startswith(COUNTED_CASES)


def spec_of(csm, bits):
    return csm.grid_spec(RANGE, RES, SIGMA, FLOOR_P, MAX_SHIFT, bits, skip_map=bits == 16)


def run(bits, out_path):
    from nautilus_amd import csm
    assert os.environ.get("NHIP_TUNABLES") == "1", "the forms are chosen through switches a process reads only then"
    arrays, meta = {}, {}

    def group(g, scans, n_targets, slot, spec, n_theta, nx, ny, step, count_at):
        st = csm.ScanTable.from_list(scans)
        grids = csm.LikelihoodGrids(st, np.arange(n_targets, dtype=np.int32), spec)
        n = len(scans) - n_targets
        src = np.arange(n_targets, n_targets + n, dtype=np.int32)
        th0 = np.zeros(n)
        meta[g] = {"n_pairs": n, "side": int(grids.layout.side), "pad": int(grids.layout.pad)}

        def once(search, env, src=src, slot=slot, th0=th0):
            os.environ.update(env)
            try:
                csm.bnb_stats_chunks()  # (reset)
                rec, sums = csm.match_pairs(st, grids, src, slot, th0, search)
                launch = csm.last_launch()
                stats = {k: int(v) for k, v in csm.bnb_stats_chunks().items()} if "NHIP_BNB_STATS" in env else None
            finally:
                for k in env:
                    os.environ.pop(k, None)
            return np.frombuffer(rec.tobytes(), np.uint8), sums, launch, stats

        bnb = csm.search_spec(n_theta, nx, ny, step)
        for v, env in variants().items():
            arrays["rec_%s_%s" % (g, v)], arrays["sum_%s_%s" % (g, v)], meta[g][v], _ = once(bnb, env)
            if "_instr" in v and not v.startswith("fused") and not v.startswith("split_rounds"):  # counted one pair at a time
                meta[g][v + "_counts"] = {str(i): once(bnb, env, src[i:i + 1], slot[i:i + 1], th0[i:i + 1])[3] for i in count_at}
        ex = csm.search_spec(n_theta, nx, ny, step, exhaustive=True)
        for name, env in EVERY_ADD.items():
            arrays["rec_%s_%s" % (g, name)], arrays["sum_%s_%s" % (g, name)], _, _ = once(ex, env)
        grids.close()
        st.close()

    for nx, ny, n_theta in LATTICES:
        srcs = sources(nx, ny, bits)
        slot = np.array([TARGETS.index(t) for _, t, _ in srcs], np.int32)
        count_at = [i for i, (name, _, _) in enumerate(srcs) if counted(name)] if n_theta == 1 else []
        group("%dx%dx%d" % (n_theta, nx, ny), [target(t) for t in TARGETS] + [scan(c) for _, _, c in srcs], len(TARGETS), slot,
              spec_of(csm, bits), n_theta, nx, ny, THETA_STEP, count_at)
    # (g) the lattice's edge: tests/lattice_edge.py's inputs on their own geometry
    srcs = L.sources(9, 9, bits)
    slot = np.array([L.TARGETS.index(t) for _, t, _, _ in srcs], np.int32)
    group("edge", [L.target(t) for t in L.TARGETS] + [S.cluster(cell, n) for _, _, cell, n in srcs], len(L.TARGETS), slot,
          L.spec_of(csm, bits), 1, 9, 9, L.THETA_STEP, [])
    np.savez(out_path, meta=np.array(json.dumps(meta)), **arrays)


if __name__ == "__main__":
    run(int(sys.argv[1]), sys.argv[2])
