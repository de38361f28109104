#!/usr/bin/env python3
"""How much of what the exact sums of the candidates' phase load is empty (CPU only: numpy and the oracle).

tools/pair_pass_study.py's numpy restatement of the candidates' phase of the branch-and-bound matcher (nhip_bnb.hip) on N pairs
sampled from the bench list -- the same bounds, seeds, best-first rotations, strips, whole blocks from WHOLE_MIN live valid
sub-blocks on, one serial worker per pair -- with a tally at every pass of exact sums: a whole block (8 row loads per entry
chunk) and a sub-block (4).  The rotation's cell list is merged by stored cell as cache_origins does (consecutive points with
one window origin are one entry, cut at every 64th point) and taken in chunks of 64 entries.  An entry is NOT EMPTY for a pass
if the 7 x 7 level-2 maximum of any sub-block of the pass is > 0 at the entry's origin's 4 x 4 level-2 entry: only such an entry
can add to a pose's sum.  Three counts of row loads (wave-level: one per chunk and row):
  all chunks           what the kernels issue when every pass walks the whole list
  chunks not empty     only the chunks that hold an entry that is not empty (a wave-uniform mask per pass; no compaction)
  compacted            the list compacted to the entries that are not empty, per pass

    python tools/zero_chunk_study.py [N pairs, default 24] [seed, default 1]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402
import pair_pass_study as P  # noqa: E402
from oracle import oracle as O  # noqa: E402

B, B4, WHOLE_MIN, STRIP, WAVES = P.B, P.B4, P.WHOLE_MIN, P.STRIP, P.WAVES
N_THETA, NX, NY, NBX, NBY = P.N_THETA, P.NX, P.NY, P.NBX, P.NBY
CHUNK = 64


def merged_entries(row, col):
    """Index of the first point of every entry of the merged cell list."""
    n = len(row)
    head = np.ones(n, bool)
    head[1:] = (row[1:] != row[:-1]) | (col[1:] != col[:-1])
    head[np.arange(n) % CHUNK == 0] = True
    return np.nonzero(head)[0]


def study_pair(src_pts, tgt_pts, th0, gs, count):
    side = O.grid_side(gs)
    img = O.grid_build(tgt_pts, gs)
    vol = O.csm_scores(src_pts, img, gs, th0, O.search_spec(N_THETA, NX, NY, P.THETA_STEP)).astype(np.int64)  # [k, ix, iy]
    pad = 2 * max(P.HX, P.HY) + 32
    big = np.zeros((side + 2 * pad, side + 2 * pad), img.dtype)
    big[pad:pad + side, pad:pad + side] = img
    p1, p2 = P.window_max(big, 2 * B - 1, B).astype(np.int64), P.window_max(big, 2 * B4 - 1, B4).astype(np.int64)
    l1 = np.zeros((N_THETA, NBY, NBX), np.int64)
    l2 = np.zeros((N_THETA, 2 * NBY, 2 * NBX), np.int64)
    ent = []  # per rotation: (row >> 2, col >> 2) of the merged list's entries
    for k in range(N_THETA):
        row, col = P.origins(src_pts, th0, k, gs.res, side, pad)
        for Y in range(NBY):
            for X in range(NBX):
                l1[k, Y, X] = p1[np.minimum((row >> 3) + Y, p1.shape[0] - 1), np.minimum((col >> 3) + X, p1.shape[1] - 1)].sum()
        for y in range(2 * NBY):
            for x in range(2 * NBX):
                l2[k, y, x] = p2[np.minimum((row >> 2) + y, p2.shape[0] - 1), np.minimum((col >> 2) + x, p2.shape[1] - 1)].sum()
        e = merged_entries(row, col)
        ent.append((row[e] >> 2, col[e] >> 2))
    best = [0]

    def tally(k, subs, rows):
        """One pass over the sub-blocks `subs` = [(y, x)] (level-2 indices) of rotation k, `rows` row loads per chunk."""
        r2, c2 = ent[k]
        live = np.zeros(len(r2), bool)
        for y, x in subs:
            live |= p2[np.minimum(r2 + y, p2.shape[0] - 1), np.minimum(c2 + x, p2.shape[1] - 1)] > 0
        nch = (len(r2) + CHUNK - 1) // CHUNK
        count["passes_whole" if rows == 8 else "passes_sub"] += 1
        count["entries"] += len(r2)
        count["entries_live"] += int(live.sum())
        count["loads_all"] += rows * nch
        count["loads_chunks"] += rows * len(np.unique(np.nonzero(live)[0] // CHUNK))
        count["loads_compact"] += rows * ((int(live.sum()) + CHUNK - 1) // CHUNK)

    def exact(k, x0, x1, y0, y1):
        v = vol[k, x0:min(x1, NX), y0:min(y1, NY)]
        if v.size:
            best[0] = max(best[0], int(v.max()))

    def strip(k, Y, xs):
        masks = [0, 0]
        for t, X in enumerate(xs):
            if l1[k, Y, X] < best[0]:
                continue
            vy, vx = P.extent(NY, Y), P.extent(NX, X)
            alive = [(sy, sx) for sy in (0, 1) for sx in (0, 1)
                     if B4 * sx < vx and B4 * sy < vy and l2[k, 2 * Y + sy, 2 * X + sx] >= best[0] and l2[k, 2 * Y + sy, 2 * X + sx] > 0]
            if len(alive) >= WHOLE_MIN:
                tally(k, [(2 * Y + sy, 2 * X + sx) for sy in (0, 1) for sx in (0, 1)], 8)
                exact(k, B * X, B * X + B, B * Y, B * Y + B)
                continue
            for sy, sx in alive:
                masks[sy] |= 1 << (2 * t + sx)
        for sy, m in enumerate(masks):
            for c in range(2 * STRIP):
                if (m >> c) & 1 and l2[k, 2 * Y + sy, 2 * xs[0] + c] >= best[0]:
                    tally(k, [(2 * Y + sy, 2 * xs[0] + c)], 4)
                    x0 = B * xs[0] + B4 * c
                    exact(k, x0, x0 + B4, B * Y + B4 * sy, B * Y + B4 * sy + B4)

    done = set()
    for w in range(WAVES):  # the seeds: every wave's highest-bound block, ties to the largest (rotation, block index)
        ks = list(range(w, N_THETA, WAVES))
        u, k, b = max((int(l1[k, Y, X]), k, 11 * Y + X) for k in ks for Y in range(NBY) for X in range(NBX))
        if u > 0:
            strip(k, b // 11, [b % 11])
            done.add((k, b // 11, b % 11))
    for k in sorted(range(N_THETA), key=lambda k: -int(l1[k].max())):  # best first
        for Y in range(NBY):
            xs = []
            for X in range(NBX + 1):
                live = X < NBX and (k, Y, X) not in done and l1[k, Y, X] >= best[0] and l1[k, Y, X] > 0
                if live:
                    xs.append(X)
                if xs and (not live or len(xs) == STRIP):
                    strip(k, Y, xs)
                    xs = []
    assert best[0] == int(vol.max()), "the search lost the optimum"


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 24
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    wl = bench.Workload("weak", 1)
    gs = O.grid_spec(cell_bits=16)
    pick = np.random.default_rng(seed).choice(wl.n_pairs, size=n, replace=False)
    count = dict.fromkeys(("passes_whole", "passes_sub", "entries", "entries_live", "loads_all", "loads_chunks", "loads_compact"), 0)
    for i in pick:
        s, t = int(wl.src[i]), int(wl.tgt[i])
        study_pair(wl.xy[wl.off[s]:wl.off[s + 1]], wl.xy[wl.off[t]:wl.off[t + 1]], float(wl.th0[i]), gs, count)
    cut = lambda key: 100.0 * (count[key] / max(count["loads_all"], 1) - 1.0)
    print("| sample | passes (whole + sub-block) | entries with a non-zero window | row loads, all chunks | only chunks that hold a "
          "non-zero entry | list compacted to non-zero entries |\n|---|---|---|---|---|---|")
    print("| %d pairs, seed %d | %s + %s | %.1f %% | %s | %s (%.1f %%) | %s (%.1f %%) |"
          % (n, seed, format(count["passes_whole"], ","), format(count["passes_sub"], ","),
             100.0 * count["entries_live"] / max(count["entries"], 1), format(count["loads_all"], ","),
             format(count["loads_chunks"], ","), cut("loads_chunks"), format(count["loads_compact"], ","), cut("loads_compact")))


if __name__ == "__main__":
    main()
