#!/usr/bin/env python3
"""How often two live sub-blocks lie side by side on a strip's sub-block row (CPU only: numpy and the oracle).

A numpy restatement of the candidates' phase of the branch-and-bound matcher (nhip_bnb.hip) on N pairs sampled from the
bench list: the oracle's 16-bit tables and `csm_scores` volumes; level-1 and level-2 bounds as the 15 x 15 and 7 x 7 maxima of
the cells an 8 x 8 block / 4 x 4 sub-block can reach from a point's window origin, summed over the points (slightly tighter
than the kernels' ceil(max / 257) bytes); every wave's seed its highest-bound block; then the rotations best first, their
live blocks in strips of up to three neighbours, a block whole from WHOLE_MIN live valid sub-blocks on, the lattice's edge
masked (81 = 8 * 10 + 1), ONE serial worker per pair (the best rises sooner than among the kernel's waves).

THE PAIRING RULE.  The live valid sub-blocks of a strip's blocks that do not go whole are noted per sub-block row sy as bit
2 t + sx (t: the block's place in the strip).  Walking a row from the left, a set bit whose right neighbour is set too is ONE
pass with it (4 rows x 12 bytes per list entry: the load a whole block issues covers both) -- inside a block when the left bit
is even, across a block boundary when it is odd; any other set bit is a pass of its own (4 rows x 8 bytes).  Each pair saves
one pass of 4 row loads.

    python tools/pair_pass_study.py [N pairs, default 120] [seed, default 1]"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from oracle import oracle as O  # noqa: E402

B, B4, WHOLE_MIN, STRIP, WAVES = 8, 4, 3, 3, 8
N_THETA, NX, NY, THETA_STEP = 21, 81, 81, math.radians(1.0)
HX, HY = (NX - 1) // 2, (NY - 1) // 2
NBX, NBY = (NX + B - 1) // B, (NY + B - 1) // B


def window_max(img, size, stride):
    """out[i, j] = max of img[stride i : stride i + size, stride j : stride j + size] (zero beyond the image)."""
    n = img.shape[0] // stride
    pad = np.zeros((n * stride + size, n * stride + size), img.dtype)
    pad[:img.shape[0], :img.shape[1]] = img
    out = np.zeros((n, n), img.dtype)
    for dy in range(size):
        for dx in range(size):
            np.maximum(out, pad[dy:dy + n * stride:stride, dx:dx + n * stride:stride], out=out)
    return out


def origins(pts, th0, k, res, side, pad):
    """(row, col) in the padded image of the cell pose (0, 0) of rotation k reads for every point (float32 rotation)."""
    d = (k - (N_THETA - 1) // 2) * THETA_STEP
    cf = np.float32(math.cos(th0) * math.cos(d) - math.sin(th0) * math.sin(d))
    sf = np.float32(math.sin(th0) * math.cos(d) + math.cos(th0) * math.sin(d))
    x, y = pts[:, 0].astype(np.float32), pts[:, 1].astype(np.float32)
    xr = (cf * x).astype(np.float32) - (sf * y).astype(np.float32)
    yr = (sf * x).astype(np.float32) + (cf * y).astype(np.float32)
    col = side // 2 + np.floor(xr.astype(np.float64) / res).astype(np.int64) - HX + pad
    row = side // 2 + np.floor(yr.astype(np.float64) / res).astype(np.int64) - HY + pad
    lim = side + 2 * pad - 1
    return np.clip(row, 0, lim), np.clip(col, 0, lim)


def extent(n, b):
    return min(max(n - B * b, 0), B)


def walk(mask):
    pairs = across = singles = 0
    c = 0
    while mask >> c:
        if (mask >> c) & 1:
            if (mask >> (c + 1)) & 1:
                pairs, across, c = pairs + 1, across + (c & 1), c + 1
            else:
                singles += 1
        c += 1
    return pairs, across, singles


def study_pair(src_pts, tgt_pts, th0, gs, count):
    side = O.grid_side(gs)
    img = O.grid_build(tgt_pts, gs)
    vol = O.csm_scores(src_pts, img, gs, th0, O.search_spec(N_THETA, NX, NY, THETA_STEP)).astype(np.int64)  # [k, ix, iy]
    pad = 2 * max(HX, HY) + 32
    big = np.zeros((side + 2 * pad, side + 2 * pad), img.dtype)
    big[pad:pad + side, pad:pad + side] = img
    p1, p2 = window_max(big, 2 * B - 1, B).astype(np.int64), window_max(big, 2 * B4 - 1, B4).astype(np.int64)
    l1 = np.zeros((N_THETA, NBY, NBX), np.int64)
    l2 = np.zeros((N_THETA, 2 * NBY, 2 * NBX), np.int64)
    for k in range(N_THETA):
        row, col = origins(src_pts, th0, k, gs.res, side, pad)
        for Y in range(NBY):
            for X in range(NBX):
                l1[k, Y, X] = p1[np.minimum((row >> 3) + Y, p1.shape[0] - 1), np.minimum((col >> 3) + X, p1.shape[1] - 1)].sum()
        for y in range(2 * NBY):
            for x in range(2 * NBX):
                l2[k, y, x] = p2[np.minimum((row >> 2) + y, p2.shape[0] - 1), np.minimum((col >> 2) + x, p2.shape[1] - 1)].sum()
    best = [0]

    def exact(k, x0, x1, y0, y1):
        v = vol[k, x0:min(x1, NX), y0:min(y1, NY)]
        if v.size:
            best[0] = max(best[0], int(v.max()))

    def strip(k, Y, xs):
        count["blocks"] += len(xs)
        masks = [0, 0]
        for t, X in enumerate(xs):
            if l1[k, Y, X] < best[0]:
                continue
            vy, vx = extent(NY, Y), extent(NX, X)
            alive = [(sy, sx) for sy in (0, 1) for sx in (0, 1)
                     if B4 * sx < vx and B4 * sy < vy and l2[k, 2 * Y + sy, 2 * X + sx] >= best[0] and l2[k, 2 * Y + sy, 2 * X + sx] > 0]
            if len(alive) >= WHOLE_MIN:
                count["whole"] += 1
                exact(k, B * X, B * X + B, B * Y, B * Y + B)
                continue
            if len(alive) == 1:
                count["one_live"] += 1
            elif len(alive) == 2:
                count["two_beside" if alive[0][0] == alive[1][0] else ("two_above" if alive[0][1] == alive[1][1] else "two_diagonal")] += 1
            for sy, sx in alive:
                masks[sy] |= 1 << (2 * t + sx)
        for sy, m in enumerate(masks):
            # (the passes are counted as the parent takes them, one per sub-block still alive at its turn; the pairs as the
            #  walk would have joined them)
            p, a, _ = walk(sum(1 << c for c in range(2 * STRIP) if (m >> c) & 1 and l2[k, 2 * Y + sy, 2 * xs[0] + c] >= best[0]))
            count["pairs_in_block"] += p - a
            count["pairs_across"] += a
            for c in range(2 * STRIP):
                if (m >> c) & 1 and l2[k, 2 * Y + sy, 2 * xs[0] + c] >= best[0]:
                    count["sub_passes"] += 1
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
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 120
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    wl = bench.Workload("weak", 1)
    gs = O.grid_spec(cell_bits=16)
    pick = np.random.default_rng(seed).choice(wl.n_pairs, size=n, replace=False)
    count = dict.fromkeys(("blocks", "whole", "sub_passes", "one_live", "two_beside", "two_above", "two_diagonal", "pairs_in_block", "pairs_across"), 0)
    for i in pick:
        s, t = int(wl.src[i]), int(wl.tgt[i])
        study_pair(wl.xy[wl.off[s]:wl.off[s + 1]], wl.xy[wl.off[t]:wl.off[t + 1]], float(wl.th0[i]), gs, count)
    rows = (("blocks refined", "blocks"), ("whole passes", "whole"), ("sub-block passes", "sub_passes"),
            ("blocks with one live sub-block", "one_live"), ("blocks with two live side by side", "two_beside"),
            ("blocks with two live one above the other", "two_above"), ("blocks with two live on a diagonal", "two_diagonal"),
            ("pairs inside a block", "pairs_in_block"), ("pairs across a block boundary", "pairs_across"))
    print("%d pairs of the bench list, seed %d\n| quantity | count |\n|---|---|" % (n, seed))
    for label, key in rows:
        print("| %s | %s |" % (label, format(count[key], ",")))
    units = 8 * count["whole"] + 4 * count["sub_passes"]
    pairs = count["pairs_in_block"] + count["pairs_across"]
    print("\npairs per sub-block pass: %.2f; exact-sum row loads saved: %.1f %% (inside a block only: %.1f %%)"
          % (pairs / max(count["sub_passes"], 1), 400.0 * pairs / max(units, 1), 400.0 * count["pairs_in_block"] / max(units, 1)))


if __name__ == "__main__":
    main()
