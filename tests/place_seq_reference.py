"""Numpy restatement of the place sequences ("Place sequences"; kernel unit K16b): a plain loop over pairs
and window offsets on the single-scan distances of tests/place_reference.py.  Nothing is imported from the product, everything
is integer.  tests/test_place_seq_cpu.py holds it to hand-worked cases; tests/test_place_seq_gpu.py holds the kernels to it byte
for byte."""
import numpy as np

from tests import place_reference as R

PAST_ONLY = R.PAST_ONLY


def single_distances(D, bits):
    """(dist int64 [n, n], shift int64 [n, n]) of every scan against every scan: dist[a, b] = min_s dist(a, b, s), shift the
    smallest minimising s.  Entries of scans without bits are computed too; the callers never use them."""
    n = len(D)
    dist, shift = np.zeros((n, n), dtype=np.int64), np.zeros((n, n), dtype=np.int64)
    for a in range(n):
        all_d = R.dist_all(D[a], D)
        dist[a], shift[a] = all_d.min(axis=1), all_d.argmin(axis=1)  # (the first minimum: the smallest shift)
    return dist, shift


def window(dist, bits, i, j, sigma, W, step):
    """(sum, norm, frames) of the pair (i, j) in direction sigma."""
    n = len(bits)
    total = norm = frames = 0
    for d in range(-W, W + 1):
        a, b = i + d * step, j + sigma * d * step
        if 0 <= a < n and 0 <= b < n and bits[a] > 0 and bits[b] > 0:
            total += int(dist[a, b])
            norm += int(bits[a]) + int(bits[b])
            frames += 1
    return total, norm, frames


def match(D, bits, ids, top_k, min_separation, max_permille, flags=0, half_window=2, step=1, tables=None):
    """(records int32 [M, K, 8], stats int64 [8]) of the list `ids` (ascending scan ids; one outside the scans is a scan without
    bits) among ALL scans D.  tables: single_distances(D, bits), if the caller has them already."""
    ids = np.asarray(ids, dtype=np.int64)
    bits = np.asarray(bits, dtype=np.int64)
    n, M, W = len(bits), len(ids), int(half_window)
    dist, shift = single_distances(D, bits) if tables is None else tables
    has_bits = lambda s: 0 <= s < n and bits[s] > 0
    rec = np.full((M, top_k, 8), -1, dtype=np.int32)
    stats = np.zeros(8, dtype=np.int64)
    stats[0] = M
    stats[5] = sum(not has_bits(int(s)) for s in ids)
    for a in range(M):
        i = int(ids[a])
        found = []
        for b in range(M):
            j = int(ids[b])
            if not abs(i - j) > min_separation or ((flags & PAST_ONLY) and not j < i) or not has_bits(i) or not has_bits(j):
                continue
            stats[1] += 1
            best = None
            for direction, sigma in ((0, 1), (1, -1)):
                total, norm, frames = window(dist, bits, i, j, sigma, W, step)
                score = (total * (2 * W + 1)) // frames
                if best is None or score < best[0]:  # (direction 0 on a tie)
                    best = (score, total, norm, frames, direction)
            score, total, norm, frames, direction = best
            if 1000 * total <= max_permille * norm:
                stats[2] += 1
                stats[6] += direction == 1
                stats[7] += frames < 2 * W + 1
                found.append((score, j, int(shift[i, j]), int(dist[i, j]), int(bits[j]), total, frames, direction))
        found.sort()
        for k, (score, j, sh, d, bj, total, frames, direction) in enumerate(found[:top_k]):
            rec[a, k] = (j, sh, d, bj, score, total, frames, direction)
        stats[3] += min(len(found), top_k)
        stats[4] += not found
    return rec, stats
