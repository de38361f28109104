"""Numpy restatement of the place descriptors ("Place descriptors"; kernel unit K16).  Nothing is
imported from the product: the tables are an argument, every float operation is a numpy float32 operation rounded on its
own, and everything after the two comparisons per point is integer.  tests/test_place_cpu.py holds it to hand-built cases;
tests/test_place_gpu.py holds the kernels to it byte for byte."""
import math

import numpy as np

SECTORS = 64
PAST_ONLY = 1
f32 = np.float32


def make_tables(n_rings, range_max):
    """(edge2 float32 [R + 1], dir float32 [32, 2]) by the formulas of the spec."""
    e = np.array([f32(float(f32(range_max)) * k / n_rings) for k in range(n_rings + 1)], dtype=f32)
    j = np.arange(32)
    d = np.stack([np.cos(2.0 * math.pi * j / SECTORS), np.sin(2.0 * math.pi * j / SECTORS)], axis=1).astype(f32)
    return (e * e).astype(f32), d


def point_bins(points, edge2, dirs):
    """(ring, sector) int64 per point; ring -1: the point is dropped."""
    p = np.asarray(points, dtype=f32).reshape(-1, 2)
    x, y = p[:, 0], p[:, 1]
    n_rings = len(edge2) - 1
    with np.errstate(invalid="ignore", over="ignore"):
        r2 = ((x * x).astype(f32) + (y * y).astype(f32)).astype(f32)
        keep = np.isfinite(r2) & (r2 < edge2[n_rings])
        ring = (r2[:, None] >= edge2[None, 1:n_rings]).sum(axis=1)
        neg = (y < 0) | ((y == 0) & (x < 0))
        u, v = np.where(neg, -x, x).astype(f32), np.where(neg, -y, y).astype(f32)
        cross = ((dirs[None, 1:, 0] * v[:, None]).astype(f32) - (dirs[None, 1:, 1] * u[:, None]).astype(f32)).astype(f32)
        sector = (cross >= 0).sum(axis=1) + np.where(neg, 32, 0)
    return np.where(keep, ring, -1).astype(np.int64), sector.astype(np.int64)


def describe(xy, offsets, edge2, dirs):
    """(D uint64 [n_scans, R], bits int32 [n_scans])."""
    xy = np.asarray(xy, dtype=f32).reshape(-1, 2)
    off = np.asarray(offsets, dtype=np.int64)
    n, n_rings = len(off) - 1, len(edge2) - 1
    D = np.zeros((n, n_rings), dtype=np.uint64)
    for s in range(n):
        ring, sector = point_bins(xy[off[s]:off[s + 1]], edge2, dirs)
        for r, c in set(zip(ring[ring >= 0].tolist(), sector[ring >= 0].tolist())):
            D[s, r] |= np.uint64(1) << np.uint64(c)
    return D, np.bitwise_count(D).sum(axis=1).astype(np.int32)


def rotl64(d, s):
    d, s = np.asarray(d, dtype=np.uint64), int(s) % 64
    return d if s == 0 else (d << np.uint64(s)) | (d >> np.uint64(64 - s))


def dist_shift(Di, Dj, s):
    """dist(i, j, s) of two descriptors."""
    return int(np.bitwise_count(np.asarray(Di, dtype=np.uint64) ^ rotl64(Dj, s)).sum())


def dist_all(Di, D):
    """dist(i, j, s) of one query against every row of D: int64 [len(D), 64]."""
    rot = np.stack([rotl64(D, s) for s in range(SECTORS)], axis=1)  # [n, 64, R]
    return np.bitwise_count(np.asarray(Di, dtype=np.uint64)[None, None, :] ^ rot).sum(axis=2).astype(np.int64)


def match(D, bits, ids, top_k, min_separation, max_permille, flags=0):
    """(records int32 [M, K, 4], stats int64 [8]) of the list `ids` (strictly ascending scan ids)."""
    ids = np.asarray(ids, dtype=np.int64)
    bits = np.asarray(bits, dtype=np.int64)
    M = len(ids)
    rec = np.full((M, top_k, 4), -1, dtype=np.int32)
    stats = np.zeros(8, dtype=np.int64)
    stats[0] = M
    stats[5] = int((bits[ids] == 0).sum())
    for a in range(M):
        i = int(ids[a])
        found = []
        if bits[i] > 0:
            all_d = dist_all(D[i], D[ids])
            for b in range(M):
                j = int(ids[b])
                if not abs(i - j) > min_separation or ((flags & PAST_ONLY) and not j < i) or not bits[j] > 0:
                    continue
                stats[1] += 1
                d = int(all_d[b].min())
                shift = int(np.argmin(all_d[b]))  # (the first minimum: the smallest shift)
                if 1000 * d <= max_permille * (int(bits[i]) + int(bits[j])):
                    stats[2] += 1
                    found.append((d, j, shift))
        found.sort()
        for k, (d, j, shift) in enumerate(found[:top_k]):
            rec[a, k] = (j, shift, d, bits[j])
        stats[3] += min(len(found), top_k)
        stats[4] += not found
    return rec, stats


def theta0(shift):
    """AngleMod(-shift 2 pi / 64) of a record's shift."""
    s = np.asarray(shift, dtype=np.int64)
    w = 2.0 * math.pi / SECTORS
    return np.where(s <= 32, -s * w, (SECTORS - s) * w)
