"""Host-side callers and file formats either side of the hot path.
These stay on the host in the reference as well; they are restated here so the examples and the
end-to-end test can be driven the way nautilus drives them.  Nothing here is on the measured path.

  LCCandidateFilter::GetLCCandidates      /root/reference/src/loop_closure/lc_candidate_filter.cc:35-81
  LCMatcher::ChiSquareScore / GetPossibleMatches                 src/loop_closure/lc_matcher.cc:48-74
  pose file  "timestamp x y theta"        written solver.cc:565-579, read back main.cc:131-157
  map file   "x1,y1,x2,y2" per line       solver.cc:608-618
  HitlSlamInputMsg (two line segments)    msg/HitlSlamInputMsg.msg:1-4, solver.cc:467-478
"""
import math
import os

import numpy as np


def scatter_matrix_score(points):
    """min/max eigenvalue of the scan's scatter matrix, float32 like the reference (:35-51)."""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 2)
    if len(p) == 0:
        return float("nan")
    mean = (np.float32(1.0 / len(p)) * p.sum(axis=0, dtype=np.float32)).astype(np.float32)
    d = p - mean
    s = (d[:, :, None] * d[:, None, :]).sum(axis=0, dtype=np.float32)
    ev = np.linalg.eigvals(s.astype(np.float32)).real
    return float(min(ev) / max(ev))


def lc_candidates(poses, scans, min_distance=5.0, min_score=0.70):
    """GetLCCandidates (:64-81): walk the nodes in order, skip nodes closer than 5 m to the last
    accepted scan, accept a node if its scatter score is >= 0.70."""
    out = []
    for i in range(len(scans)):
        if out:
            last = np.asarray(poses[out[-1]][:2], dtype=np.float32)
            here = np.asarray(poses[i][:2], dtype=np.float32)
            if float(np.linalg.norm(here - last)) < min_distance:
                continue
        if scatter_matrix_score(scans[i]) >= min_score:
            out.append(i)
    return out


def scatter_scores(backend, xy, offsets):
    """ComputeScatterMatrixScore of EVERY scan in one pass of the backend (product: nhip_lc_scatter_scores)."""
    return backend.scatter_scores(xy, offsets)


def lc_candidates_from_scores(poses, scores, min_distance=5.0, min_score=0.70):
    """GetLCCandidates (lc_candidate_filter.cc:64-81) on precomputed scores: walk the nodes in order, skip nodes
    closer than 5 m (float norm of the Vector2f translations, :53-62) to the last accepted scan, accept a node whose
    score is >= 0.70.  The walk is sequential (each accept depends on the previous one) and stays on the host."""
    out = []
    P = np.asarray(poses, dtype=np.float64)
    for i in range(len(scores)):
        if out:
            d = P[i, :2].astype(np.float32) - P[out[-1], :2].astype(np.float32)
            if np.float32(np.sqrt(np.float32(d[0] * d[0]) + np.float32(d[1] * d[1]))) < min_distance:
                continue
        if scores[i] >= min_score:
            out.append(i)
    return out


def geometric_pair_gate(poses, candidates, max_range=3.5, min_separation=20, backend=None):
    """All candidate pairs (later node = source, earlier = target) that pass the geometric gate: closer than
    max_range (lc_base_max_range, default_config.lua:122) and more than min_separation nodes apart -- in place of
    LCMatcher::GetPossibleMatches' per-pair ceres::Covariance (lc_matcher.cc:28-74).  With a backend the n x n
    flags come from it (product: nhip_lc_pair_gate); the unordered pairs are then read off on the host."""
    cand = np.asarray(candidates, dtype=np.int32)
    if len(cand) == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    if backend is None:
        from .posegraph import HipBackend
        backend = HipBackend()
    flags = backend.pair_gate(poses, cand, max_range, min_separation)
    i, j = np.nonzero(flags)
    keep = cand[i] > cand[j]
    return cand[i[keep]].astype(np.int32), cand[j[keep]].astype(np.int32)


def chi_square_score(cov2x2, source_xy, target_xy):
    """ChiSquareScore (lc_matcher.cc:50-57): d^T cov^-1 d with d = target - source translation, float32
    matrix as the reference casts it; cov is the cross-covariance block of the two poses."""
    cov = np.asarray(cov2x2, dtype=np.float32).reshape(2, 2)
    d = (np.asarray(target_xy, dtype=np.float32) - np.asarray(source_xy, dtype=np.float32)).astype(np.float32)
    return float(d @ np.linalg.inv(cov) @ d)


def lc_possible_matches(source, candidates, poses, covariance_fn, max_score=5000.0, backend=None):
    """GetPossibleMatches (lc_matcher.cc:59-74): every other candidate whose chi-square score against
    `source` is below 5000.  covariance_fn(pairs) -> (n, 2, 2) float32 (PoseGraph.cross_covariances).
    With a backend the scores and flags of all pairs come from one call of its chi_square_gate (product:
    nhip_lc_chi_square_gate); without one they are taken pair by pair with chi_square_score, the numpy statement
    of the same test that the backend is checked against in tests/."""
    others = [c for c in candidates if c != source]
    if not others:
        return []
    cov = covariance_fn([(source, c) for c in others])
    if backend is not None:
        _, flags = backend.chi_square_gate(poses, [source] * len(others), others, cov, max_score)
        return [c for c, f in zip(others, flags) if f]
    out = []
    for c, m in zip(others, cov):
        if chi_square_score(m, poses[source][:2], poses[c][:2]) < max_score:
            out.append(c)
    return out


def submap_members(n_scans, targets, radius):
    """The index-window membership of a submap ("Submaps"): target t's members are the scans
    t - radius .. t + radius clipped to [0, n_scans), the anchor among them; radius 0 is one member per target.
    Returns (member_scan int32, member_offsets int32 (len(targets) + 1))."""
    radius = int(radius)
    if radius < 0:
        raise ValueError("submap_members: radius %d" % radius)
    targets = np.asarray(targets, dtype=np.int64).reshape(-1)
    if len(targets) and (targets.min() < 0 or targets.max() >= n_scans):
        raise ValueError("submap_members: target outside the %d scans" % n_scans)
    lo, hi = np.maximum(targets - radius, 0), np.minimum(targets + radius, n_scans - 1) + 1
    member_offsets = np.concatenate([[0], np.cumsum(hi - lo)]).astype(np.int32)
    member_scan = np.concatenate([np.arange(a, b) for a, b in zip(lo, hi)]) if len(targets) else np.zeros(0)
    return member_scan.astype(np.int32), member_offsets


def submap_member_affines(poses, anchor_of_member, member_scan):
    """Each member's frame in its anchor's: the entries (c, s, tx, ty) of inverse(A(anchor)) * A(member) in double, A as
    PoseArrayToAffine (slam_util.h:20-28), rounded to float32 (the cast of TransformPointcloud, slam_util.h:55-63) --
    the numpy statement of nhip_submap_member_affines (held to it bit for bit in tests/)."""
    P = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    out = np.empty((len(member_scan), 4), dtype=np.float32)
    for m, (a, b) in enumerate(zip(anchor_of_member, member_scan)):
        ca, sa, cm, sm = math.cos(P[a, 2]), math.sin(P[a, 2]), math.cos(P[b, 2]), math.sin(P[b, 2])
        dx, dy = float(P[b, 0]) - float(P[a, 0]), float(P[b, 1]) - float(P[a, 1])
        out[m] = (ca * cm + sa * sm, ca * sm - sa * cm, ca * dx + sa * dy, ca * dy - sa * dx)
    return out


def submap_clouds(xy, offsets, member_scan, member_affine, member_offsets):
    """The merged clouds of submaps, float32 as the spec has them ("Submaps"; the device form is
    nhip_submaps_gather_dev): member points (x, y) -> (((c x) + ((-s) y)) + tx, ((s x) + (c y)) + ty), every operation
    rounded to float32 on its own, in member order then point order; nothing dropped, a member id outside the scans is an
    empty member.  Returns (xy (n, 2) float32, offsets int32 (n_targets + 1)).  Product code: a backend without a device
    gather matches against these clouds passed as extra scans (examples/slam_loop.py --lc-submap)."""
    f = np.float32
    xy = np.asarray(xy, dtype=f).reshape(-1, 2)
    off = np.asarray(offsets, dtype=np.int64)
    member_scan, member_offsets = np.asarray(member_scan, dtype=np.int64), np.asarray(member_offsets, dtype=np.int64)
    aff = np.asarray(member_affine, dtype=f).reshape(-1, 4)
    n_scans, parts, out_off = len(off) - 1, [], [0]
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(len(member_offsets) - 1):
            n = 0
            for m in range(member_offsets[t], member_offsets[t + 1]):
                i = member_scan[m]
                if not 0 <= i < n_scans:
                    continue
                p = xy[off[i]:max(off[i + 1], off[i])]
                c, s, tx, ty = aff[m]
                x = ((c * p[:, 0]).astype(f) + ((-s) * p[:, 1]).astype(f)).astype(f) + tx
                y = ((s * p[:, 0]).astype(f) + (c * p[:, 1]).astype(f)).astype(f) + ty
                parts.append(np.stack([x.astype(f), y.astype(f)], axis=1))
                n += len(p)
            out_off.append(out_off[-1] + n)
    merged = np.concatenate(parts).astype(f) if parts else np.zeros((0, 2), f)
    return merged, np.asarray(out_off, dtype=np.int32)


def submap_extra_scans(xy, offsets, poses, pair_tgt, radius):
    """The host-merge route to submap tables for a backend whose match() has no submap_radius: the merged cloud of every
    distinct target of the list (members by submap_members, affines from `poses`) appended to the bag as an extra scan.
    Returns (xy, offsets, pair_tgt) with every target replaced by the id of its merged scan."""
    off = np.asarray(offsets, dtype=np.int32)
    n_scans = len(off) - 1
    targets = np.unique(np.asarray(pair_tgt))
    member_scan, member_offsets = submap_members(n_scans, targets, radius)
    aff = submap_member_affines(poses, np.repeat(targets, np.diff(member_offsets)), member_scan)
    mxy, moff = submap_clouds(xy, off, member_scan, aff, member_offsets)
    xy2 = np.concatenate([np.asarray(xy, dtype=np.float32).reshape(-1, 2), mxy])
    off2 = np.concatenate([off, off[-1] + moff[1:]]).astype(np.int32)
    return xy2, off2, (n_scans + np.searchsorted(targets, pair_tgt)).astype(np.int32)


def _freespace_planes(points, side, res):
    """One target scan's (hits, free) planes, (side, side) bool, row = y: "Free-space check" item 1."""
    half = side // 2
    p = np.asarray(points, dtype=np.float32).reshape(-1, 2)
    hits, free = np.zeros((side, side), bool), np.zeros((side, side), bool)
    with np.errstate(invalid="ignore", over="ignore"):
        fl = np.floor(p.astype(np.float64) / res)
    ok = np.isfinite(p).all(axis=1) & (fl >= -half).all(axis=1) & (fl < side - half).all(axis=1)
    ends = np.unique(fl[ok].astype(np.int64), axis=0)
    for dx, dy in ends:
        hits[half + dy, half + dx] = True
        n = max(abs(dx), abs(dy))
        k = np.arange(n, dtype=np.int64)
        free[half + (2 * k * dy + n) // (2 * n), half + (2 * k * dx + n) // (2 * n)] = True
    return hits, free & ~hits


def _dilated(hits, r):
    """hits OR-ed over every Chebyshev neighbourhood of radius r (separable, by shifted copies)."""
    out = hits.copy()
    for axis in (0, 1):
        acc = out.copy()
        for s in range(1, r + 1):
            lo, hi = [slice(None)] * 2, [slice(None)] * 2
            lo[axis], hi[axis] = slice(0, -s), slice(s, None)
            acc[tuple(hi)] |= out[tuple(lo)]
            acc[tuple(lo)] |= out[tuple(hi)]
        out = acc
    return out


def freespace_counts(xy, offsets, pair_src, pair_tgt, theta0, matches, grid_spec, search, fs_spec=None, pair_origin=None):
    """The free-space check of match records in plain numpy on the host ("Free-space check"; the device
    form is nhip_freespace_check_dev): int32 (n, 8) per pair {n_points, dropped, outside, hit, free, unknown, through, 0},
    eight -1 for a rejected record.  pair_tgt are SCAN ids (a target's planes are made from its scan here, not read from a
    slot).  Product code: a backend whose match() has no `freespace` parameter verifies its records with this
    (examples/slam_loop.py --lc-verify free-space).  fs_spec: anything with hit_radius and end_margin (None: 2 and 3)."""
    from . import csm
    f = np.float32
    xy = np.asarray(xy, dtype=f).reshape(-1, 2)
    off = np.asarray(offsets, dtype=np.int64)
    pair_src, pair_tgt = np.asarray(pair_src, dtype=np.int64), np.asarray(pair_tgt, dtype=np.int64)
    n_pairs = len(pair_src)
    radius, margin = (2, 3) if fs_spec is None else (int(fs_spec.hit_radius), int(fs_spec.end_margin))
    if not (0 <= radius <= 16 and 0 <= margin <= 64):
        raise ValueError("freespace_counts: hit_radius %d outside 0..16 or end_margin %d outside 0..64" % (radius, margin))
    side, res = csm.grid_layout(grid_spec).side, float(grid_spec.res)
    if side // 2 > 4096:
        raise ValueError("freespace_counts: a grid of side %d: side / 2 exceeds 4096" % side)
    half = side // 2
    org = np.zeros((n_pairs, 2), np.int64) if pair_origin is None else np.asarray(pair_origin, dtype=np.int64).reshape(n_pairs, 2)
    rot0 = csm.rot0_table(np.asarray(theta0, dtype=np.float64)) if n_pairs else np.zeros((0, 2))
    delta = csm.delta_table(search)
    counts, planes = np.zeros((n_pairs, 8), np.int32), {}
    for i in range(n_pairs):
        m = matches[i]
        if m["itheta"] < 0:
            counts[i] = -1
            continue
        t = int(pair_tgt[i])
        if t not in planes:
            hits, free = _freespace_planes(xy[off[t]:off[t + 1]], side, res)
            planes[t] = (hits, free, _dilated(hits, radius))
        hits, free, near = planes[t]
        c0, s0 = rot0[i]
        cd, sd = delta[int(m["itheta"])]
        cf, sf = f(c0 * cd - s0 * sd), f(s0 * cd + c0 * sd)  # (double products and sums, each rounded, then to float)
        q = xy[off[pair_src[i]]:off[pair_src[i] + 1]]
        shift = org[i] + (int(m["ix"]) - (search.nx - 1) // 2, int(m["iy"]) - (search.ny - 1) // 2)
        with np.errstate(invalid="ignore", over="ignore"):
            v = np.stack([(cf * q[:, 0]).astype(f) - (sf * q[:, 1]).astype(f), (sf * q[:, 0]).astype(f) + (cf * q[:, 1]).astype(f)], axis=1).astype(f)
            fin = np.isfinite(v).all(axis=1)
            fl = np.floor(v.astype(np.float64) / res)
            short = fin & (np.abs(fl) <= 4096).all(axis=1)
        d = np.where(short[:, None], fl, 0).astype(np.int64)
        cell = half + d + shift
        inside = short & (cell >= 0).all(axis=1) & (cell < side).all(axis=1)
        cx, cy = cell[inside, 0], cell[inside, 1]
        is_hit = near[cy, cx]
        is_free = ~is_hit & free[cy, cx]
        through = 0
        o = half + shift
        beams, copies = np.unique(d[inside], axis=0, return_counts=True)  # (equal offsets, equal rays)
        for (dx, dy), mult in zip(beams, copies):
            n = max(abs(dx), abs(dy))
            k = np.arange(max(n - margin, 0), dtype=np.int64)
            if not len(k):
                continue
            rx, ry = o[0] + (2 * k * dx + n) // (2 * n), o[1] + (2 * k * dy + n) // (2 * n)
            ok = (rx >= 0) & (rx < side) & (ry >= 0) & (ry < side)
            if hits[ry[ok], rx[ok]].any():
                through += int(mult)
        counts[i] = (len(q), int((~fin).sum()), int((fin & ~inside).sum()), int(is_hit.sum()), int(is_free.sum()),
                     int((~is_hit & ~is_free).sum()), through, 0)
    return counts


def transient_spec_check(spec):
    """The accepted ranges of nhip_transient_spec_t (include/nautilus_hip.h); ValueError otherwise."""
    res = float(spec.res)
    if not (math.isfinite(res) and res > 0):
        raise ValueError("transient_filter: res must be finite and > 0")
    for name, lo, hi in (("width", 1, 16384), ("height", 1, 16384), ("support_radius", 0, 4), ("min_through", 1, 1 << 30),
                         ("transient_permille", 0, 1000), ("flags", 0, 0), ("reserved", 0, 0)):
        if not lo <= int(getattr(spec, name)) <= hi:
            raise ValueError("transient_filter: %s %d outside %d..%d" % (name, int(getattr(spec, name)), lo, hi))


def transient_filter(xy, offsets, poses, spec, hits, misses):
    """Transient returns in plain numpy on the host ("Transient returns"; the device form is
    nhip_transient_filter_dev, and transient.filter returns the same five arrays bit for bit): every return of the packed
    scans at `poses` classified by the occupancy planes `hits` and `misses` (int32 (H, W), read only) under it, the returns
    that are not transient packed.  spec: anything with the fields of nhip_transient_spec_t (transient.spec_from(occupancy
    spec)).  Returns (out_xy float32 (kept, 2), out_offsets int32 (n_scans + 1,), out_index int32 (kept,), labels uint8
    (n_points,): 0 static, 1 transient, 2 unobserved, 3 invalid, stats int64 (8,): transient.STATS_FIELDS).  The hit support
    S of a cell is read from a summed-area table of `hits`.  A scan whose offsets are not a scan is empty and counted
    (stats[5]); nothing is raised for it."""
    from .vectorize import pose_affines
    transient_spec_check(spec)
    f = np.float32
    xy = np.ascontiguousarray(xy, dtype=f).reshape(-1, 2)
    off = np.asarray(offsets, dtype=np.int64)
    n_scans, n_points = len(off) - 1, len(xy)
    aff = pose_affines(poses)
    if len(aff) != n_scans:
        raise ValueError("transient_filter: %d poses for %d scans" % (len(aff), n_scans))
    w, h, r, res = int(spec.width), int(spec.height), int(spec.support_radius), float(spec.res)
    x0, y0 = int(spec.cell_x0), int(spec.cell_y0)
    H = np.asarray(hits).reshape(h, w).astype(np.int64)
    M = np.asarray(misses).reshape(h, w).astype(np.int64)
    area = np.zeros((h + 1, w + 1), np.int64)  # area[y, x] = the sum of H[:y, :x] (< 2^59: no sum wraps)
    area[1:, 1:] = H.cumsum(axis=0).cumsum(axis=1)
    labels = np.full(n_points, 3, np.uint8)
    stats, index, out_off = np.zeros(8, np.int64), [], np.zeros(n_scans + 1, np.int32)
    stats[4], n_kept = n_scans, 0
    for i in range(n_scans):
        b, e = int(off[i]), int(off[i + 1])
        out_off[i] = n_kept
        if b < 0 or e < b or e > n_points:
            stats[5] += 1
            continue
        p = xy[b:e]
        c, s, tx, ty = (f(v) for v in aff[i])
        with np.errstate(invalid="ignore", over="ignore"):
            wx = ((c * p[:, 0]).astype(f) + ((-s) * p[:, 1]).astype(f)).astype(f) + tx
            wy = ((s * p[:, 0]).astype(f) + (c * p[:, 1]).astype(f)).astype(f) + ty
            wpt = np.stack([wx.astype(f), wy.astype(f)], axis=1).astype(np.float64)
            fl = np.floor(wpt / res)
            valid = np.isfinite(p).all(axis=1) & np.isfinite(wpt).all(axis=1) & (np.abs(fl) < 2.0 ** 62).all(axis=1)
        lab = np.full(len(p), 3, np.uint8)
        cell = np.where(valid[:, None], fl, 0.0).astype(np.int64) - (x0, y0)  # (window coordinates, int64)
        inside = valid & (cell >= 0).all(axis=1) & (cell[:, 0] < w) & (cell[:, 1] < h)
        lab[valid & ~inside] = 2
        cx, cy = cell[inside, 0], cell[inside, 1]
        xa, xb = np.maximum(cx - r, 0), np.minimum(cx + r, w - 1) + 1
        ya, yb = np.maximum(cy - r, 0), np.minimum(cy + r, h - 1) + 1
        S = area[yb, xb] - area[ya, xb] - area[yb, xa] + area[ya, xa]
        m = M[cy, cx]
        lab[inside] = ((m >= int(spec.min_through)) & (1000 * S <= int(spec.transient_permille) * (S + m))).astype(np.uint8)
        labels[b:e] = lab
        stats[:4] += np.bincount(lab, minlength=4)
        kept = np.nonzero((lab & 1) == 0)[0]
        stats[6] += int(len(p) > 0 and len(kept) == 0)
        index.append((b + kept).astype(np.int32))
        n_kept += len(kept)
    out_index = np.concatenate(index).astype(np.int32) if index else np.zeros(0, np.int32)
    out_off[n_scans] = len(out_index)
    return xy[out_index], out_off, out_index, labels, stats


def place_descriptors(xy, offsets, spec):
    """The ring descriptors of the packed scans in plain numpy ("Place descriptors"; the device form is
    nhip_place_describe_dev): (D uint64 (n_scans, R), bits int32 (n_scans,)).  The tables are the library's
    (nhip_place_tables: pure host)."""
    from . import place
    f = np.float32
    edge2, dirs = place.tables(spec)
    R = int(spec.n_rings)
    p = np.asarray(xy, dtype=f).reshape(-1, 2)
    off = np.asarray(offsets, dtype=np.int64)
    x, y = p[:, 0], p[:, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        r2 = ((x * x).astype(f) + (y * y).astype(f)).astype(f)
        kept = np.isfinite(r2) & (r2 < edge2[R])
        ring = np.searchsorted(edge2[1:R], r2, side="right")  # (#{k: r2 >= edge2[k]}: the edges ascend)
        neg = (y < 0) | ((y == 0) & (x < 0))
        u, v = np.where(neg, -x, x).astype(f), np.where(neg, -y, y).astype(f)
        sector = np.where(neg, 32, 0)
        for j in range(1, 32):
            sector = sector + (((dirs[j, 0] * v).astype(f) - (dirs[j, 1] * u).astype(f)).astype(f) >= 0)
    scan = np.repeat(np.arange(len(off) - 1), np.diff(off))
    D = np.zeros((len(off) - 1, R), dtype=np.uint64)
    np.bitwise_or.at(D, (scan[kept], ring[kept]), np.uint64(1) << sector[kept].astype(np.uint64))
    return D, np.bitwise_count(D).sum(axis=1).astype(np.int32)


def place_candidates(xy, offsets, ids, spec=None):
    """Loop-closure candidates by appearance in plain numpy on the host (the device form is nhip_place_candidates): (records
    int32 (n_ids, K, 4) = {j, shift, dist, bits_j}, four -1 where unfilled; stats int64 (8,)).  Product code: a backend
    without place_candidates() proposes its pairs with this (examples/slam_loop.py --lc-gate appearance)."""
    from . import place
    spec = place.default_spec() if spec is None else spec
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    n_scans = len(offsets) - 1
    if len(ids) and (ids[0] < 0 or ids[-1] >= n_scans or (np.diff(ids) <= 0).any()):
        raise ValueError("place_candidates: ids must ascend strictly inside the %d scans" % n_scans)
    R, K = int(spec.n_rings), int(spec.top_k)
    if not (1 <= R <= 15 and 1 <= K <= 32 and spec.min_separation >= 0 and 0 <= spec.max_permille <= 1000):
        raise ValueError("place_candidates: n_rings 1..15, top_k 1..32, min_separation >= 0, max_permille 0..1000")
    D, bits = place_descriptors(xy, offsets, spec)
    D, bits = D[ids], bits[ids].astype(np.int64)
    M = len(ids)
    rec, stats = np.full((M, K, 4), -1, dtype=np.int32), np.zeros(8, dtype=np.int64)
    stats[0], stats[5] = M, int((bits == 0).sum())
    if M == 0:
        return rec, stats
    # rotl64(D_j, s) for every candidate and shift, once: (M, 64, R)
    s = np.arange(1, 64, dtype=np.uint64)[None, :, None]
    rot = np.concatenate([D[:, None, :], (D[:, None, :] << s) | (D[:, None, :] >> (np.uint64(64) - s))], axis=1)
    for a in range(M):
        adm = (np.abs(ids - ids[a]) > spec.min_separation) & (bits > 0) & (bits[a] > 0)
        if spec.flags & place.NHIP_PLACE_PAST_ONLY:
            adm &= ids < ids[a]
        b = np.nonzero(adm)[0]
        stats[1] += len(b)
        if len(b):
            d = np.bitwise_count(D[a][None, None, :] ^ rot[b]).sum(axis=2).astype(np.int64)  # (len(b), 64)
            shift = d.argmin(axis=1)  # (the first minimum: the smallest shift)
            dist = d[np.arange(len(b)), shift]
            gate = 1000 * dist <= int(spec.max_permille) * (bits[a] + bits[b])
            b, shift, dist = b[gate], shift[gate], dist[gate]
            stats[2] += len(b)
            order = np.lexsort((b, dist))[:K]
            rec[a, :len(order)] = np.stack([ids[b[order]], shift[order], dist[order], bits[b[order]]], axis=1)
            stats[3] += len(order)
        stats[4] += not (rec[a, 0, 0] >= 0)
    return rec, stats


def place_sequence_candidates(xy, offsets, ids, spec=None, seq=None, descriptors=None):
    """Loop-closure candidates by sequence in plain numpy on the host ("Place sequences"; the device form
    is nhip_place_seq_candidates): (records int32 (n_ids, K, 8) = {j, shift, dist, bits_j, seq, sum, frames, direction}, eight
    -1 where unfilled; stats int64 (8,)).  The window frames are scan ids: every scan is described, not only the list's.
    descriptors: (D uint64 (n_scans, R), bits (n_scans,)) to use instead of describing xy.  Product code: a backend without
    place_sequence_candidates() proposes its pairs with this (examples/slam_loop.py --lc-gate appearance --lc-sequence W)."""
    from . import place
    spec = place.default_spec() if spec is None else spec
    seq = place.default_seq_spec() if seq is None else seq
    R, K, W, step = int(spec.n_rings), int(spec.top_k), int(seq.half_window), int(seq.step)
    if not (1 <= R <= 15 and 1 <= K <= 32 and 0 <= spec.max_permille <= 1000 and 0 <= W <= 8 and 1 <= step <= 16 and
            spec.min_separation >= 2 * W * step):
        raise ValueError("place_sequence_candidates: n_rings 1..15, top_k 1..32, max_permille 0..1000, half_window 0..8, "
                         "step 1..16, min_separation >= 2 half_window step")
    D, bits = place_descriptors(xy, offsets, spec) if descriptors is None else descriptors
    D, bits = np.asarray(D, dtype=np.uint64).reshape(-1, R), np.asarray(bits, dtype=np.int64).reshape(-1)
    n = len(bits)
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    if len(ids) and (ids[0] < 0 or ids[-1] >= n or (np.diff(ids) <= 0).any()):
        raise ValueError("place_sequence_candidates: ids must ascend strictly inside the %d scans" % n)
    M = len(ids)
    rec, stats = np.full((M, K, 8), -1, dtype=np.int32), np.zeros(8, dtype=np.int64)
    stats[0], stats[5] = M, int((bits[ids] == 0).sum())
    if M == 0:
        return rec, stats
    # rotl64(D_b, s) for every scan and shift, once: (n, 64, R); a row of single distances when a window first asks for it
    s = np.arange(1, 64, dtype=np.uint64)[None, :, None]
    rot = np.concatenate([D[:, None, :], (D[:, None, :] << s) | (D[:, None, :] >> (np.uint64(64) - s))], axis=1)
    rows = {}

    def row(a):
        if a not in rows:
            d = np.bitwise_count(D[a][None, None, :] ^ rot).sum(axis=2).astype(np.int64)  # (n, 64)
            shift = d.argmin(axis=1)  # (the first minimum: the smallest shift)
            rows[a] = (d[np.arange(n), shift], shift)
        return rows[a]

    for a in range(M):
        i = int(ids[a])
        adm = (np.abs(ids - i) > spec.min_separation) & (bits[ids] > 0) & (bits[i] > 0)
        if spec.flags & place.NHIP_PLACE_PAST_ONLY:
            adm &= ids < i
        b = np.nonzero(adm)[0]
        stats[1] += len(b)
        if len(b):
            j = ids[b]
            total, norm, frames = (np.zeros((2, len(b)), dtype=np.int64) for _ in range(3))
            for d in range(-W, W + 1):
                fa = i + d * step
                if not (0 <= fa < n and bits[fa] > 0):
                    continue
                dist_a = row(fa)[0]
                for g, sigma in enumerate((1, -1)):
                    fb = j + sigma * d * step
                    ok = (fb >= 0) & (fb < n)
                    fb = np.where(ok, fb, 0)
                    ok &= bits[fb] > 0
                    total[g] += np.where(ok, dist_a[fb], 0)
                    norm[g] += np.where(ok, bits[fa] + bits[fb], 0)
                    frames[g] += ok
            score = (total * (2 * W + 1)) // frames  # (frames >= 1: d = 0 always counts)
            direction = (score[0] > score[1]).astype(np.int64)
            at = np.arange(len(b))
            score, total, norm, frames = score[direction, at], total[direction, at], norm[direction, at], frames[direction, at]
            gate = 1000 * total <= int(spec.max_permille) * norm
            stats[2] += int(gate.sum())
            stats[6] += int((gate & (direction == 1)).sum())
            stats[7] += int((gate & (frames < 2 * W + 1)).sum())
            order = np.nonzero(gate)[0]
            order = order[np.lexsort((j[order], score[order]))][:K]
            dist_i, shift_i = row(i)
            jo = j[order]
            rec[a, :len(order)] = np.stack([jo, shift_i[jo], dist_i[jo], bits[jo], score[order], total[order], frames[order],
                                            direction[order]], axis=1)
            stats[3] += len(order)
        stats[4] += not (rec[a, 0, 0] >= 0)
    return rec, stats


def _consistency_rows(rec, rows, tol):
    """Rows `rows` of the consistency matrix of the prepared records, as booleans (len(rows), M): the pair test of DESIGN.md
    section 3, "Loop-closure consistency", every operation a float64 operation of numpy, rounded on its own."""
    M = len(rec)
    m, n = np.asarray(rows)[:, None], np.arange(M)[None, :]
    row_is_lo = m < n
    a = [np.where(row_is_lo, rec[m, k], rec[n, k]) for k in range(8)]  # lo
    b = [np.where(row_is_lo, rec[n, k], rec[m, k]) for k in range(8)]  # hi
    t0, t_rate, t_max, r0, r_rate, r_max = tol
    with np.errstate(invalid="ignore", over="ignore"):
        ihx, ihy = -((b[0] * b[2]) + (b[1] * b[3])), (b[1] * b[2]) - (b[0] * b[3])
        cq, sq = (a[0] * b[0]) + (a[1] * b[1]), (a[1] * b[0]) - (a[0] * b[1])
        qx, qy = ((a[0] * ihx) - (a[1] * ihy)) + a[2], ((a[1] * ihx) + (a[0] * ihy)) + a[3]
        ex = (((cq * a[4]) - (sq * a[5])) + qx) - a[4]
        ey = (((sq * a[4]) + (cq * a[5])) + qy) - a[5]
        e2, chord = (ex * ex) + (ey * ey), 2.0 - (2.0 * cq)
        length = np.abs(a[6] - b[6]) + np.abs(a[7] - b[7])
        tt, tr = t0 + (t_rate * length), r0 + (r_rate * length)
        tt, tr = np.where(t_max < tt, t_max, tt), np.where(r_max < tr, r_max, tr)
        return (e2 <= tt * tt) & (chord <= tr * tr) & (m != n)


def consistent_set(records, spec=None, adjacency=False):
    """The consistent set of prepared loop-closure records (consistency.prepare) in plain numpy on the host (the device form is
    nhip_consistency): (members int32 (M,) in pick order, -1 behind them; n_members; stats int64 (8,)), with adjacency=True also
    (matrix uint64 (M, W), degrees int32 (M,)).  Product code: a backend without consistent_set() filters its records with this
    (examples/slam_loop.py --lc-consistency)."""
    from . import consistency
    spec = consistency.default_spec() if spec is None else spec
    rec = np.ascontiguousarray(records, dtype=np.float64)
    if rec.ndim != 2 or rec.shape[1] != 8 or len(rec) > consistency.MAX_RECORDS:
        raise ValueError("consistent_set: records of shape %s; (M, 8) with M <= %d wanted" % (rec.shape, consistency.MAX_RECORDS))
    tol = [float(getattr(spec, k)) for k in ("t0", "t_rate", "t_max", "r0", "r_rate", "r_max")]
    if not (all(np.isfinite(v) and v >= 0 for v in tol) and tol[2] >= tol[0] and tol[5] >= tol[3] and spec.max_steps >= 1 and spec.flags == 0):
        raise ValueError("consistent_set: tolerances finite and >= 0, t_max >= t0, r_max >= r0, max_steps >= 1, flags 0")
    M, W = len(rec), (len(rec) + 63) // 64
    bits = np.zeros((M, W * 64), dtype=bool)
    for r0_ in range(0, M, 256):  # (rows in chunks: a chunk's temporaries are 256 x M doubles)
        rows = np.arange(r0_, min(r0_ + 256, M))
        bits[rows, :M] = _consistency_rows(rec, rows, tol)
    A = np.packbits(bits, axis=1, bitorder="little").view(np.uint64).reshape(M, W) if M else np.zeros((0, 0), dtype=np.uint64)
    deg = np.bitwise_count(A).sum(axis=1).astype(np.int32)
    members, stats = np.full(M, -1, dtype=np.int32), np.zeros(8, dtype=np.int64)
    stats[0] = M
    n = 0
    if M:
        stats[1], stats[2] = int(deg.sum()) // 2, int(deg.max())
        live = np.ones(M, dtype=bool)  # (C as booleans, and as words for the popcounts)
        C_words = np.packbits(np.concatenate([live, np.zeros(W * 64 - M, dtype=bool)]), bitorder="little").view(np.uint64)
        score = deg.astype(np.int64)
        cap = min(int(spec.max_steps), M)
        while True:
            idx = np.nonzero(live)[0]
            u = int(idx[np.argmax(score[idx])])  # (the first maximum: the smallest index)
            members[n] = u
            n += 1
            C_words = C_words & A[u]
            C_words[u >> 6] &= ~(np.uint64(1) << np.uint64(u & 63))
            live = np.unpackbits(C_words.view(np.uint8), bitorder="little")[:M].astype(bool)
            if not live.any() or n >= cap:
                break
            score = np.zeros(M, dtype=np.int64)
            rows = np.nonzero(live)[0]
            score[rows] = np.bitwise_count(A[rows] & C_words[None, :]).sum(axis=1)
        stats[3], stats[4] = n, int(live.any())
    return (members, n, stats, A, deg) if adjacency else (members, n, stats)


def distance_to_line_segment_f32(points, seg):
    """DistanceToLineSegment<float> (slam_util.h:92-110) for an (n, 2) float32 array: Hyperplane::Through normal,
    projection inside the endpoints' closed x and y intervals -> |signed distance|, else nearest endpoint."""
    f = np.float32
    p = np.asarray(points, dtype=f).reshape(-1, 2)
    x0, y0, x1, y1 = (f(v) for v in seg)
    dx, dy = f(x1 - x0), f(y1 - y0)
    nx, ny = f(-dy), dx
    ln = f(np.sqrt(f(f(nx * nx) + f(ny * ny))))
    nx, ny = f(nx / ln), f(ny / ln)
    off = f(-f(f(x0 * nx) + f(y0 * ny)))
    sd = (p[:, 0] * nx + p[:, 1] * ny + off).astype(f)
    prx, pry = (p[:, 0] - sd * nx).astype(f), (p[:, 1] - sd * ny).astype(f)
    between = lambda v, a, b: ((v >= a) & (v <= b)) | ((v >= b) & (v <= a))
    inside = between(prx, x0, x1) & between(pry, y0, y1)
    d0 = np.sqrt((p[:, 0] - x0) ** 2 + (p[:, 1] - y0) ** 2).astype(f)
    d1 = np.sqrt((p[:, 0] - x1) ** 2 + (p[:, 1] - y1) ** 2).astype(f)
    return np.where(inside, np.abs(sd), np.minimum(d0, d1)).astype(f)


def hitl_relevant_poses(poses, scans, line_a, line_b, line_width=0.05, point_threshold=10):
    """GetRelevantPosesForHITL (solver.cc:479-513): per node, the points (scan frame) whose world position under the
    node's pose (Affine2f, float) lies within hitl_line_width of line a -- else of line b; a node with at least
    hitl_pose_point_threshold points on a joins line_a_poses, else with that many on b joins line_b_poses.
    Returns (a_poses, b_poses): lists of (node index, points (k, 2) float32)."""
    a_poses, b_poses = [], []
    for i, pts in enumerate(scans):
        pts = np.asarray(pts, dtype=np.float32).reshape(-1, 2)
        if len(pts) == 0:
            continue
        c, s = np.float32(np.cos(poses[i][2])), np.float32(np.sin(poses[i][2]))
        tx, ty = np.float32(poses[i][0]), np.float32(poses[i][1])
        w = np.stack([c * pts[:, 0] - s * pts[:, 1] + tx, s * pts[:, 0] + c * pts[:, 1] + ty], axis=1).astype(np.float32)
        on_a = distance_to_line_segment_f32(w, line_a) <= line_width
        on_b = ~on_a & (distance_to_line_segment_f32(w, line_b) <= line_width)
        if on_a.sum() >= point_threshold:
            a_poses.append((i, pts[on_a]))
        elif on_b.sum() >= point_threshold:
            b_poses.append((i, pts[on_b]))
    return a_poses, b_poses


def write_poses(path, timestamps, poses):
    """solver.cc:573-577: std::fixed (6 decimals) 'timestamp x y theta' per node."""
    with open(path, "w") as f:
        for t, p in zip(timestamps, poses):
            f.write("%.6f %.6f %.6f %.6f\n" % (t, p[0], p[1], p[2]))


def read_poses(path):
    """main.cc:139-146: whitespace-separated double timestamp + three floats; returns {timestamp: pose}."""
    out = {}
    with open(path) as f:
        for line in f:
            parts = line.split()
            if len(parts) < 4:
                break
            out[float(parts[0])] = np.array([np.float32(parts[1]), np.float32(parts[2]), np.float32(parts[3])], dtype=np.float32)
    return out


def load_solution(path, timestamps, poses):
    """LoadSolutionFromFile (main.cc:131-157): overwrite poses whose (6-decimal) timestamp is in the file."""
    table = read_poses(path)
    poses = np.array(poses, dtype=np.float64)
    missing = []
    for i, t in enumerate(timestamps):
        key = float("%.6f" % t)
        if key in table:
            poses[i] = table[key]
        else:
            missing.append(i)
    return poses, missing


def write_map_lines(path, lines):
    """solver.cc:612-616: 'x1,y1,x2,y2' per vectorised map line (default ostream precision: 6 significant)."""
    with open(path, "w") as f:
        for l in lines:
            f.write("%g,%g,%g,%g\n" % (l[0], l[1], l[2], l[3]))


def read_map_lines(path):
    return np.array([[float(v) for v in line.split(",")] for line in open(path) if line.strip()], dtype=np.float64).reshape(-1, 4)


def map_window(poses, range_m, res):
    """The smallest raster window that holds every pose +- range_m on both axes, in world cells of `res` metres (cell of x:
    floor(x / res), cimg_debug.h:31-37): (cell_x0, cell_y0, width, height), what the map vectorisation's spec takes
    ("Map vectorisation").  No poses: the one cell at the origin."""
    P = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    if len(P) == 0:
        return 0, 0, 1, 1
    lo = np.floor((P[:, :2].min(axis=0) - float(range_m)) / float(res)).astype(np.int64)
    hi = np.floor((P[:, :2].max(axis=0) + float(range_m)) / float(res)).astype(np.int64)
    return int(lo[0]), int(lo[1]), int(hi[0] - lo[0] + 1), int(hi[1] - lo[1] + 1)


OCCUPANCY_PIXELS = ((100, 0), (0, 254), (-1, 205))  # (grid value, pixel): map_server's convention with negate 0


def write_occupancy_map(path_stem, grid, spec):
    """An occupancy grid (int8 (H, W): 100 occupied, 0 free, -1 unknown; occupancy.occupancy_grid) as the pair of files
    map_server loads: path_stem + '.pgm', a binary PGM (occupied 0, free 254, unknown 205; image row 0 = the highest y), and
    path_stem + '.yaml' beside it (plain text: image, resolution, origin = the window's corner in metres, negate,
    occupied_thresh, free_thresh).  Returns the two paths."""
    g = np.asarray(grid, dtype=np.int8)
    if g.shape != (spec.height, spec.width):
        raise ValueError("write_occupancy_map: grid of shape %s for a window of %d x %d" % (g.shape, spec.height, spec.width))
    img = np.full(g.shape, 205, np.uint8)
    for value, pixel in OCCUPANCY_PIXELS:
        img[g == value] = pixel
    pgm, yaml = path_stem + ".pgm", path_stem + ".yaml"
    with open(pgm, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (spec.width, spec.height))
        f.write(img[::-1].tobytes())
    with open(yaml, "w") as f:
        f.write("image: %s\nresolution: %r\norigin: [%r, %r, 0.0]\nnegate: 0\noccupied_thresh: %r\nfree_thresh: %r\n"
                % (os.path.basename(pgm), float(spec.res), spec.cell_x0 * float(spec.res), spec.cell_y0 * float(spec.res),
                   spec.occ_permille / 1000.0, spec.free_permille / 1000.0))
    return pgm, yaml


def read_occupancy_map(path_stem):
    """What write_occupancy_map wrote: (grid int8 (H, W), dict of the YAML's entries: image (str), resolution, origin (list),
    negate, occupied_thresh, free_thresh)."""
    info = {}
    for line in open(path_stem + ".yaml"):
        if ":" in line:
            k, v = (t.strip() for t in line.split(":", 1))
            info[k] = ([float(t) for t in v.strip("[]").split(",")] if v.startswith("[") else
                       v if k == "image" else int(v) if k == "negate" else float(v))
    raw = open(os.path.join(os.path.dirname(path_stem), info["image"]), "rb").read()
    head = raw.split(b"\n", 3)
    if head[0] != b"P5" or head[2] != b"255":
        raise ValueError("read_occupancy_map: %s is not a binary PGM with 255 levels" % info["image"])
    w, h = (int(t) for t in head[1].split())
    img = np.frombuffer(head[3], dtype=np.uint8, count=w * h).reshape(h, w)[::-1]
    grid = np.full((h, w), -1, np.int8)
    for value, pixel in OCCUPANCY_PIXELS:
        grid[img == pixel] = value
    return grid, info


def occupancy_map_window(grid, info):
    """(res, cell_x0, cell_y0, width, height) of a map read_occupancy_map returned: the YAML's origin is the window's corner in
    metres, a whole number of cells."""
    res = float(info["resolution"])
    h, w = np.asarray(grid).shape
    return res, int(round(info["origin"][0] / res)), int(round(info["origin"][1] / res)), int(w), int(h)


def mapwin_spec_check(spec):
    """The accepted ranges of nhip_mapwin_spec_t (include/nautilus_hip.h); ValueError otherwise."""
    res = float(spec.res)
    if not (math.isfinite(res) and res > 0):
        raise ValueError("map_windows: res must be finite and > 0")
    for name, lo, hi in (("width", 1, 16384), ("height", 1, 16384), ("side", 2, 8192), ("occ_min", 1, 100), ("flags", 0, 0),
                         ("reserved", 0, 0)):
        if not lo <= int(getattr(spec, name)) <= hi:
            raise ValueError("map_windows: %s %d outside %d..%d" % (name, int(getattr(spec, name)), lo, hi))


def map_window_origins(priors, res):
    """The origins of priors (n, 3) in a map of `res` metres per cell ("Map windows", item 2; held equal
    to nhip_mapwin_origins): (origins int32 (n, 2): the world cell (floor(x / res), floor(y / res)) of each, theta0 float64
    (n,): its heading).  ValueError for a pose that is not finite or 2^30 cells or more from the origin, naming its index."""
    P = np.asarray(priors, dtype=np.float64).reshape(-1, 3)
    res = float(res)
    if not (math.isfinite(res) and res > 0):
        raise ValueError("map_window_origins: res must be finite and > 0")
    bad = np.nonzero(~np.isfinite(P).all(axis=1))[0]
    if len(bad):
        raise ValueError("map_window_origins: pose %d is not finite" % bad[0])
    fl = np.floor(P[:, :2] / res)
    bad = np.nonzero((np.abs(fl) >= 2.0 ** 30).any(axis=1))[0]
    if len(bad):
        raise ValueError("map_window_origins: pose %d lies 2^30 cells or more from the origin" % bad[0])
    return fl.astype(np.int32), P[:, 2].copy()


def map_cells(grid, spec):
    """The occupied cells of an occupancy grid, row by row ("Map windows", item 1; the device form is nhip_mapwin_cells_dev):
    (row_ptr int32 (height + 1,), cols int32 (n_occ,)) -- cols[row_ptr[y]:row_ptr[y + 1]] are the local x indices of the cells
    of row y whose int8 value is >= spec.occ_min, ascending."""
    mapwin_spec_check(spec)
    g = np.asarray(grid, dtype=np.int8).reshape(int(spec.height), int(spec.width))
    ys, xs = np.nonzero(g >= int(spec.occ_min))  # (row-major: y ascending, then x ascending)
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(ys, minlength=g.shape[0]))]).astype(np.int32)
    return row_ptr, xs.astype(np.int32)


def map_windows(grid, spec, origins):
    """The windows of an occupancy grid around `origins` (n, 2) in plain numpy ("Map windows", items 3 and 5; the device form
    is nhip_mapwin_gather_dev behind nhip_mapwin_cells_dev, and localize.windows returns the same three arrays bit for bit):
    (xy float32 (n_points, 2), offsets int32 (n + 1,), stats int64 (8,): localize.STATS_FIELDS).  Window q holds the occupied
    world cells (wx, wy) with wx - ox and wy - oy in [-side/2, side - side/2 - 1], as the points ((k + 0.5) res) of the frame
    whose origin is the lower-left corner of world cell (ox, oy), y ascending then x ascending.  The capacity is unbounded
    here: the two overflow words of the stats are 0."""
    row_ptr, cols = map_cells(grid, spec)
    org = np.asarray(origins, dtype=np.int64).reshape(-1, 2)
    side, half, res = int(spec.side), int(spec.side) // 2, float(spec.res)
    w, h, x0, y0 = int(spec.width), int(spec.height), int(spec.cell_x0), int(spec.cell_y0)
    rows = np.repeat(np.arange(h, dtype=np.int64), np.diff(row_ptr))  # the map row of every entry of cols
    parts, offsets = [], np.zeros(len(org) + 1, np.int64)
    for q, (ox, oy) in enumerate(org):
        y_lo, y_hi = max(oy - half - y0, 0), min(oy - half + side - 1 - y0, h - 1)
        x_lo, x_hi = max(ox - half - x0, 0), min(ox - half + side - 1 - x0, w - 1)
        n = 0
        if y_lo <= y_hi and x_lo <= x_hi:
            b, e = int(row_ptr[y_lo]), int(row_ptr[y_hi + 1])
            c = cols[b:e].astype(np.int64)
            keep = (c >= x_lo) & (c <= x_hi)
            kx, ky = c[keep] + x0 - ox, rows[b:e][keep] + y0 - oy
            parts.append(np.stack([((kx.astype(np.float64) + 0.5) * res).astype(np.float32),
                                   ((ky.astype(np.float64) + 0.5) * res).astype(np.float32)], axis=1))
            n = len(kx)
        offsets[q + 1] = offsets[q] + n
    if offsets[-1] > 2 ** 31 - 1:
        raise ValueError("map_windows: %d points, more than 2^31 - 1" % offsets[-1])
    xy = np.concatenate(parts).astype(np.float32) if parts else np.zeros((0, 2), np.float32)
    counts = np.diff(offsets)
    stats = np.array([len(cols), len(org), offsets[-1], int((counts == 0).sum()), int(counts.max()) if len(org) else 0, 0, 0, 0], np.int64)
    return xy, offsets.astype(np.int32), stats


def localize_compose(records, origins, theta0, grid_spec, search):
    """World poses (n, 3) float64 from match records against map windows ("Map windows", item 6): the matcher's conventions
    (csm.match_to_transform) with pair_origin 0 in the frame whose origin is the corner of world cell (ox, oy), all in double:
    x = (ox + ix - (nx - 1) / 2) res, y likewise, theta = angle_mod(theta0 + (itheta - (n_theta - 1) / 2) theta_step).  A
    rejected record (itheta -1: a gated match) gives NaN."""
    rec = np.asarray(records)
    org = np.asarray(origins, dtype=np.int64).reshape(-1, 2)
    th0 = np.asarray(theta0, dtype=np.float64).reshape(-1)
    if not (len(rec) == len(org) == len(th0)):
        raise ValueError("localize_compose: %d records, %d origins, %d headings" % (len(rec), len(org), len(th0)))
    res = float(grid_spec.res)
    out = np.empty((len(rec), 3), np.float64)
    out[:, 0] = (org[:, 0] + rec["ix"].astype(np.int64) - (int(search.nx) - 1) // 2).astype(np.float64) * res
    out[:, 1] = (org[:, 1] + rec["iy"].astype(np.int64) - (int(search.ny) - 1) // 2).astype(np.float64) * res
    a = th0 + (rec["itheta"].astype(np.int64) - (int(search.n_theta) - 1) // 2).astype(np.float64) * float(search.theta_step)
    out[:, 2] = a - 2.0 * math.pi * np.rint(a / (2.0 * math.pi))
    out[rec["itheta"] < 0] = np.nan
    return out


def localize(backend, xy, offsets, priors, grid, occ_spec, occ_min=100, cell_bits=16, grid_spec=None, search=None):
    """Scans localised in a finished occupancy grid through ANY backend with a match() method (the host route to
    HipBackend.localize, as submap_extra_scans is to submap tables): scan q of the packed scans (xy, offsets) is matched from
    priors[q] (x, y, heading) against the window of `grid` (int8 (H, W), window and res of occ_spec) around the prior's world
    cell.  The windows are made in numpy (map_windows), one per distinct origin, and appended to the bag as extra scans;
    backend.match(xy, offsets, pair_src, pair_tgt, theta0, cell_bits=) then sees ordinary pairs.  grid_spec / search: passed on
    to match() when given (a backend whose match() takes them), else the backend's own (BASELINE config #2) -- either way the
    spec match() returns must have the map's res.  Returns the dict of localize.localize: poses (n, 3) float64, records,
    origins int32 (n, 2), rejected (bool), points_per_window."""
    from . import csm
    off = np.asarray(offsets, dtype=np.int32)
    n = len(off) - 1
    P = np.asarray(priors, dtype=np.float64).reshape(-1, 3)
    if len(P) != n:
        raise ValueError("localize: %d priors for %d scans" % (len(P), n))
    gs = grid_spec if grid_spec is not None else csm.grid_spec(30.0, 0.05, 2.0, 1e-10, 40, cell_bits)
    if float(gs.res) != float(occ_spec.res):
        raise ValueError("localize: the tables' res %r is not the map's %r" % (float(gs.res), float(occ_spec.res)))
    mw = _MapwinFields(occ_spec, csm.grid_layout(gs).side, occ_min)
    origins, theta0 = map_window_origins(P, mw.res)
    uniq, slot = np.unique(origins, axis=0, return_inverse=True)
    slot = np.asarray(slot).reshape(-1)
    wxy, woff, _ = map_windows(grid, mw, uniq)
    xy2 = np.concatenate([np.asarray(xy, dtype=np.float32).reshape(-1, 2), wxy])
    off2 = np.concatenate([off, off[-1] + woff[1:]]).astype(np.int32)
    kw = {} if grid_spec is None and search is None else dict(grid_spec=grid_spec, search=search)
    rec, spec, srch = backend.match(xy2, off2, np.arange(n, dtype=np.int32), (n + slot).astype(np.int32), theta0,
                                    cell_bits=cell_bits, **kw)[:3]
    if float(spec.res) != mw.res or csm.grid_layout(spec).side != mw.side:
        raise ValueError("localize: the backend matched at res %r on tables of another side; the map's res is %r" % (float(spec.res), mw.res))
    return {"poses": localize_compose(rec, origins, theta0, spec, srch), "records": rec, "origins": origins,
            "rejected": np.asarray(rec["itheta"] < 0), "points_per_window": np.diff(woff)[slot].astype(np.int32)}


class _MapwinFields:
    """The fields of nhip_mapwin_spec_t from an occupancy spec (anything with res and the window), for the numpy statements."""

    def __init__(self, occ_spec, side, occ_min=100):
        self.res, self.cell_x0, self.cell_y0 = float(occ_spec.res), int(occ_spec.cell_x0), int(occ_spec.cell_y0)
        self.width, self.height, self.side, self.occ_min, self.flags, self.reserved = \
            int(occ_spec.width), int(occ_spec.height), int(side), int(occ_min), 0, 0


def rangesig_spec_check(spec):
    """The accepted ranges of nhip_rangesig_spec_t (include/nautilus_hip.h); ValueError otherwise."""
    for name in ("res", "unit"):
        v = float(getattr(spec, name))
        if not (math.isfinite(v) and v > 0):
            raise ValueError("range_signatures: %s must be finite and > 0" % name)
    for name, lo, hi in (("width", 1, 16384), ("height", 1, 16384), ("occ_min", 1, 127), ("free_max", 0, int(spec.occ_min) - 1),
                         ("stride", 1, 1024), ("max_ray_cells", 1, 4096), ("top_k", 1, 16), ("min_sep", 0, 64), ("min_sectors", 1, 64),
                         ("flags", 0, 1), ("reserved", 0, 0)):
        if not lo <= int(getattr(spec, name)) <= hi:
            raise ValueError("range_signatures: %s %d outside %d..%d" % (name, int(getattr(spec, name)), lo, hi))
    if int(spec.rays_per_sector) not in (1, 2, 4, 8):
        raise ValueError("range_signatures: rays_per_sector %d is not 1, 2, 4 or 8" % int(spec.rays_per_sector))


def range_signatures(grid, spec, rays=None):
    """The anchors of an occupancy grid and their range signatures in plain numpy ("Range signatures", items
    1 - 3; the device forms are nhip_rangesig_anchors_dev and nhip_rangesig_map_dev): (anchors int32 (A, 4) = {cx, cy, i, j},
    sig uint8 (A, 64), stats int64 (8,): words 0 - 5 of rangesig.STATS_FIELDS).  rays: the table, int32 (64 m, 4) (None: the
    library's, nhip_rangesig_tables: pure host).  All rays of all anchors walk together, a step at a time; a ray leaves the walk
    where it ends."""
    from . import rangesig
    rangesig_spec_check(spec)
    g = np.asarray(grid, dtype=np.int8).reshape(int(spec.height), int(spec.width))
    H, W = g.shape
    st, h, m = int(spec.stride), int(spec.stride) // 2, int(spec.rays_per_sector)
    nodes = g[h::st, h::st]
    jj, ii = np.nonzero((nodes >= 0) & (nodes <= int(spec.free_max)))  # (row-major: j ascending, then i)
    anchors = np.stack([ii * st + h, jj * st + h, ii, jj], axis=1).astype(np.int32).reshape(-1, 4)
    rays = (rangesig.tables(spec)[0] if rays is None else np.asarray(rays)).astype(np.int64).reshape(64 * m, 4)
    A, R = len(anchors), 64 * m
    val = np.full(A * R, 255, np.int64)
    end = np.full(A * R, 2, np.int8)
    live = np.arange(A * R)
    ax, ay = anchors[:, 0].astype(np.int64), anchors[:, 1].astype(np.int64)
    for k in range(1, int(rays[:, 2].max()) + 1 if A else 0):
        t = live % R
        live = live[rays[t, 2] >= k]  # (a ray that found nothing by its n: 255, already)
        if not len(live):
            break
        a, t = live // R, live % R
        n = rays[t, 2]
        x = ax[a] + (2 * k * rays[t, 0] + n) // (2 * n)
        y = ay[a] + (2 * k * rays[t, 1] + n) // (2 * n)
        inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        live, x, y, t = live[inside], x[inside], y[inside], t[inside]
        v = g[y, x].astype(np.int64)
        unknown, wall = v < 0, v >= int(spec.occ_min)
        end[live[unknown]] = 1
        end[live[wall]] = 0
        ranged = wall | unknown if int(spec.flags) & 1 else wall  # (NHIP_RANGESIG_UNKNOWN_STOPS: an unknown cell gives its range too)
        val[live[ranged]] = np.minimum(254, (k * rays[t[ranged], 3]) >> 16)
        live = live[~(unknown | wall)]
    sig = val.reshape(A, 64, m).min(axis=2).astype(np.uint8)
    stats = np.zeros(8, np.int64)
    stats[0], stats[1] = nodes.size, A
    stats[3:6] = np.bincount(end, minlength=3)[:3]
    return anchors, sig, stats


def scan_signatures(xy, offsets, spec):
    """The range signatures of the packed scans in plain numpy ("Range signatures", item 4; the device form is
    nhip_rangesig_scans_dev): uint8 (n_scans, 64).  The edges are the library's (nhip_rangesig_tables), the sectors the place
    descriptor's (nhip_place_tables): both pure host."""
    from . import place, rangesig
    rangesig_spec_check(spec)
    f = np.float32
    edge2, dirs = rangesig.tables(spec)[1], place.tables()[1]
    p = np.asarray(xy, dtype=f).reshape(-1, 2)
    off = np.asarray(offsets, dtype=np.int64)
    x, y = p[:, 0], p[:, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        r2 = ((x * x).astype(f) + (y * y).astype(f)).astype(f)
        kept = np.isfinite(r2)
        q = np.searchsorted(edge2[1:255], r2, side="right")  # (#{k in 1..254: r2 >= edge2[k]}: the edges ascend)
        neg = (y < 0) | ((y == 0) & (x < 0))
        u, v = np.where(neg, -x, x).astype(f), np.where(neg, -y, y).astype(f)
        sector = np.where(neg, 32, 0)
        for j in range(1, 32):
            sector = sector + (((dirs[j, 0] * v).astype(f) - (dirs[j, 1] * u).astype(f)).astype(f) >= 0)
    scan = np.repeat(np.arange(len(off) - 1), np.diff(off))
    sig = np.full((len(off) - 1, 64), 255, np.uint8)
    np.minimum.at(sig, (scan[kept], sector[kept]), q[kept].astype(np.uint8))
    return sig


def signature_candidates(query_sig, map_sig, anchors, spec):
    """The records of query signatures against map signatures in plain numpy ("Range signatures", items 5 and 6; the device form
    is nhip_rangesig_match_dev): (records int32 (Q, K, 4) = {anchor, shift, cost, valid}, four -1 where unfilled; stats int64
    (8,): words 6 and 7 of rangesig.STATS_FIELDS).  Any bytes are signatures; an anchor entry whose cell is outside the window is
    no anchor."""
    rangesig_spec_check(spec)
    Qs = np.asarray(query_sig, dtype=np.uint8).reshape(-1, 64)
    As = np.asarray(map_sig, dtype=np.uint8).reshape(-1, 64)
    an = np.asarray(anchors, dtype=np.int64).reshape(-1, 4)
    if len(an) != len(As):
        raise ValueError("signature_candidates: %d anchors for %d signatures" % (len(an), len(As)))
    K, sep = int(spec.top_k), int(spec.min_sep)
    rec, stats = np.full((len(Qs), K, 4), -1, np.int32), np.zeros(8, np.int64)
    ok = (an[:, 0] >= 0) & (an[:, 0] < int(spec.width)) & (an[:, 1] >= 0) & (an[:, 1] < int(spec.height))
    idx = np.nonzero(ok)[0]
    # A[(j + s) mod 64] for every anchor and shift: (64, A', 64) int16, 8 KB an anchor -- kept for all queries while the anchors
    # are one chunk, made again per query and chunk beyond that
    rolled = lambda rows: np.stack([np.roll(As[rows], -s, axis=1) for s in range(64)]).astype(np.int16)
    chunks = [idx[c:c + 8192] for c in range(0, len(idx), 8192)]
    kept = rolled(chunks[0]) if len(chunks) == 1 else None
    for q, Q in enumerate(Qs):
        mask = Q != 255
        valid = int(mask.sum())
        if valid >= int(spec.min_sectors) and len(idx):
            keys = []
            for rows in chunks:
                rot = kept if kept is not None else rolled(rows)
                cost = np.abs(rot[:, :, mask] - Q[mask].astype(np.int16)).sum(axis=2, dtype=np.int64)  # (64, rows)
                shift = cost.argmin(axis=0)  # (the first minimum: the smallest shift)
                keys.append(cost[shift, np.arange(len(rows))] * 64 + shift)
            key = np.concatenate(keys)
            order = np.lexsort((idx, key))
            taken = np.zeros(len(idx), bool)  # accepted, or suppressed by an accepted one
            for k in range(K):
                left = order[~taken[order]]
                if not len(left):
                    break
                b = left[0]
                rec[q, k] = (idx[b], key[b] % 64, key[b] // 64, valid)
                taken |= (np.abs(an[idx, 2] - an[idx[b], 2]) <= sep) & (np.abs(an[idx, 3] - an[idx[b], 3]) <= sep)
        n = int((rec[q, :, 0] >= 0).sum())
        stats[7] += n
        stats[6] += n == 0
    return rec, stats


def global_localize(backend, xy, offsets, grid, occ_spec, spec=None, grid_spec=None, search=None, cell_bits=16, occ_min=100):
    """Scans localised in a finished occupancy grid from NO prior, through ANY backend with a match() method (the host route to
    HipBackend.global_localize): the signatures, the records and their priors in numpy (range_signatures, scan_signatures,
    signature_candidates, rangesig.priors), then localize() above on the filled (scan, prior) entries, the scans repeated in
    the packed cloud; per query the entry with the highest record score wins, ties to the lower rank.  spec: a RangesigSpec
    (None: the defaults on occ_spec's window and res with NHIP_RANGESIG_UNKNOWN_STOPS, what a map ray-traced from scans needs).
    Returns {"poses": (Q, 3) float64, NaN where no entry matched;
    "rank": int32 (Q,), -1 likewise; "proposals": (Q, K, 3) float64; "candidates": int32 (Q, K, 4); "anchors": int32 (A, 4);
    "records": MATCH_DTYPE (Q, K), itheta -1 for an unfilled or rejected entry; "stats": int64 (8,)}."""
    from . import rangesig
    spec = rangesig.spec(occ_spec, occ_min=int(occ_min), flags=rangesig.NHIP_RANGESIG_UNKNOWN_STOPS) if spec is None else spec
    anchors, map_sig, stats = range_signatures(grid, spec)
    cand, s2 = signature_candidates(scan_signatures(xy, offsets, spec), map_sig, anchors, spec)
    stats[6:] = s2[6:]
    return global_localize_finish(lambda *a, **kw: localize(backend, *a, **kw), xy, offsets, cand, anchors, spec, stats, grid, occ_spec,
                                  dict(occ_min=occ_min, cell_bits=cell_bits, grid_spec=grid_spec, search=search))


def global_localize_finish(localize_fn, xy, offsets, cand, anchors, spec, stats, grid, occ_spec, kw):
    """The second half of global_localize, shared with relocalize.global_localize: the priors of the records, the (scan, prior)
    entries through localize_fn(xy, offsets, priors, grid, occ_spec, **kw), and the winner per query."""
    from . import csm, rangesig
    proposals = rangesig.priors(cand, anchors, spec)
    Q, K = cand.shape[:2]
    qq, kk = np.nonzero(cand[:, :, 0] >= 0)  # (query by query, rank by rank)
    p = np.asarray(xy, dtype=np.float32).reshape(-1, 2)
    off = np.asarray(offsets, dtype=np.int64)
    rec = np.zeros((Q, K), dtype=csm.MATCH_DTYPE)
    rec["itheta"] = -1
    rec["score"] = -np.inf
    poses_all = np.full((Q, K, 3), np.nan)
    if len(qq):
        xy2 = np.concatenate([p[off[q]:off[q + 1]] for q in qq]) if len(p) else p
        off2 = np.concatenate([[0], np.cumsum(np.diff(off)[qq])]).astype(np.int32)
        r = localize_fn(xy2, off2, proposals[qq, kk], grid, occ_spec, **kw)
        rec[qq, kk] = r["records"]
        poses_all[qq, kk] = r["poses"]
    score = np.where(rec["itheta"] >= 0, rec["score"].astype(np.float64), -np.inf)
    rank = score.argmax(axis=1).astype(np.int32) if K else np.zeros(Q, np.int32)  # (the first maximum: the lower rank)
    none = ~np.isfinite(score[np.arange(Q), rank]) if Q else np.zeros(0, bool)
    poses = poses_all[np.arange(Q), rank]
    poses[none] = np.nan
    rank[none] = -1
    return {"poses": poses, "rank": rank, "proposals": proposals, "candidates": cand, "anchors": anchors, "records": rec,
            "stats": stats}


def hitl_segments(msg):
    """LineSegmentsFromHitlMsg (solver.cc:467-478): msg = dict with line_a_start, line_a_end, line_b_start,
    line_b_end, each (x, y[, z]) -> two LineSegment<float> as (x0, y0, x1, y1) float32 rows."""
    row = lambda a, b: [msg[a][0], msg[a][1], msg[b][0], msg[b][1]]
    return np.array([row("line_a_start", "line_a_end"), row("line_b_start", "line_b_end")], dtype=np.float32)


# ---- match refinement ("Match refinement"; the device form is nhip_refine_icp_dev, K22) ----
REFINED_DTYPE = np.dtype([("c", "<f8"), ("s", "<f8"), ("tx", "<f8"), ("ty", "<f8"), ("info", "<f8", (6,)), ("cost", "<f8"),
                          ("n_corr", "<i4"), ("iterations", "<i4"), ("flags", "<u4"), ("pad", "<u4")])
REFINE_SKIPPED, REFINE_TARGET_TOO_LONG, REFINE_FEW, REFINE_SINGULAR, REFINE_RUNAWAY, REFINE_NOT_CONVERGED = 1, 2, 4, 8, 16, 32
REFINE_FLAG_NAMES = {1: "SKIPPED", 2: "TARGET_TOO_LONG", 4: "FEW", 8: "SINGULAR", 16: "RUNAWAY", 32: "NOT_CONVERGED"}
REFINE_THRESHOLDS, REFINE_TARGET_MAX = 16, 2048


def refine_thresholds(thr0, shrink, thr_min):
    """The spec's table: thr[k] = float32(max(thr_min, thr0 shrink^k)), the power by repeated products in double."""
    out, v = np.zeros(REFINE_THRESHOLDS, np.float32), float(thr0)
    for k in range(REFINE_THRESHOLDS):
        out[k] = np.float32(v if v > float(thr_min) else float(thr_min))
        v = v * float(shrink)
    return out


class RefineFields:
    """The fields of nhip_refine_spec_t with nhip_refine_spec_default's values, for callers without the library."""

    def __init__(self, **overrides):
        self.thr0, self.shrink, self.thr_min = 0.25, 0.5, 0.05
        self.step_tol_m = self.step_tol_rad = 1e-5
        self.min_spread, self.max_shift_m, self.max_turn_sin = 0.02, 0.5, math.sin(5.0 * math.pi / 180.0)
        self.max_iterations, self.min_corr, self.flags, self.reserved = 8, 30, 0, 0
        for k, v in overrides.items():
            if k != "thr" and not hasattr(self, k):
                raise TypeError("RefineFields: no field %r" % k)
            setattr(self, k, v)
        if "thr" not in overrides:
            self.thr = refine_thresholds(self.thr0, self.shrink, self.thr_min)


def refine_spec_check(spec):
    """The accepted ranges of nhip_refine_spec_t (include/nautilus_hip.h); ValueError otherwise."""
    thr = np.asarray(list(spec.thr), dtype=np.float32)
    n = int(spec.max_iterations)
    if not 1 <= n <= REFINE_THRESHOLDS:
        raise ValueError("refine: max_iterations %d outside 1..%d" % (n, REFINE_THRESHOLDS))
    if int(spec.min_corr) < 3 or int(spec.flags) != 0 or int(spec.reserved) != 0:
        raise ValueError("refine: min_corr below 3, or flags / reserved not 0")
    if not (0 < thr[0] < 1e6) or not np.all((thr[:n] > 0) & (thr[:n] <= thr[0])):
        raise ValueError("refine: thresholds outside (0, thr[0]]")
    for f in ("step_tol_m", "step_tol_rad", "min_spread", "max_shift_m", "max_turn_sin"):
        if not float(getattr(spec, f)) >= 0:
            raise ValueError("refine: %s negative or NaN" % f)


def refine_start_poses(records, theta0, grid_spec, search, pair_origin=None):
    """nhip_refine_start_poses in Python: (n, 4) float64 (cos, sin, tx, ty) of the records' lattice poses, theta formed in
    double and (cos, sin) from libm (math.cos / math.sin); four NaNs for a rejected record."""
    n = len(records)
    theta0 = np.asarray(theta0, dtype=np.float64).reshape(n)
    org = np.zeros((n, 2), np.int64) if pair_origin is None else np.asarray(pair_origin, dtype=np.int64).reshape(n, 2)
    out = np.full((n, 4), np.nan)
    ht, hx, hy = (int(search.n_theta) - 1) // 2, (int(search.nx) - 1) // 2, (int(search.ny) - 1) // 2
    step, res = float(search.theta_step), float(grid_spec.res)
    for i in range(n):
        it = int(records["itheta"][i])
        if it < 0:
            continue
        theta = float(theta0[i]) + float(it - ht) * step
        out[i] = (math.cos(theta), math.sin(theta), float(int(org[i, 0]) + int(records["ix"][i]) - hx) * res,
                  float(int(org[i, 1]) + int(records["iy"][i]) - hy) * res)
    return out


def _refine_evaluate(src, src_ok, tgt, tgt_ok, tgn, pose, thr):
    """One evaluation: the ten sums (H00 H01 H02 H11 H12 H22 g0 g1 g2 cost) and the count, in the rule's order."""
    f = np.float32
    c, s, tx, ty = pose
    cf, sf, txf, tyf = f(c), f(s), f(tx), f(ty)
    ns, nt = len(src), len(tgt)
    rounds = (ns + 255) // 256
    terms = np.zeros((rounds * 256, 10))
    kept = np.zeros(rounds * 256, bool)
    if ns and nt:
        with np.errstate(all="ignore"):
            px, py = src[:, 0], src[:, 1]
            qx = ((cf * px).astype(f) + ((-sf) * py).astype(f)).astype(f) + txf
            qy = ((sf * px).astype(f) + (cf * py).astype(f)).astype(f) + tyf
            dx, dy = tgt[None, :, 0] - qx[:, None], tgt[None, :, 1] - qy[:, None]
            d2 = dx * dx + dy * dy
            d2[:, ~tgt_ok] = np.inf
            d2[np.isnan(d2)] = np.inf
            idx = np.argmin(d2, axis=1)  # (the first minimum: ties to the lowest index)
            best = d2[np.arange(ns), idx]
            g, gn = tgt[idx], tgn[idx]
            keep = src_ok & (best < f(3.0e38)) & (np.sqrt(best) < f(thr)) & np.isfinite(gn).all(axis=1)
            nx, ny = gn[:, 0].astype(np.float64), gn[:, 1].astype(np.float64)
            dpx, dpy = px.astype(np.float64), py.astype(np.float64)
            ex, ey = qx.astype(np.float64) - g[:, 0].astype(np.float64), qy.astype(np.float64) - g[:, 1].astype(np.float64)
            r = nx * ex + ny * ey
            a, b = -(s * dpx) - c * dpy, c * dpx - s * dpy
            jt = nx * a + ny * b
            t = np.stack([nx * nx, nx * ny, nx * jt, ny * ny, ny * jt, jt * jt, nx * r, ny * r, jt * r, r * r], axis=1)
        terms[:ns] = np.where(keep[:, None], t, 0.0)  # (adding +0.0 leaves a lane's sum as it is, bit for bit)
        kept[:ns] = keep
    acc = np.zeros((256, 10))
    with np.errstate(all="ignore"):
        for k in range(rounds):  # point i belongs to lane i mod 256; a lane adds its points in ascending i
            acc = acc + terms[256 * k:256 * (k + 1)]
        while len(acc) > 1:  # adjacent-pair halving, eight levels
            acc = acc[0::2] + acc[1::2]
    return [float(v) for v in acc[0]], int(kept.sum())


def refine_icp(xy, normals, offsets, pair_src, pair_tgt, pose0, spec=None):
    """The match refinement in vectorised numpy on the host, equal to the device's bit for bit ("Match
    refinement"): (refined REFINED_DTYPE (n,), trace float64 (n, 16, 4)) from the start poses pose0 (n, 4) = (cos, sin, tx,
    ty).  Scan ids outside the scans raise ValueError."""
    f = np.float32
    spec = RefineFields() if spec is None else spec
    refine_spec_check(spec)
    xy, normals = np.asarray(xy, dtype=f).reshape(-1, 2), np.asarray(normals, dtype=f).reshape(-1, 2)
    off = np.asarray(offsets, dtype=np.int64)
    pair_src, pair_tgt = np.asarray(pair_src, dtype=np.int64).reshape(-1), np.asarray(pair_tgt, dtype=np.int64).reshape(-1)
    n = len(pair_src)
    pose0 = np.asarray(pose0, dtype=np.float64).reshape(n, 4)
    n_scans = len(off) - 1
    if n and (min(pair_src.min(), pair_tgt.min()) < 0 or max(pair_src.max(), pair_tgt.max()) >= n_scans):
        raise ValueError("refine_icp: a pair names a scan outside the %d scans" % n_scans)
    thr = np.asarray(list(spec.thr), dtype=f)
    max_it, min_corr = int(spec.max_iterations), int(spec.min_corr)
    tol_m, tol_rad = float(spec.step_tol_m), float(spec.step_tol_rad)
    min_spread, max_shift, max_turn = float(spec.min_spread), float(spec.max_shift_m), float(spec.max_turn_sin)
    out, trace = np.zeros(n, REFINED_DTYPE), np.zeros((n, REFINE_THRESHOLDS, 4))
    limit = f(1.0e6)
    with np.errstate(invalid="ignore"):
        ok_all = (np.abs(xy[:, 0]) < limit) & (np.abs(xy[:, 1]) < limit)
    for i in range(n):
        c0, s0, tx0, ty0 = (float(v) for v in pose0[i])
        rec = out[i]
        rec["c"], rec["s"], rec["tx"], rec["ty"] = c0, s0, tx0, ty0
        if not all(math.isfinite(v) for v in (c0, s0, tx0, ty0)):
            rec["c"] = rec["s"] = rec["tx"] = rec["ty"] = np.nan
            rec["flags"] = REFINE_SKIPPED
            continue
        sa, sb, ta, tb = off[pair_src[i]], off[pair_src[i] + 1], off[pair_tgt[i]], off[pair_tgt[i] + 1]
        if tb - ta > REFINE_TARGET_MAX:
            rec["flags"] = REFINE_TARGET_TOO_LONG
            continue
        data = (xy[sa:sb], ok_all[sa:sb], xy[ta:tb], ok_all[ta:tb], normals[ta:tb])
        c, s, tx, ty = c0, s0, tx0, ty0
        flags, it, converged = 0, 0, False
        while it < max_it:
            v, cnt = _refine_evaluate(*data, (c, s, tx, ty), thr[it])
            if cnt < min_corr:
                flags = REFINE_FEW
                break
            with np.errstate(all="ignore"):
                d = _refine_solve(v, cnt, min_spread)
            if d is None:
                flags = REFINE_SINGULAR
                break
            dx, dy, dth = d
            tx, ty = tx + dx, ty + dy
            hu = dth * 0.5
            u2 = hu * hu
            den = 1.0 + u2
            cd, sd = (1.0 - u2) / den, (2.0 * hu) / den
            c, s = c * cd - s * sd, s * cd + c * sd
            mx, my = tx - tx0, ty - ty0
            if not (math.sqrt(mx * mx + my * my) <= max_shift) or not (abs(s * c0 - c * s0) <= max_turn):
                flags = REFINE_RUNAWAY
                break
            trace[i, it] = (c, s, tx, ty)
            it += 1
            if math.sqrt(dx * dx + dy * dy) < tol_m and abs(dth) < tol_rad:
                converged = True
                break
        if flags == 0:
            flags = 0 if converged else REFINE_NOT_CONVERGED
            v, cnt = _refine_evaluate(*data, (c, s, tx, ty), thr[max_it - 1])
            if cnt < min_corr:
                flags = REFINE_FEW
            else:
                rec["c"], rec["s"], rec["tx"], rec["ty"] = c, s, tx, ty
                rec["info"], rec["cost"], rec["n_corr"] = v[:6], v[9], cnt
        rec["iterations"], rec["flags"] = it, flags
    return out, trace


def _refine_solve(v, cnt, min_spread):
    """H delta = -g by the square-root-free Cholesky of the rule, in Python floats (IEEE double): (dx, dy, dtheta), or None
    for SINGULAR."""
    H00, H01, H02, H11, H12, H22, g0, g1, g2 = (np.float64(x) for x in v[:9])  # (numpy scalars: a division by zero is inf / nan)
    hm, hd = (H00 + H11) * 0.5, (H00 - H11) * 0.5
    lam = hm - np.sqrt(hd * hd + H01 * H01)
    d0 = H00
    l10, l20 = H01 / d0, H02 / d0
    d1 = H11 - l10 * H01
    u = H12 - l20 * H01
    l21 = u / d1
    d2 = (H22 - l20 * H02) - l21 * u
    if not (lam / np.float64(cnt) >= min_spread) or not (d0 > 0.0) or not (d1 > 0.0) or not (d2 > 0.0):
        return None
    y0 = -g0
    y1 = -g1 - l10 * y0
    y2 = (-g2 - l20 * y0) - l21 * y1
    dth = y2 / d2
    dy = y1 / d1 - l21 * dth
    dx = (y0 / d0 - l10 * dy) - l20 * dth
    return float(dx), float(dy), float(dth)


def refine_matches(xy, normals, offsets, pair_src, pair_tgt, theta0, records, grid_spec, search, spec=None, pair_origin=None):
    """The match records refined on the host: refine_start_poses, then refine_icp; the refined array (REFINED_DTYPE).  What
    HipBackend.refine_matches returns, bit for bit; for a backend without that method (examples/slam_loop.py --lc-refine icp)."""
    pose0 = refine_start_poses(records, theta0, grid_spec, search, pair_origin)
    return refine_icp(xy, normals, offsets, pair_src, pair_tgt, pose0, spec)[0]


def refine_keeps_pose(refined):
    """Which refined records carry a refined pose: no flag, or NOT_CONVERGED alone (any other flag returned the start pose)."""
    return (np.asarray(refined)["flags"] & ~np.uint32(REFINE_NOT_CONVERGED)) == 0


def refine_flag_counts(refined):
    """{flag name: refined records that carry it}."""
    fl = np.asarray(refined)["flags"]
    return {name: int(((fl & bit) != 0).sum()) for bit, name in sorted(REFINE_FLAG_NAMES.items())}


def refined_to_transform(refined):
    """(n, 3) float64 (tx, ty, theta = atan2(s, c)) of refined records."""
    r = np.asarray(refined, dtype=REFINED_DTYPE).reshape(-1)
    theta = np.array([math.atan2(s, c) for s, c in zip(r["s"], r["c"])], dtype=np.float64)  # (libm's, as the C helper's)
    return np.stack([r["tx"], r["ty"], theta], axis=1)


# ---- relative-pose factors ("Relative-pose factors"; the device form is nhip_relpose.hip, K23) ----
RELPOSE_BAD_INFO, RELPOSE_BAD_MEASUREMENT, RELPOSE_SAME_POSE = 1, 2, 4


def relpose_information(refined, n=None, sigma_m=1.0, weights=(10.0, 10.0)):
    """nhip_relpose_information in Python, bit for bit: ((n, 6) float64 information L00 L01 L02 L11 L12 L22, (n,) bool mask of
    the records that took their H).  A record that carries a refined pose (refine_keeps_pose) gets H (1 / sigma_m^2) -- one
    rounded reciprocal of one rounded product, six products; any other, and every record when `refined` is None (then n
    counts them), gets diag(w_t w_t, w_t w_t, w_r w_r) of `weights`."""
    sigma_m, wt, wr = float(sigma_m), float(weights[0]), float(weights[1])
    if not (math.isfinite(sigma_m) and sigma_m > 0.0):
        raise ValueError("relpose_information: sigma_m %r must be finite and > 0" % (sigma_m,))
    if not (math.isfinite(wt) and math.isfinite(wr)):
        raise ValueError("relpose_information: weights %r must be finite" % (weights,))
    if refined is None:
        n = int(n or 0)
        took = np.zeros(n, dtype=bool)
        H = np.zeros((n, 6))
    else:
        refined = np.asarray(refined, dtype=REFINED_DTYPE).reshape(-1)
        took = refine_keeps_pose(refined)
        H = np.array(refined["info"], dtype=np.float64).reshape(-1, 6)
    inv = 1.0 / (sigma_m * sigma_m)
    diag = np.array([wt * wt, 0.0, 0.0, wt * wt, 0.0, wr * wr])
    with np.errstate(all="ignore"):
        info = np.where(took[:, None], H * inv, diag[None, :])
    return np.ascontiguousarray(info), took


def relpose_rows(z, info, pose_i, pose_j, poses, loss=None, trig=None):
    """The relative-pose factors in numpy, in the kernel's operation order ("Relative-pose factors"): z (F, 4)
    (z_x, z_y, c_z, s_z), info (F, 6), pose_i = the target's pose a, pose_j = the source's pose b, poses (n, 3); loss: None or a
    loss.Loss.  Returns (r (F, 3), J_i (F, 3, 3), J_j (F, 3, 3), rows (F, 28), weights (F, 4), flags (F,) int32): the whitened
    residual and its Jacobian halves without the loss; the rows and {s, rho, rho', sqrt(rho')} under it.  A flagged factor and one
    with a pose id outside [0, n) are zeros.  trig: None -- cos, sin and atan2 are libm's -- or the (F,) arrays
    (c_a, s_a, c_b, s_b, e_theta) of a device run (nhip_resid_relpose_dev's parts): everything else is recomputed from them."""
    z = np.asarray(z, dtype=np.float64).reshape(-1, 4)
    F = len(z)
    L = np.asarray(info, dtype=np.float64).reshape(F, 6)
    ia, ib = np.asarray(pose_i, dtype=np.int64).reshape(F), np.asarray(pose_j, dtype=np.int64).reshape(F)
    P = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    n = len(P)
    with np.errstate(all="ignore"):
        L00, L01, L02, L11, L12, L22 = (L[:, k] for k in range(6))
        D0 = L00
        l10, l20 = L01 / D0, L02 / D0
        D1 = L11 - l10 * L01
        u = L12 - l20 * L01
        l21 = u / D1
        D2 = (L22 - l20 * L02) - l21 * u
        flags = np.zeros(F, dtype=np.int32)
        flags[~(np.isfinite(L).all(axis=1) & (D0 > 0.0) & (D1 > 0.0) & (D2 > 0.0))] |= RELPOSE_BAD_INFO
        flags[~np.isfinite(z).all(axis=1)] |= RELPOSE_BAD_MEASUREMENT
        flags[ia == ib] |= RELPOSE_SAME_POSE
        in_range = (ia >= 0) & (ia < n) & (ib >= 0) & (ib < n)
        ok = in_range & (flags == 0)
        pa, pb = P[np.where(ok, ia, 0)] if n else np.zeros((F, 3)), P[np.where(ok, ib, 0)] if n else np.zeros((F, 3))
        if trig is None:
            ca = np.array([math.cos(t) if math.isfinite(t) else math.nan for t in pa[:, 2]], dtype=np.float64)
            sa = np.array([math.sin(t) if math.isfinite(t) else math.nan for t in pa[:, 2]], dtype=np.float64)
            cb = np.array([math.cos(t) if math.isfinite(t) else math.nan for t in pb[:, 2]], dtype=np.float64)
            sb = np.array([math.sin(t) if math.isfinite(t) else math.nan for t in pb[:, 2]], dtype=np.float64)
        else:
            ca, sa, cb, sb = (np.asarray(t, dtype=np.float64).reshape(F) for t in trig[:4])
        Dx, Dy = pb[:, 0] - pa[:, 0], pb[:, 1] - pa[:, 1]
        dx, dy = ca * Dx + sa * Dy, (-sa) * Dx + ca * Dy
        cr, sr = ca * cb + sa * sb, ca * sb - sa * cb
        ce, se = cr * z[:, 2] + sr * z[:, 3], sr * z[:, 2] - cr * z[:, 3]
        if trig is None:
            eth = np.array([math.atan2(s_, c_) for s_, c_ in zip(se, ce)], dtype=np.float64)
        else:
            eth = np.asarray(trig[4], dtype=np.float64).reshape(F)
        e = np.stack([dx - z[:, 0], dy - z[:, 1], eth], axis=1)
        zero, one = np.zeros(F), np.ones(F)
        E = np.stack([np.stack([-ca, -sa, dy, ca, sa, zero], axis=1), np.stack([sa, -ca, -dx, -sa, ca, zero], axis=1),
                      np.stack([zero, zero, -one, zero, zero, one], axis=1)], axis=1)  # (F, 3, 6)
        q0, q1, q2 = np.sqrt(D0), np.sqrt(D1), np.sqrt(D2)
        W00, W01, W02, W11, W12, W22 = q0, q0 * l10, q0 * l20, q1, q1 * l21, q2
        r = np.stack([W00 * e[:, 0] + W01 * e[:, 1] + W02 * e[:, 2], W11 * e[:, 1] + W12 * e[:, 2], W22 * e[:, 2]], axis=1)
        J = np.stack([W00[:, None] * E[:, 0] + W01[:, None] * E[:, 1] + W02[:, None] * E[:, 2],
                      W11[:, None] * E[:, 1] + W12[:, None] * E[:, 2], W22[:, None] * E[:, 2]], axis=1)  # (F, 3, 6)
        r[~ok], J[~ok] = 0.0, 0.0
        s = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2]
        if loss is None:
            rho, rho1 = s.copy(), np.ones(F)
        else:
            rho, rho1 = loss.pinned().evaluate(np.where(ok, s, 0.0))  # (cauchy: log1p in IEEE operations, as the kernel's)
        w = np.sqrt(rho1)
        rt, Jt = w[:, None] * r, w[:, None, None] * J
        rows = np.zeros((F, 28))
        k = 0
        for p in range(6):
            for q in range(p, 6):
                rows[:, k] = Jt[:, 0, p] * Jt[:, 0, q] + Jt[:, 1, p] * Jt[:, 1, q] + Jt[:, 2, p] * Jt[:, 2, q]
                k += 1
        for p in range(6):
            rows[:, 21 + p] = Jt[:, 0, p] * rt[:, 0] + Jt[:, 1, p] * rt[:, 1] + Jt[:, 2, p] * rt[:, 2]
        rows[:, 27] = rho
        weights = np.stack([s, rho, rho1, w], axis=1)
        rows[~ok], weights[~ok] = 0.0, 0.0
    return r, np.ascontiguousarray(J[:, :, :3]), np.ascontiguousarray(J[:, :, 3:]), rows, weights, flags
