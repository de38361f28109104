"""Definitions of every plane of a likelihood-table slot, in numpy, and the target scans the table build is tested on.

The definitions restate DESIGN.md section 3 and oracle/csm_oracle.c: hit raster -> exact integer separable blur ->
quantisation by the threshold table; the stored image with its zero border; the matcher's tiled copies; the hit raster;
the two max-pooled tables; the skip map.  expected_slot() derives all of them from the oracle's image (libm log in
double); tests/test_grid_targets_cpu.py proves hit_raster / blur_sums / quantise_by_table equal to that oracle.

The targets are built from CELL LISTS, so a test knows which cell every point is in: rim, seams, filled blocks, a
density ramp, points on cell edges and piles (targets()).  Plain module, imported by the tests that need it."""
import ctypes as C
import functools
import math

import numpy as np

from nautilus_amd import _lib, csm
from oracle import oracle as O

TILE = 64        # the build works in 64 x 64 tiles (nhip_grid.h)
HIT_PAD = 32     # zero border of the hit raster, in cells (include/nautilus_hip.h, hits_bytes)
LINE = 128       # bytes of one tile of the matcher's tiled planes


# ------------------------------------------------------------------------------------------------ definitions
def skip_map_definition(stored, width=21):
    """include/nautilus_hip.h (nhip_grid_layout_t.skip_bytes): bit (r, c) = any non-zero cell in stored rows
    [r, r + 21) x aligned dwords [c, c + 21 * cell_bytes), clipped to the image.  stored: (rows, pitch) bytes."""
    rows, pitch = stored.shape
    nz = stored.reshape(rows, pitch // 4, 4).any(axis=2)
    big = np.zeros((rows + 21, pitch // 4 + width), dtype=np.int64)
    big[:rows, :pitch // 4] = nz
    I = np.zeros((big.shape[0] + 1, big.shape[1] + 1), dtype=np.int64)
    I[1:, 1:] = big.cumsum(0).cumsum(1)
    r = np.arange(rows)[:, None]
    c = np.arange(pitch // 4)[None, :]
    cnt = I[r + 21, c + width] - I[r, c + width] - I[r + 21, c] + I[r, c]
    return (cnt > 0).astype(np.uint8)


def _pool_numpy(stored, cell_bits, stride=8):
    """pool[i][j] = max of stored[8i : 8i + 15, 8j : 8j + 15] (clipped; stride 4: [4i : 4i + 7, 4j : 4j + 7]);
    16-bit cells scaled by ceil(max / 257)."""
    rows = stored.shape[0]
    n = (rows + stride - 1) // stride
    win = 2 * stride - 1
    out = np.zeros((n, n), dtype=np.int64)
    for i in range(n):
        band = stored[stride * i:stride * i + win, :rows].max(axis=0).astype(np.int64)
        for j in range(n):
            out[i, j] = band[stride * j:stride * j + win].max()
    return out if cell_bits == 8 else (out + 256) // 257


def pool_definition(stored, cell_bits, stride=8):
    """_pool_numpy without its loops over entries (tests/test_grid_targets_cpu.py holds the two equal): the window
    maximum as 2 * stride - 1 shifted views of the image, zero beyond it (cells are >= 0, so clipping = zero padding)."""
    rows = stored.shape[0]
    n = (rows + stride - 1) // stride
    win = 2 * stride - 1
    big = np.zeros((stride * n + win, stride * n + win), dtype=np.int64)
    big[:rows, :rows] = stored[:, :rows]
    down = np.zeros((n, big.shape[1]), dtype=np.int64)
    for k in range(win):
        np.maximum(down, big[k:k + stride * n:stride], out=down)
    out = np.zeros((n, n), dtype=np.int64)
    for k in range(win):
        np.maximum(out, down[:, k:k + stride * n:stride], out=out)
    return out if cell_bits == 8 else (out + 256) // 257


def hit_raster(points, side, res):
    """(side, side) uint8 of 0 / 1, [row (y)][column (x)]: cell = side // 2 + floor(x / res) with the float promoted to
    double (cimg_debug.h:31-37); points with a non-finite coordinate or |v| >= 1e9 and cells outside the grid are
    dropped (cimg_debug.h:48-50; oracle/csm_oracle.c, orc_cell)."""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 2)
    cells = np.zeros((side, side), np.uint8)
    with np.errstate(invalid="ignore"):
        sane = np.all(np.isfinite(p) & (np.abs(p) < np.float32(1e9)), axis=1)
    p = p[sane].astype(np.float64)
    c = side // 2 + np.floor(p[:, 0] / res).astype(np.int64)
    r = side // 2 + np.floor(p[:, 1] / res).astype(np.int64)
    ok = (c >= 0) & (c < side) & (r >= 0) & (r < side)
    cells[r[ok], c[ok]] = 1
    return cells


def blur_sums(hits, taps):
    """The exact integer separable blur, int64: V[r][c] = sum_i sum_j taps[i] taps[j] H[r + i][c + j], terms outside the
    grid left out (oracle/csm_oracle.c:148-168)."""
    taps = np.asarray(taps, dtype=np.int64)
    R = (len(taps) - 1) // 2
    S = hits.shape[0]
    big = np.zeros((S, S + 2 * R), dtype=np.int64)
    big[:, R:R + S] = hits
    v1 = np.zeros((S + 2 * R, S), dtype=np.int64)
    for j in range(2 * R + 1):
        v1[R:R + S] += taps[j] * big[:, j:j + S]
    out = np.zeros((S, S), dtype=np.int64)
    for i in range(2 * R + 1):
        out += taps[i] * v1[i:i + S]
    return out


def quantise_by_table(sums, thr):
    """Cell value of a blur sum V: the number of levels k >= 1 with thr[k] <= V (thr[k] = smallest sum whose quantised
    value is >= k, 0xffffffff for a level no sum reaches)."""
    return np.searchsorted(np.asarray(thr, dtype=np.int64)[1:], np.asarray(sums, dtype=np.int64), side="right")


def grid_tables(spec):
    """(taps int32[2R + 1], thresholds uint32[256 or 65536]) of a spec: nhip_grid_tables, a host function."""
    L = csm.grid_layout(spec)
    taps = np.zeros(2 * L.blur_radius + 1, dtype=np.int32)
    thr = np.zeros(256 if L.cell_bytes == 1 else 65536, dtype=np.uint32)
    _lib.check(_lib.load().nhip_grid_tables(C.byref(spec), _lib.ptr(taps), _lib.ptr(thr)))
    return taps, thr


def first_guess(sums, thr):
    """Where the 16-bit quantiser of the build (grid_blur_kernel<2>, nhip_grid_blur.hip) starts its search of the table for
    a blur sum: the line through (ln thr[57344], 57344) and (ln thr[65535], 65535) that launch_grid_build (nhip_grid.hip)
    fits, evaluated in single precision.
    Within 6 levels of the answer a few table steps settle the cell; further off, a binary search of the whole table
    does.  Only to state which of the two an INPUT reaches (numpy's float32 log stands in for the device's)."""
    t1, t2 = float(thr[57344]), float(thr[65535])
    a = (65535.0 - 57344.0) / (math.log(t2) - math.log(t1))
    b = 57344.0 - a * math.log(t1)
    lg = np.log(np.asarray(sums).astype(np.float32)).astype(np.float32)
    gf = (np.float32(a) * lg).astype(np.float32) + np.float32(b)
    return np.clip(np.floor(gf.astype(np.float64)), 0, 65534).astype(np.int64)


def has_map(spec, layout):
    """The slot carries a built skip map: 8-bit grids with an image always, 16-bit ones when the spec asks."""
    return layout.grid_bytes > 0 and (layout.cell_bytes == 1 or bool(spec.flags & _lib.NHIP_GRID_SKIP_MAP))


def expected_slot(points, spec, ospec, layout):
    """Every plane a slot built from `points` must hold, by definition, from the oracle's image: a dict of
    image (rows, pitch / cell_bytes), hi (rows, hi_pitch), tiled16 (16-bit cells), hits (side, side), pool (level 1),
    pool4 (level 2, byte pairs {P4[i][j], P4[i + 1][j]}), skip (rows, bytes per map row).  All of them, whatever the
    spec stores: assert_slot leaves out what a spec does not have."""
    L = layout
    cb, bits = L.cell_bytes, 8 * L.cell_bytes
    S, pad, rows = L.side, L.pad, L.rows
    assert rows == S + 2 * pad
    inner = O.grid_build(points, ospec)
    assert inner.shape == (S, S) and inner.dtype == (np.uint8 if cb == 1 else np.uint16)
    image = np.zeros((rows, L.pitch // cb), dtype=inner.dtype)
    image[pad:pad + S, pad:pad + S] = inner
    hi = np.zeros((rows, L.hi_pitch), dtype=np.uint8)
    hi[:, :rows] = (image[:, :rows] >> 8).astype(np.uint8) if cb == 2 else image[:, :rows]
    out = {"image": image, "hi": hi, "hits": hit_raster(points, S, spec.res)}
    if cb == 2:
        out["tiled16"] = image
    p8 = pool_definition(image[:, :rows], bits, 8)
    pool = np.zeros((L.pool_rows, L.pool_pitch), dtype=np.uint8)
    pool[:p8.shape[0], :p8.shape[1]] = p8
    out["pool"] = pool
    p4 = pool_definition(image[:, :rows], bits, 4)
    n4 = p4.shape[0]
    pairs = np.zeros((L.pool4_rows, L.pool4_pitch), dtype=np.uint8)
    pairs[:n4, 0:2 * n4:2] = p4
    pairs[:n4 - 1, 1:2 * n4:2] = p4[1:]
    out["pool4"] = pairs
    mp = 8 * ((L.pitch // 4 + 63) // 64)
    bitmap = np.zeros((rows, 8 * mp), dtype=np.uint8)
    bitmap[:, :L.pitch // 4] = skip_map_definition(image.view(np.uint8).reshape(rows, L.pitch), width=21 * cb)
    out["skip"] = np.packbits(bitmap, axis=1, bitorder="little")
    return out


def _planes_of(spec, layout):
    """Names of the planes a slot of this spec holds."""
    names = ["hi0", "hi1", "hits", "pool", "pool4"]
    if layout.cell_bytes == 2:
        names.append("tiled16")
    if layout.grid_bytes > 0:
        names.append("image")
    if has_map(spec, layout):
        names.append("skip")
    return names


def _compare(got, expected, spec, layout, what):
    names = _planes_of(spec, layout)
    assert sorted(got) == sorted(names), (sorted(got), sorted(names))
    for name in names:
        want = expected["hi" if name in ("hi0", "hi1") else name]
        g = got[name]
        assert g.shape == want.shape and g.dtype == want.dtype, (what, name, g.shape, want.shape, g.dtype, want.dtype)
        if not np.array_equal(g, want):
            bad = np.argwhere(g != want)
            r, c = bad[0]
            raise AssertionError("%s: plane %s differs from its definition in %d places, first at (%d, %d): got %d, want %d"
                                 % (what, name, len(bad), r, c, g[r, c], want[r, c]))


def assert_slot(grids, slot, expected, what=""):
    """Every plane slot `slot` of a LikelihoodGrids handle holds, against expected_slot(): the stored image, both copies
    of the 8-bit plane, the tiled 16-bit copy, the hit raster, both pooled tables and the skip map, each by
    np.array_equal.  Left out only what the spec does not have: image and map under no_image, the map at 16 bits without
    skip_map=True, the tiled 16-bit copy at 8 bits."""
    L, spec = grids.layout, grids.spec
    got = {"hi0": grids.hi_plane(slot, copy=0), "hi1": grids.hi_plane(slot, copy=1), "hits": grids.hits(slot),
           "pool": grids.pooled(slot, 1), "pool4": grids.pooled(slot, 2)}
    if L.cell_bytes == 2:
        got["tiled16"] = grids.tiled16(slot)
    if L.grid_bytes > 0:
        got["image"] = grids.download(slot)
    if has_map(spec, L):
        got["skip"] = grids.skip_map(slot)
    _compare(got, expected, spec, L, "%s slot %d" % (what, slot))


def raw_slot_planes(raw, spec, layout):
    """The same planes out of the bytes of one slot as the device-pointer API leaves them (include/nautilus_hip.h,
    nhip_grid_layout_t: image | skip map | pooled table | second-level table | the matcher's tiled planes | hit raster;
    nhip_common.h, hi_tiled / t16_tiled: tiles of 8 rows x 16 bytes, the second copy shifted by 8 columns, then the 16-bit
    image in tiles of 8 rows x 8 cells)."""
    L = layout
    cb, rows = L.cell_bytes, L.rows
    raw = np.asarray(raw, dtype=np.uint8)
    assert raw.size == L.slot_bytes == L.grid_bytes + L.skip_bytes + L.pool_bytes + L.pool4_bytes + L.hi_bytes + L.hits_bytes
    o_skip = L.grid_bytes
    o_pool = o_skip + L.skip_bytes
    o_pool4 = o_pool + L.pool_bytes
    o_hi = o_pool4 + L.pool4_bytes
    o_hits = o_hi + L.hi_bytes
    got = {}
    if L.grid_bytes > 0:
        img = raw[:L.grid_bytes].reshape(rows, L.pitch)
        got["image"] = img.view(np.uint16) if cb == 2 else img
    if has_map(spec, L):
        mp = 8 * ((L.pitch // 4 + 63) // 64)
        got["skip"] = raw[o_skip:o_skip + rows * mp].reshape(rows, mp)
    got["pool"] = raw[o_pool:o_pool + L.pool_rows * L.pool_pitch].reshape(L.pool_rows, L.pool_pitch)
    got["pool4"] = raw[o_pool4:o_pool4 + L.pool4_rows * L.pool4_pitch].reshape(L.pool4_rows, L.pool4_pitch)
    tpr = L.hi_pitch // 16 + 1
    copy_bytes = ((rows + 7) // 8) * tpr * LINE
    r = np.arange(rows, dtype=np.int64)[:, None]
    c = np.arange(L.hi_pitch, dtype=np.int64)[None, :]
    for cp in (0, 1):
        cc = c + 8 * cp
        off = cp * copy_bytes + ((r >> 3) * tpr + (cc >> 4)) * LINE + (r & 7) * 16 + (cc & 15)
        got["hi%d" % cp] = raw[o_hi + off]
    if cb == 2:
        t16_tpr = L.hi_pitch // 8
        assert L.hi_bytes == 2 * copy_bytes + ((rows + 7) // 8) * t16_tpr * LINE
        c = np.arange(rows, dtype=np.int64)[None, :]
        off = o_hi + 2 * copy_bytes + ((r >> 3) * t16_tpr + (c >> 3)) * LINE + (r & 7) * 16 + (c & 7) * 2
        t16 = np.zeros((rows, L.pitch // 2), dtype=np.uint16)
        t16[:, :rows] = raw[off].astype(np.uint16) | (raw[off + 1].astype(np.uint16) << 8)
        got["tiled16"] = t16
    else:
        assert L.hi_bytes == 2 * copy_bytes
    hp = L.hits_pitch
    bit_rows = raw[o_hits:o_hits + hp * (L.side + 2 * HIT_PAD)].reshape(L.side + 2 * HIT_PAD, hp)
    bits = np.unpackbits(bit_rows, axis=1, bitorder="little")
    got["hits"] = bits[HIT_PAD:HIT_PAD + L.side, HIT_PAD:HIT_PAD + L.side]
    border = bits.copy()
    border[HIT_PAD:HIT_PAD + L.side, HIT_PAD:HIT_PAD + L.side] = 0
    assert not border.any() and not raw[o_hits + bit_rows.size:o_hits + L.hits_bytes].any(), "hit raster: border not zero"
    return got


def assert_raw_slot(raw, spec, layout, expected, what=""):
    """assert_slot on the bytes of a slot that a device-pointer build wrote."""
    _compare(raw_slot_planes(raw, spec, layout), expected, spec, layout, what)


# ------------------------------------------------------------------------------------------------ targets
def geometry_of(range_m, res, sigma):
    """(side, blur radius) of a geometry: cimg_debug.h:21-22 and ceil(3 sigma)."""
    return int(math.floor(2.0 * range_m / res)), int(math.ceil(3.0 * sigma))


def cells_of(points, side, res):
    """(column, row) of every point by the definition -- side // 2 + floor(double(v) / res) -- unclipped, int64."""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 2).astype(np.float64)
    return side // 2 + np.floor(p / res).astype(np.int64)


def cell_centres(cells, side, res):
    """float32 points in the middle of the cells (column, row), checked to lie in them."""
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 2)
    assert cells.min() >= 0 and cells.max() < side, "cell outside the grid"
    pts = ((cells - side // 2 + 0.5) * res).astype(np.float32)
    assert np.array_equal(cells_of(pts, side, res), cells), "a cell centre fell into another cell"
    return pts


def _rim(range_m, res, S, R):
    """Single hits along the grid's border, and points ON its rim.  Returns (points, facts about the rim points)."""
    cells = [(0, 0), (S - 1, 0), (0, S - 1), (S - 1, S - 1),                      # corners
             (S // 2, 0), (S // 2, S - 1), (0, S // 2), (S - 1, S // 2)]          # middle of each border row / column
    for i, d in enumerate((R - 1, R, R + 1)):                                      # distance d from each border
        along = S // 4 + i * (2 * R + 5)
        cells += [(d, along), (S - 1 - d, along + 2), (along + 1, d), (along + 3, S - 1 - d)]
    pts = [cell_centres(cells, S, res)]
    # the rim itself: -range, +range and the float below +range, on x and on y; where 2 range / res is no integer the
    # raster ends inside the range (the grid covers [-(S // 2) res, (S - S // 2) res)), so the ends of the raster too
    lo, hi = np.float32(-range_m), np.float32(range_m)
    glo, ghi = np.float32(-(S // 2) * res), np.float32((S - S // 2) * res)
    on_rim = [lo, hi, np.nextafter(hi, np.float32(0)), glo, np.nextafter(glo, np.float32(0)), np.nextafter(glo, -np.float32(np.inf)),
              ghi, np.nextafter(ghi, np.float32(0)), np.nextafter(ghi, np.float32(np.inf))]
    mid = [np.float32((k + 0.5) * res) for k in range(-len(on_rim), len(on_rim))]  # distinct cells along the other axis
    rim_pts = np.array([(v, mid[2 * i]) for i, v in enumerate(on_rim)] + [(mid[2 * i + 1], v) for i, v in enumerate(on_rim)],
                       dtype=np.float32)
    pts.append(rim_pts)
    k = cells_of(rim_pts, S, res)
    facts = {"minus_range_cell": (int(k[0, 0]), int(k[len(on_rim), 1])), "plus_range_cell": (int(k[1, 0]), int(k[len(on_rim) + 1, 1])),
             "below_plus_range_cell": (int(k[2, 0]), int(k[len(on_rim) + 2, 1]))}
    return np.concatenate(pts), facts


def _seam_cells(S, R):
    tiles = (S + TILE - 1) // TILE
    last0 = TILE * (tiles - 1)
    cells = [(63, 20), (64, 24), (20, 63), (24, 64), (63, 63), (63, 64), (64, 63), (64, 64)]
    cells += [(c, 64) for c in range(50, 141)] + [(63, r) for r in range(50, 141)]   # runs across the seams at 64 and 128
    cells += [(last0, S // 2 + 5), (S - 1, S // 2 + 9), (S // 2 + 5, last0), (S // 2 + 9, S - 1), (last0, last0), (S - 1, S - 1)]
    # R cells from the seam at 128 (inside the blur reach of the tile across it) and R + 1 (just outside), on both
    # sides and both axes
    for i, c in enumerate((128 + R - 1, 128 + R, 128 - R, 128 - R - 1)):
        cells += [(c, 8 + 3 * i), (S - 4 - 3 * i, c)]
    return sorted(set(cells))


def _block(lo, hi, S):
    a = np.arange(max(lo, 0), min(hi, S))
    return np.stack(np.meshgrid(a, a, indexing="xy"), axis=-1).reshape(-1, 2)


def _on_edges(S, res, rng, n=3000):
    """Both coordinates at float32(k res), k uniform over [-S // 2, S // 2]; a third left there, a third one float step
    down, a third one up (tests/test_bnb_cell_edges_gpu.py, _on_edges).  Then every k once more, left on its edge, on both
    axes: whether float32(k res) * (1 / res) and float32(k res) / res fall on different sides of an integer depends on k
    (at res 0.03: k = -250, -225, -125), and a draw may miss those.  Returns (points, k)."""
    every = np.arange(-(S // 2), S // 2 + 1)
    k = np.concatenate([rng.integers(-(S // 2), S // 2 + 1, size=(n, 2)), np.stack([every, rng.permutation(every)], axis=1)])
    snapped = (k * res).astype(np.float32)
    out = snapped.copy()
    i = np.arange(len(k))
    down, up = (i < n) & (i % 3 == 1), (i < n) & (i % 3 == 2)
    out[down] = np.nextafter(snapped[down], np.float32(-np.inf))
    out[up] = np.nextafter(snapped[up], np.float32(np.inf))
    return np.ascontiguousarray(out), k


@functools.lru_cache(maxsize=None)
def targets(range_m, res, sigma, seed=20):
    """The target scans of one geometry: (names, list of (n, 2) float32 clouds, facts).  Every generator places its
    points by cell and re-derives the cells from the float32 points by the definition; `facts` holds what the tests'
    preconditions need to know about the inputs (never anything a GPU computed)."""
    S, R = geometry_of(range_m, res, sigma)
    assert S >= 160 and R >= 1
    rng = np.random.default_rng(seed)
    facts = {"side": S, "R": R}
    scans = {}
    scans["rim"], facts["rim"] = _rim(range_m, res, S, R)
    scans["seams"] = cell_centres(_seam_cells(S, R), S, res)
    # every cell of a (2R + 3)^2 block around the corner four tiles share; every cell of tile (1, 1)'s whole neighbourhood
    scans["filled_corner"] = cell_centres(_block(64 - R - 1, 64 + R + 2, S), S, res)
    whole = _block(64 - R, 128 + R, S)
    scans["filled_tile"] = cell_centres(whole, S, res)
    facts["filled_tile_cells"] = len(np.unique(cells_of(scans["filled_tile"], S, res), axis=0))
    facts["filled_tile_inside"] = 64 - R >= 0 and 128 + R <= S
    # density ramp: 96 rows x width columns from cell (40, 40), cell (r, c) hit with probability (c / width)^2
    width = min(192, S - 40)
    hit = rng.random((96, width)) < (np.arange(width)[None, :] / width) ** 2
    rr, cc = np.nonzero(hit)
    scans["ramp"] = cell_centres(np.stack([40 + cc, 40 + rr], axis=1), S, res)
    scans["edges"], k = _on_edges(S, res, rng)
    got = cells_of(scans["edges"], S, res) - S // 2
    facts["edges_at_k"] = ((got == k).sum(axis=0) / len(k)).tolist()
    facts["edges_at_k_minus_1"] = ((got == k - 1).sum(axis=0) / len(k)).tolist()
    assert np.all((got == k) | (got == k - 1)), "a point one float step from k res lies in cell k or k - 1"
    # piles
    cell = np.array([[S // 2 + 7, S // 2 - 11]])
    scans["pile_same"] = np.repeat(cell_centres(cell, S, res), 5000, axis=0)
    lo = ((cell - S // 2) * res).astype(np.float64)
    many = (lo + rng.uniform(0.02, 0.98, (1000, 2)) * res).astype(np.float32)
    assert np.all(cells_of(many, S, res) == cell) and len(np.unique(many, axis=0)) == 1000
    scans["pile_floats"] = many
    scans["empty"] = np.zeros((0, 2), np.float32)
    scans["one_point"] = cell_centres([(S // 2 - 3, S // 2 + 2)], S, res)
    bad = np.array([[np.nan, 0.0], [0.0, np.nan], [np.inf, 1.0], [1.0, -np.inf], [1e12, 0.5], [0.5, -1e12], [np.nan, np.nan],
                    [2e9, 2e9]], dtype=np.float32)
    scans["not_finite"] = np.tile(bad, (5, 1))
    names = list(scans)
    clouds = [np.ascontiguousarray(scans[n_], dtype=np.float32) for n_ in names]
    for c_ in clouds:
        c_.setflags(write=False)
    return names, clouds, facts


# ------------------------------------------------------------------------------------------------ the test matrix
# (range, res, sigma, max_shift): A the production sigma on 7.5 tiles; B a side that is no multiple of 4 (666); C the
# largest blur radius (16: the build's tile neighbourhood at its LDS capacity); D end taps of 1 (blur sums from 1 up).
# max_shift sets the border: 48 cells at A and 32 at D (tiles start on the 16-byte boundaries of the tiled planes: the
# build writes line masks), 36 at B and 24 at C (they do not).
GEOMETRIES = {"A": (12.0, 0.05, 2.0, 16), "B": (10.0, 0.03, 1.0, 10), "C": (4.0, 0.05, 5.3, 3), "D": (12.0, 0.05, 0.7, 8)}
# ... and one floor just below 1 at 16 bits: the 65535 levels then span ln(1 / 0.999) = 0.001, the quantiser's
# single-precision first guess is up to ~150 levels off and the cells are settled by its binary search over the whole
# table -- which no floor of the list above reaches (there the guess is within one level: first_guess()).
COMBINATIONS = [(g, bits, 1e-10) for g in "ABCD" for bits in (8, 16)] + \
               [(g, bits, floor_p) for g in "DA" for bits in (8, 16) for floor_p in (1e-3, 1e-30)] + [("D", 16, 0.999)]


def combination_id(c):
    return "%s-%dbit-floor%g" % c


def specs(geometry, cell_bits, floor_p=1e-10, skip_map=None, no_image=False):
    """(spec, oracle spec, layout) of a geometry of the matrix; 16-bit specs carry a skip map unless told otherwise (so
    that the map is checked)."""
    range_m, res, sigma, max_shift = GEOMETRIES[geometry]
    if skip_map is None:
        skip_map = cell_bits == 16 and not no_image
    spec = csm.grid_spec(range_m, res, sigma, floor_p, max_shift, cell_bits, skip_map=skip_map, no_image=no_image)
    return spec, O.grid_spec(range_m, res, sigma, floor_p, cell_bits), csm.grid_layout(spec)


def geometry_targets(geometry):
    return targets(*GEOMETRIES[geometry][:3])


@functools.lru_cache(maxsize=None)
def expected_slots(geometry, cell_bits, floor_p=1e-10):
    """expected_slot() of every target of the geometry, computed once and shared (read-only) by the tests of a run."""
    spec, ospec, L = specs(geometry, cell_bits, floor_p)
    _, clouds, _ = geometry_targets(geometry)
    out = [expected_slot(c, spec, ospec, L) for c in clouds]
    for e in out:
        for a in e.values():
            a.setflags(write=False)
    return out
