"""The second list of the kernels that work candidates rotation by rotation (nhip_bnb_origin.h cache_origins): runs of
consecutive window origins inside one 4 x 4 level-2 entry, and the strip bounds taken over them (nhip_bnb_bounds.h
strip_bounds_c<RunList>) -- stated in numpy, with the hand-placed scans the tests run.  No GPU, no library.

A rotation's window origins are the spec's cells: rotate in single precision, every operation rounded on
its own, floor(double(v) / res), clamp, shift by the stored border.  The wave sweeps them in chunks of 64 points:

    cell list   a head is a live lane whose (row, col) differs from its predecessor's, or lane 0 of a chunk
    run list    ... whose (row >> 2, col >> 2) differs, or lane 0 of a chunk    (A, B, A stays three runs)

Entry i of either list sits in lane i % 64 of chunk i // 64.  The strip bounds add byte * points into 16-bit fields and sum
them over aligned groups of 8 lanes before unpacking, so a list is usable only while no group holds more than 257 points
over all chunks (257 * 255 = 65,535); the run list also has room for 512 entries only.  status() says what a rotation pass
does: "runs", or per cell because of the "field" check / the "capacity"."""
import math

import numpy as np

CHUNK, RUN_CAPACITY, GROUP_LIMIT = 64, 512, 257
RES, SIDE, PAD = 0.05, 1200, 96  # the 1,200-cell grid of the tests: csm.grid_spec(30.0, 0.05, 2.0, 1e-10, 40, bits)
POOL4_ROWS, POOL4_PITCH = 372, 768


def rotation(th0, k, n_theta, theta_step):
    """(cos, sin) of rotation k as the kernels compose it: R(theta0) R(delta_k) in double, rounded to float once."""
    c0, s0 = math.cos(th0), math.sin(th0)
    d = (k - (n_theta - 1) // 2) * theta_step
    cd, sd = math.cos(d), math.sin(d)
    return np.float32(c0 * cd - s0 * sd), np.float32(s0 * cd + c0 * sd)


def origins(pts, cf, sf, hx, hy, cx=0, cy=0):
    """Stored-grid (row, col) of the top-left lookup cell of every point."""
    x, y = pts[:, 0].astype(np.float32), pts[:, 1].astype(np.float32)
    xr = (cf * x).astype(np.float32) - (sf * y).astype(np.float32)
    yr = (sf * x).astype(np.float32) + (cf * y).astype(np.float32)
    fin = (np.abs(xr) < 1e9) & (np.abs(yr) < 1e9)
    ix = np.floor(np.where(fin, xr, 0).astype(np.float64) / RES).astype(np.int64)
    iy = np.floor(np.where(fin, yr, 0).astype(np.float64) / RES).astype(np.int64)
    col = np.where(fin, np.clip(SIDE // 2 + ix + cx, -hx - 1, SIDE + hx), -hx - 1)
    row = np.where(fin, np.clip(SIDE // 2 + iy + cy, -hy - 1, SIDE + hy), -hy - 1)
    return row - hy + PAD, col - hx + PAD


def _lists(key_r, key_c):
    """(index of each head, points of its run) of the list whose key is (key_r, key_c), cut at every chunk start."""
    n = len(key_r)
    head = np.ones(n, bool)
    head[1:] = (key_r[1:] != key_r[:-1]) | (key_c[1:] != key_c[:-1])
    head[::CHUNK] = True
    first = np.nonzero(head)[0]
    return first, np.diff(np.r_[first, n])


def cell_list(row, col):
    first, cnt = _lists(row, col)
    return row[first], col[first], cnt


def run_list(row, col):
    """(row >> 2, col >> 2, points) per run."""
    first, cnt = _lists(row >> 2, col >> 2)
    return row[first] >> 2, col[first] >> 2, cnt


def group_totals(cnt):
    """Points per aligned group of 8 lanes over all chunks of a list: 8 totals."""
    lanes = np.zeros(CHUNK, np.int64)
    np.add.at(lanes, np.arange(len(cnt)) % CHUNK, cnt)
    return lanes.reshape(8, 8).sum(axis=1)


def status(row, col):
    """What cache_origins reports of a rotation: the order of its checks."""
    if group_totals(cell_list(row, col)[2]).max() > GROUP_LIMIT:
        return "field"  # (the cell list is rebuilt unmerged: no run list)
    cnt = run_list(row, col)[2]
    if len(cnt) > RUN_CAPACITY:
        return "capacity"
    return "field" if group_totals(cnt).max() > GROUP_LIMIT else "runs"


def strip_bound(table, r2, c2, cnt, Y, X0, length, scale=1):
    """The twelve sub-block bounds of blocks (Y, X0 .. X0 + length - 1) from a list of level-2 entries (r2, c2) with `cnt`
    points each: out[4 t + q], q = 2 sy + sx.  The table holds the byte pair {P4[i][j], P4[i + 1][j]} at (i, 2 j)."""
    flat = table.reshape(-1).astype(np.int64)
    a = r2 * POOL4_PITCH + 2 * c2 + 2 * Y * POOL4_PITCH + 4 * X0
    assert a.min() >= 0 and a.max() + 16 <= flat.size, "a strip load outside the table"
    out = np.zeros(12, np.int64)
    for t in range(length):
        b = [flat[a + 4 * t + j] for j in range(4)]  # (sy 0, sx 0), (sy 1, sx 0), (sy 0, sx 1), (sy 1, sx 1)
        for q, j in ((0, 0), (2, 1), (1, 2), (3, 3)):
            out[4 * t + q] = int((b[j] * cnt).sum()) * scale
    return out


def strip_bound_packed(table, r2, c2, cnt, Y, X0, length, scale=1):
    """The same through the kernel's arithmetic: per lane 16-bit fields of byte * points, summed over the aligned group of 8
    lanes MODULO 2^16 per field (a carry out of a field is lost, or lands in its neighbour), then over the groups."""
    flat = table.reshape(-1).astype(np.int64)
    a = r2 * POOL4_PITCH + 2 * c2 + 2 * Y * POOL4_PITCH + 4 * X0
    lane = np.arange(len(cnt)) % CHUNK
    out = np.zeros(12, np.int64)
    for t in range(length):
        for q, j in ((0, 0), (2, 1), (1, 2), (3, 3)):
            per_lane = np.zeros(CHUNK, np.int64)
            np.add.at(per_lane, lane, flat[a + 4 * t + j] * cnt)
            out[4 * t + q] = int((per_lane.reshape(8, 8).sum(axis=1) & 0xffff).sum()) * scale
    return out


# ---- the hand-placed scans ---------------------------------------------------------------------------------------------
def points_of_cells(iy, ix):
    """A point in the middle of each cell (iy, ix), cells counted from the grid's centre: under the identity its origin is
    row = iy + 600 - hy + 96, col = ix + 600 - hx + 96, and 600 + 96 - h is a multiple of 4 for the lattices used here
    (h = 4, 8), so ix & 3 is the column inside the level-2 entry."""
    return np.stack([(np.asarray(ix) + 0.5) * RES, (np.asarray(iy) + 0.5) * RES], axis=1).astype(np.float32)


def cells_of_scan(scan):
    return np.floor(scan[:, 1].astype(np.float64) / RES).astype(np.int64), np.floor(scan[:, 0].astype(np.float64) / RES).astype(np.int64)


def _distinct_entries(by, bx, k):
    """k cells of a scan that lie in k different level-2 entries with alternating parity of col >> 2, in beam order."""
    out, seen, want = [], set(), 0
    for y, x in zip(by, bx):
        e = (y >> 2, x >> 2)
        if e in seen or ((x >> 2) & 1) != want:
            continue
        seen.add(e)
        out.append((int(y), int(x)))
        want ^= 1
        if len(out) == k:
            return out
    raise AssertionError("the scan has too few level-2 entries")


def cases(scan):
    """name -> (points, what every rotation pass of the pair must do, runs of the centre rotation or None), built from the
    cells of one real scan so that the points lie on walls the neighbouring target scan also sees."""
    by, bx = cells_of_scan(scan)
    (ya, xa), (yb, xb), (yc, xc) = _distinct_entries(by, bx, 3)
    assert ((xa >> 2) & 1, (xb >> 2) & 1) == (0, 1)  # both values of the (a & 2) alignment of the strip load
    alt = lambda n: (np.where(np.arange(n) & 1, yb, ya), np.where(np.arange(n) & 1, xb, xa))
    x0 = xc & ~3  # the first column of entry C
    out = {}
    for n in (1, 63, 64, 65, 1081, 1088):
        out["len%d" % n] = (points_of_cells(np.resize(by, n), np.resize(bx, n)), "runs", None)
    # ten points in one cell from point 60 on: the run is cut at point 64
    iy, ix = by[:100].copy(), bx[:100].copy()
    iy[60:70], ix[60:70] = ya, xa
    out["straddle"] = (points_of_cells(iy, ix), "runs", None)
    # beams alternating between two entries: A, B, A are three runs; 64 | 65 runs are one | two chunks, 512 fill the list
    for n in (64, 65, 512):
        out["alt%d" % n] = (points_of_cells(*alt(n)), "runs", n)
    out["alt513"] = (points_of_cells(*alt(513)), "capacity", 513)
    # all 1081 points in one 20 cm patch, walking its 16 cells: 17 runs of 64 (the last: 57), lanes 0..7 hold 512 points
    w = np.arange(1081) % 16
    out["patch"] = (points_of_cells(yc & ~3 | (w >> 2), x0 | (w & 3)), "field", 17)
    # lanes 0..7 of the run list hold exactly 257 | 258 points: runs of 64, 64, 64, 61 | 62 points that alternate between two
    # cells of entry C (the cell list's entries hold one point each: only the run list's own check can object), then singles
    for big, name, what in ((61, "group257", "runs"), (62, "group258", "field")):
        n = 192 + big
        sy, sx = alt(40)
        iy = np.r_[np.full(n, yc), sy]
        ix = np.r_[x0 + (np.arange(n) & 1), sx]
        out[name] = (points_of_cells(iy, ix), what, 4 + 40)
    # columns 0 | 1 of one entry alternate: different cells, one run (which the first point in column 3 still joins: 41
    # points); then columns 3 | 4 alternate, cells 3 | 4 lie on either side of an entry's edge: 39 runs of one point
    k = np.arange(40) & 1
    iy = np.full(80, yc)
    ix = np.r_[x0 + k, x0 + 3 + k]
    out["boundary"] = (points_of_cells(iy, ix), "runs", 1 + 39)
    return out
