"""The per-cell statement of the map windows ("Map windows"; the device form is K20,
nautilus_amd/csrc/nhip_mapwin.hip), and the crafted inputs its tests share.  Written from the spec's text and differently from
the kernels and from hostside.map_windows on purpose: the occupied cells are listed by two nested loops over the map, a window
is a membership test of EVERY occupied cell of the map against the query's bounds in python integers -- no row pointers are
used to find a window, no bisection, no searchsorted, no code shared with the product.

A spec is anything with the fields of nhip_mapwin_spec_t as attributes (a ctypes struct, or make_spec() below).
"""
import functools
from types import SimpleNamespace

import numpy as np

FIELDS = ("res", "cell_x0", "cell_y0", "width", "height", "side", "occ_min", "flags", "reserved")
VALUES = (-128, -1, 0, 99, 100, 127)  # around occ_min = 100 and occ_min = 1; -1 is "unknown" and never occupied
INT32_MAX = 2 ** 31 - 1


def make_spec(**kw):
    s = SimpleNamespace(res=0.05, cell_x0=0, cell_y0=0, width=1, height=1, side=2, occ_min=100, flags=0, reserved=0)
    for k, v in kw.items():
        assert k in FIELDS, k
        setattr(s, k, v)
    return s


def occupied_cells(grid, spec):
    """[(y, x)] of the occupied cells, rows in order, x ascending inside a row."""
    g = np.asarray(grid, dtype=np.int8).reshape(spec.height, spec.width).tolist()
    out = []
    for y in range(spec.height):
        row = g[y]
        for x in range(spec.width):
            if row[x] >= spec.occ_min:
                out.append((y, x))
    return out


def map_cells(grid, spec, max_cells=None):
    """(row_ptr int32 (height + 1,), cols int32, n_occ): item 1.  More cells than max_cells: nothing packed, zeros throughout."""
    cells = occupied_cells(grid, spec)
    if max_cells is not None and len(cells) > max_cells:
        return np.zeros(spec.height + 1, np.int32), np.zeros(0, np.int32), len(cells)
    row_ptr = np.zeros(spec.height + 1, np.int32)
    for y, _ in cells:
        row_ptr[y + 1] += 1
    return np.cumsum(row_ptr).astype(np.int32), np.array([x for _, x in cells], dtype=np.int32).reshape(-1), len(cells)


def map_windows(grid, spec, origins, max_cells=None, capacity=None):
    """(xy float32 (n, 2), offsets int32 (n_queries + 1,), stats int64 (8,)): items 3 to 5."""
    cells = occupied_cells(grid, spec)
    n_occ = len(cells)
    cells_fit = max_cells is None or n_occ <= max_cells
    if not cells_fit:
        cells = []
    wy = np.array([y for y, _ in cells], dtype=np.int64) + int(spec.cell_y0)  # world cells
    wx = np.array([x for _, x in cells], dtype=np.int64) + int(spec.cell_x0)
    side = int(spec.side)
    k_lo, k_hi = -(side // 2), side - side // 2 - 1
    parts, counts = [], []
    for ox, oy in np.asarray(origins, dtype=np.int64).reshape(-1, 2).tolist():
        kx, ky = wx - ox, wy - oy
        inside = (kx >= k_lo) & (kx <= k_hi) & (ky >= k_lo) & (ky <= k_hi)
        x = ((kx[inside].astype(np.float64) + 0.5) * float(spec.res)).astype(np.float32)
        y = ((ky[inside].astype(np.float64) + 0.5) * float(spec.res)).astype(np.float32)
        parts.append(np.stack([x, y], axis=1))  # (the cells are in row order already)
        counts.append(int(inside.sum()))
    total = sum(counts)
    points_fit = total <= INT32_MAX and (capacity is None or total <= capacity)
    stats = np.array([n_occ, len(counts), total if points_fit else 0, sum(c == 0 for c in counts), max(counts) if counts else 0,
                      0 if cells_fit else 1, 0 if points_fit else 1, 0], dtype=np.int64)
    if not points_fit:
        return np.zeros((0, 2), np.float32), np.zeros(len(counts) + 1, np.int32), stats
    xy = np.concatenate(parts).astype(np.float32) if parts else np.zeros((0, 2), np.float32)
    return xy.reshape(-1, 2), np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), stats


def same(got, want, name):
    """(xy, offsets, stats) bit for bit"""
    for k, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (name, k, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (name, k, np.nonzero(g.reshape(-1) != w.reshape(-1))[0][:8])


def same_cells(got, want, name):
    """(row_ptr, cols) bit for bit"""
    same(got[:2], want[:2], name)


# ---------------------------------------------------------------- the crafted inputs
WIDTHS = (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 130, 1025)  # every load width and tail of the row kernels
HEIGHTS = (1, 130)
SIDES = (2, 3, 8, 41, 300)                                 # even and odd, smaller and larger than the maps


def window_origins(spec):
    """Origins whose windows lie inside the map, hang over each edge and corner, touch one rim column or row only, miss the map
    by one cell and by far -- the product of eight positions per axis -- plus origins at the ends of the admitted range and of
    int32."""
    side, half = spec.side, spec.side // 2

    def axis(c0, n):
        last = c0 + n - 1
        return [c0 - side - 3, c0 - (side - half - 1) - 1, c0 - (side - half - 1), c0, c0 + n // 2, last, last + half, last + half + 1]
    xs, ys = axis(spec.cell_x0, spec.width), axis(spec.cell_y0, spec.height)
    out = [(x, y) for y in ys for x in xs]
    cx, cy = spec.cell_x0 + spec.width // 2, spec.cell_y0 + spec.height // 2
    out += [(2 ** 30 - 1, cy), (-2 ** 30, cy), (cx, 2 ** 30 - 1), (cx, -2 ** 30), (2 ** 31 - 1, -2 ** 31), (-2 ** 31, 2 ** 31 - 1),
            (2 ** 31 - 1, cy), (cx, -2 ** 31)]
    return np.array(out, dtype=np.int32)


def value_map(width, height, seed):
    rng = np.random.default_rng(seed)
    return rng.choice(np.array(VALUES, dtype=np.int8), size=(height, width), p=[0.1, 0.3, 0.3, 0.1, 0.1, 0.1])


def counted_rows_map():
    """1025 x 12: rows with exactly 63, 64, 65 and 200 occupied cells (a compaction that ends inside a wave, on its edge, one
    past it, and that loops), spread, packed at the start and packed at the end of the row; the rest empty or sparse."""
    g = np.full((12, 1025), -1, np.int8)
    rng = np.random.default_rng(5)
    for y, n in enumerate((63, 64, 65, 200)):
        g[y, np.sort(rng.choice(1025, n, replace=False))] = 100
        g[4 + y, :n] = 100
    g[8, 1025 - 65:] = 127
    g[9, 1025 - 200:] = 100
    g[11, ::64] = 100
    return g


def rim_map(width=65, height=33):
    g = np.zeros((height, width), np.int8)
    g[0, :] = g[-1, :] = 100
    g[:, 0] = g[:, -1] = 100
    return g


def corners_map(width=130, height=130):
    g = np.full((height, width), -1, np.int8)
    g[0, 0] = g[0, -1] = g[-1, 0] = g[-1, -1] = 100
    return g


@functools.lru_cache(maxsize=None)
def shared_cases():
    """[(name, grid int8 (H, W), spec, origins int32 (n, 2))]"""
    out = []
    k = 0
    for h in HEIGHTS:
        for w in WIDTHS:
            for occ_min in (100, 1):
                side = SIDES[k % len(SIDES)]
                spec = make_spec(res=(0.05, 0.01, 0.3)[k % 3], cell_x0=(-7, 0, 1000, -2000)[k % 4], cell_y0=(3, -130, 0)[k % 3],
                                 width=w, height=h, side=side, occ_min=occ_min)
                out.append(("values %dx%d occ_min %d side %d" % (w, h, occ_min, side), value_map(w, h, 100 + k), spec, window_origins(spec)))
                k += 1
    for side in (2, 41, 300):
        spec = make_spec(cell_x0=-30, cell_y0=-60, width=65, height=130, side=side)
        out.append(("empty side %d" % side, np.full((130, 65), -1, np.int8), spec, window_origins(spec)))
        out.append(("full side %d" % side, np.full((130, 65), 100, np.int8), spec, window_origins(spec)))
    for side in (3, 300, 2048):
        spec = make_spec(cell_x0=-500, cell_y0=7, width=1025, height=12, side=side)
        out.append(("counted rows side %d" % side, counted_rows_map(), spec, window_origins(spec)))
    for side in (8, 41):
        spec = make_spec(cell_x0=5, cell_y0=-16, width=65, height=33, side=side, res=0.3)
        out.append(("rim side %d" % side, rim_map(), spec, window_origins(spec)))
        spec = make_spec(cell_x0=-65, cell_y0=-65, width=130, height=130, side=side, res=0.01)
        out.append(("corners side %d" % side, corners_map(), spec, window_origins(spec)))
    return out


@functools.lru_cache(maxsize=None)
def shared_results():
    """{name: ((row_ptr, cols, n_occ), (xy, offsets, stats))} of shared_cases(), computed once"""
    return {name: (map_cells(grid, spec), map_windows(grid, spec, org)) for name, grid, spec, org in shared_cases()}


def many_queries_case(n=2500, seed=9):
    """a 17 x 130 map and n origins drawn with duplicates from a few hundred places in and around it"""
    spec = make_spec(cell_x0=-8, cell_y0=-65, width=17, height=130, side=41)
    grid = value_map(17, 130, 77)
    rng = np.random.default_rng(seed)
    places = np.stack([rng.integers(-40, 40, 300), rng.integers(-120, 120, 300)], axis=1)
    return "many queries", grid, spec, places[rng.integers(0, 300, n)].astype(np.int32)
