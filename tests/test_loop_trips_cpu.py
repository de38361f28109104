"""tests/loop_trips.py holds what it is for (no GPU): every case crosses the seam it is named after -- which scans sit past it,
non-zero carries, the chunk sizes -- and the hostside numpy forms agree with the references on these inputs.  The sector rule
on its boundaries is held to the references' text and, away from the boundaries, to a longdouble atan2."""
import numpy as np
import pytest

from nautilus_amd import hostside, localize, place, rangesig
from tests import localize_reference as LR
from tests import loop_trips as T
from tests import place_reference as PR
from tests import rangesig_reference as RR


def product(spec_fn, ref_spec, fields):
    s = spec_fn()
    for f in fields:
        setattr(s, f, getattr(ref_spec, f))
    return s


# ---------------------------------------------------------------- K8
@pytest.mark.parametrize("name,n", T.HITL_CASES)
def test_hitl_tables_put_the_nodes_where_the_carries_need_them(name, n):
    table = T.hitl_table(name, n)
    cls, cnt, blk, so, tot = T.hitl_expected(table)
    lengths = np.diff(table.offsets)
    assert len(table.scans) == n and lengths.min() == 0 and 3 <= lengths.max() <= 12
    want = np.array([T.hitl_membership(name, k) for k in range(n)])
    is_a, is_b = cnt[0::2] >= 3, (cnt[0::2] < 3) & (cnt[1::2] >= 3)
    assert np.array_equal(is_a, want == "a") and np.array_equal(is_b, want == "b")  # (hostside sees the plan)
    assert tot.tolist() == [is_a.sum(), is_b.sum(), cnt[0::2][is_a].sum() + cnt[1::2][is_b].sum()]
    assert (blk[~(is_a | is_b)] == -1).all() and sorted(blk[is_a | is_b].tolist()) == list(range(tot[0] + tot[1]))
    assert (cnt[1::2][is_a] > 0).any()  # (b-points of an a-node: not packed)
    first = slice(0, 1024)
    if name == "b then a" and n > 1024:
        # no a-node in the first step: n_a and pts_a come from the later ones, and b-nodes of BOTH steps must get them
        assert not is_a[first].any() and is_b[first].sum() > 300 and is_a[1024:].any() and (n < 1030 or is_b[1024:].any())
        assert blk[is_b][0] == tot[0] and so[np.nonzero(is_b)[0][0]] == cnt[0::2][is_a].sum() > 0
    if name == "a then b" and n > 1024:
        assert not is_b[first].any() and is_a[first].sum() > 300 and is_b[1024:].any() and (n < 1030 or is_a[1024:].any())
        k = int(np.nonzero(is_b[1024:])[0][0]) + 1024  # the first b-node: behind every a-node, those of later steps included
        assert blk[k] == tot[0] and so[k] == cnt[0::2][is_a].sum()
    if name == "mix":
        for lo in range(0, n, 1024):  # a, b and neither in every step, on both sides of each seam
            part = want[lo:lo + 1024]
            assert {"a", "b", "-"} <= set(part.tolist()) or len(part) < 9
        if n > 1024:
            assert {"a", "b", "-"} <= set(want[1020:1024].tolist() + want[1024:1029].tolist())
            assert is_a[:1024].any() and is_b[:1024].any()  # all four carries are non-zero at the seam
        if n > 2048:
            assert {"a", "b"} & set(want[2048:].tolist())


# ---------------------------------------------------------------- K16, K21: scans beyond 4096
def test_many_scans_differ_between_a_workgroups_trips():
    xy, off = T.many_scans()
    n = len(off) - 1
    assert n == 4200 == max(T.N_MANY_SCANS) and np.diff(off).max() == 3 and np.diff(off).min() == 0
    D, bits = T.many_scans_descriptors()
    sig = T.many_scans_signatures()
    h_D, h_bits = hostside.place_descriptors(xy, off, place.default_spec())
    assert np.array_equal(h_D, D) and np.array_equal(h_bits, bits)
    assert np.array_equal(hostside.scan_signatures(xy, off, product(rangesig.default_spec, RR.make_spec(), RR.FIELDS)), sig)
    later = np.arange(4096, n)
    assert (bits[later] != bits[later - 4096]).all()  # (the numbers of points differ)
    for s in later:
        assert not np.array_equal(D[s], D[s - 4096]) and not np.array_equal(sig[s], sig[s - 4096])
        stale_d, stale_s = D[s] & D[s - 4096], (sig[s] != 255) & (sig[s - 4096] != 255)
        assert not stale_d.any() and not stale_s.any()  # no bin in common: a stale word of the first trip cannot hide
    assert (bits[later] == 0).sum() > 20 and (bits[later - 4096] == 0).sum() > 20 and bits[4096] > 0 and bits[0] == 0


# ---------------------------------------------------------------- K20
@pytest.mark.parametrize("width,height", T.TALL_MAPS)
def test_tall_maps_have_cells_on_both_sides_of_the_row_steps(width, height):
    grid, spec, origins = T.tall_map(width, height)
    row_ptr, cols, n_occ = LR.map_cells(grid, spec)
    h_row_ptr, h_cols = hostside.map_cells(grid, product(localize.default_spec, spec, LR.FIELDS))
    assert np.array_equal(h_row_ptr, row_ptr) and np.array_equal(h_cols, cols)
    per_row = np.diff(row_ptr)
    assert per_row.max() == 5 and per_row.min() == 0 and set(range(6)) == set(per_row.tolist())
    for seam in range(1024, height, 1024):
        if seam == 2048:
            assert not per_row[2044:min(2053, height)].any() and per_row[2043] + per_row[min(2053, height - 1)] > 0 or height == 2049
        else:
            assert per_row[seam - 1] > 0 and per_row[seam] > 0
    if height > 1024:
        assert 0 < row_ptr[1024] <= n_occ - 1  # one cell short of n_occ is passed only in a later step than the first
    for side in (8, 41):
        sp = T.with_side(spec, side)
        xy, off, stats = LR.map_windows(grid, sp, origins)
        h = hostside.map_windows(grid, product(localize.default_spec, sp, LR.FIELDS), origins)
        LR.same(h, (xy, off, stats), "hostside")
        if height > 1030:
            q = [i for i, (ox, oy) in enumerate(origins.tolist()) if oy + 1000 in (1023, 1024)]
            rows = [set(np.floor(xy[off[i]:off[i + 1], 1] / sp.res).astype(int) + int(origins[i, 1]) + 1000) for i in q]
            assert any(min(r) < 1024 <= max(r) for r in rows if r)  # a window with cells on both sides of the step


def test_many_queries_differ_between_a_workgroups_trips():
    grid, spec, origins = T.many_queries()
    xy, off, stats = T.many_queries_windows()
    assert len(origins) == 16700 == max(T.N_MANY_QUERIES) and spec.side == 3 and (spec.width, spec.height) == (17, 130)
    counts = np.diff(off)
    later = np.arange(16384, 16700)
    assert (origins[later] != origins[later - 16384]).any(axis=1).all()
    differ = [not np.array_equal(xy[off[q]:off[q + 1]], xy[off[q - 16384]:off[q - 16384 + 1]]) for q in later]
    assert sum(differ) > 200 and (counts[later] > 0).sum() > 100 and (counts[later] == 0).sum() > 20
    assert stats[3] == (counts == 0).sum() > 1000
    h = hostside.map_windows(grid, product(localize.default_spec, spec, LR.FIELDS), origins[:400])
    LR.same(h, LR.map_windows(grid, spec, origins[:400]), "hostside")


def test_wide_windows_cover_more_than_256_rows_of_the_map():
    grid, spec, origins = T.wide_window_map()
    for side in (255, 256, 257):
        sp = T.with_side(spec, side)
        xy, off, stats = LR.map_windows(grid, sp, origins)
        LR.same(hostside.map_windows(grid, product(localize.default_spec, sp, LR.FIELDS), origins), (xy, off, stats), "hostside")
        assert stats[4] == stats[0] and stats[3] >= 1 and (np.diff(off) > 0).sum() >= 5  # the whole map, a part, nothing
    # a window whose LAST row alone (row 256 of side 257) meets the map, and one whose first row alone does
    sp = T.with_side(spec, 257)
    xy, off, _ = LR.map_windows(grid, sp, origins)
    k_lo, k_hi = -(257 // 2), 257 - 257 // 2 - 1
    rows = [set(np.floor(xy[off[i]:off[i + 1], 1] / sp.res).astype(int).tolist()) for i in range(len(origins))]
    assert {k_hi} in rows and {k_lo} in rows


# ---------------------------------------------------------------- K21: the lattice
@pytest.mark.parametrize("name", [c[0] for c in T.lattice_cases()])
def test_lattice_maps_have_anchors_on_both_sides_of_the_steps(name):
    _, grid, spec = next(c for c in T.lattice_cases() if c[0] == name)
    anchors, sig, stats = T.lattice_results()[name]
    h = hostside.range_signatures(grid, product(rangesig.default_spec, spec, RR.FIELDS))
    assert np.array_equal(h[0], anchors) and np.array_equal(h[1], sig) and h[2].tolist() == stats.tolist()
    ni, nj = (spec.width + spec.stride - 1 - spec.stride // 2) // spec.stride, (spec.height + spec.stride - 1 - spec.stride // 2) // spec.stride
    assert stats[0] == ni * nj and stats[1] == len(anchors) > 0
    per_row = np.bincount(anchors[:, 3], minlength=nj)
    if name.startswith("nj"):
        assert nj == int(name.split()[1]) and 3 <= ni <= 8 and per_row.max() == 3 and per_row.min() == 0
        for seam in range(1024, nj, 1024):
            assert per_row[seam - 1] > 0 and per_row[seam] > 0
        if nj > 1024:
            assert 0 < per_row[:1024].sum() <= len(anchors) - 1  # (a capacity one short cuts in a later step than the first)
    else:
        assert nj == 5 and ni == int(name.split()[1]) and per_row[0] == ni and per_row[1] == 0  # a full row, an empty one
        assert anchors[anchors[:, 3] == 2, 2].tolist() == sorted({63, min(64, ni - 1), ni - 1})  # the steps' last and first nodes


# ---------------------------------------------------------------- K21: the match
def test_match_workspaces_give_chunks_that_are_no_multiple_of_eight():
    qs, ms, an, spec, records = T.match_case()
    assert T.key_row_bytes(T.MATCH_A) == 512 and T.key_row_bytes(64) == 256 and T.key_row_bytes(0) == 256
    assert [T.chunk_rows(rows * 512, T.MATCH_A) for rows in T.MATCH_CHUNK_ROWS] == [3, 8, 9, 12]
    assert T.chunk_rows(512 * 4 + 511, T.MATCH_A) == 4
    # the workspace the library asks for holds every query: one chunk of Q rows, Q % 8 in {7, 0, 1, 0, 1}
    ps = product(rangesig.default_spec, spec, RR.FIELDS)
    for Q in T.MATCH_QUERIES:
        assert T.chunk_rows(rangesig.workspace_bytes(ps, T.MATCH_A, Q), T.MATCH_A) >= Q
        want, (none, written) = RR.match(qs[:Q], ms, an, spec) if Q in (7, 9) else (records[:Q], (None, None))
        assert np.array_equal(want, records[:Q])  # (a query's records depend on no other query)
        h_rec, h_stats = hostside.signature_candidates(qs[:Q], ms, an, ps)
        assert np.array_equal(h_rec, records[:Q])
    assert (records[5] == -1).all() and (records[13] == -1).all() and (records[[0, 7, 8, 24], 0, 0] >= 0).all()


# ---------------------------------------------------------------- the sector count
def test_boundary_points_fall_into_the_sector_that_starts_there():
    pts = T.boundary_points()
    assert len(pts) == 31 * 3 * 2 * 3
    _, dirs = PR.make_tables(8, 64.0)
    assert np.array_equal(dirs, np.array(RR.DIRS, np.float32))
    moved = 0
    for x, y, j, kind in pts:
        neg = y < 0 or (y == 0 and x < 0)
        u, v = (-x, -y) if neg else (x, y)
        cross = np.float32(np.float32(RR.DIRS[j][0] * v) - np.float32(RR.DIRS[j][1] * u))
        sector = RR.point_sector(x, y)
        assert sector == PR.point_bins([(x, y)], *PR.make_tables(8, 64.0))[1][0]
        if kind == 0:
            assert cross == 0 and sector == j + (32 if neg else 0), (x, y, j)  # `>=`: the boundary belongs to the sector it starts
        else:
            # one float beside it the products may still round alike (cross 0: sector j); else the sign of the difference decides
            assert sector in (j + (32 if neg else 0), j - 1 + (32 if neg else 0)), (x, y, j, kind)
            assert (sector % 32 == j) == (cross >= 0)
            moved += cross != 0
            if cross != 0 and RR.DIRS[j][0] > 1e-3:
                assert (cross > 0) == ((kind > 0) != neg)  # (v up: towards the higher sector, in the mirrored half-plane down)
    assert moved > len(pts) // 3  # (most neighbours do leave the boundary, to either side)
    xy, off = T.boundary_scans()
    ps = product(rangesig.default_spec, RR.make_spec(), RR.FIELDS)
    assert np.array_equal(hostside.scan_signatures(xy, off, ps), RR.scan_signatures(xy, off, RR.make_spec()))
    ps = place.spec(n_rings=8, range_max=64.0)
    D, bits = PR.describe(xy, off, *PR.make_tables(8, 64.0))
    h_D, h_bits = hostside.place_descriptors(xy, off, ps)
    assert np.array_equal(h_D, D) and (bits == 1).all()  # (2^5 = 32 m lies inside range_max 64: no point is dropped)


def test_point_sector_is_the_angles_sector_away_from_the_boundaries():
    xy, off, _ = RR.scan_case()
    pts = xy[off[1]:off[7]]  # the random scans: 1 .. 3000 points, uniform in angle
    assert len(pts) == 1 + 63 + 64 + 65 + 1081 + 3000
    LD = np.longdouble
    two_pi = 2 * np.arctan2(LD(0), LD(-1))
    a = np.arctan2(pts[:, 1].astype(LD), pts[:, 0].astype(LD)) % two_pi
    t = a / (two_pi / 64)
    away = np.abs(t - np.rint(t)) * (two_pi / 64) > LD(1e-5)
    left_out = int((~away).sum())
    assert left_out < 0.01 * len(pts)  # (uniform angles: about 64 * 2e-5 / 2 pi = 0.02 % lie that close)
    for (x, y), sector in zip(pts[away], np.floor(t[away]).astype(int)):
        assert RR.point_sector(x, y) == sector
    assert np.array_equal(PR.point_bins(pts[away], *PR.make_tables(10, 30.0))[1], np.floor(t[away]).astype(int))
