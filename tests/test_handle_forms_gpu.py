"""Every handle form (host arrays in, host arrays out) against its `_dev` counterpart on the same tiny input: both launch the
same kernels on the same data, so what they return is compared as bytes, with no tolerance.  The handle forms share one
staged call (nhip_host.h, Staged) for their buffers, copies and waits; this file is what pins that layer.

Shapes: three scans of 40, 64 and 130 points (a scan ends before, on and after a 64-lane chunk), a 64 x 64-cell window for the
map units, five ids or pairs.  Empty edges: a table whose scans are all empty, no ids / pairs / records, optional outputs
passed as null, NHIP_OCC_ACCUMULATE with planes given.  Every output starts from the same fill in both forms, so an element
neither form writes compares equal and one only the handle form's download touches does not."""
import ctypes as C
import functools

import numpy as np
import pytest

from nautilus_amd import _lib, csm
from nautilus_amd._lib import (ConsistencySpec, FeatureSpec, FreespaceSpec, NormalsSpec, OccupancySpec, PlaceSeqSpec, PlaceSpec,
                               TransientSpec, VectorizeSpec, ptr)

pytestmark = pytest.mark.gpu

SIZES = (40, 64, 130)
FILL = 0x5A
W = 64  # the map units' window: 64 x 64 cells of 0.05 m around the origin


def clouds(sizes, seed=3):
    """Scan-like rings (ordered by angle) of 0.6 .. 1.4 m: inside the window and the 3 m grids."""
    rng = np.random.default_rng(seed)
    out = []
    for i, n in enumerate(sizes):
        a = np.sort(rng.uniform(-np.pi, np.pi, n))
        r = 1.0 + 0.3 * np.sin(3 * a + i) + rng.normal(0, 0.01, n)
        out.append(np.stack([r * np.cos(a), r * np.sin(a)], axis=1).astype(np.float32))
    return out


def filled(shape, dtype):
    return np.frombuffer(bytes([FILL]) * (int(np.prod(shape)) * np.dtype(dtype).itemsize), dtype=dtype).reshape(shape).copy()


class Rig:
    """The scans as a handle and as device tensors, three poses and their affines."""

    def __init__(self, sizes):
        import torch
        self.torch, self.lib, self.dev = torch, _lib.load(), torch.device("cuda:0")
        self.sp = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)
        self.alive = []
        self.xy, self.off = csm.pack_scans(clouds(sizes))
        self.n, self.np = len(sizes), int(self.off[-1])
        self.st = csm.ScanTable(self.xy, self.off)
        self.d_xy, self.d_off = self.up(self.xy), self.up(self.off)
        self.poses = np.array([[0.0, 0.0, 0.0], [0.1, -0.05, 0.2], [-0.08, 0.12, -0.3]])[:self.n].copy()
        self.aff = np.zeros((self.n, 4), np.float32)
        _lib.check(self.lib.nhip_map_pose_affines(ptr(self.poses), self.n, ptr(self.aff)))
        self.d_aff = self.up(self.aff)

    def up(self, a):
        """a host array on the device (an empty one: 16 bytes, never a null pointer)"""
        a = np.ascontiguousarray(a)
        t = self.torch.from_numpy(a).to(self.dev) if a.size else self.torch.zeros(16, dtype=self.torch.uint8, device=self.dev)
        self.alive.append(t)  # (kept: a tensor made inside a call's argument list would be released before the call)
        return t

    def out(self, shape, dtype):
        """(the handle form's host output, the dev form's device output): the same fill, the device one padded to 16 bytes"""
        h = filled(shape, dtype)
        pad = max(h.nbytes, 16) + (-max(h.nbytes, 16)) % 16
        d = self.torch.full((pad,), FILL, dtype=self.torch.uint8, device=self.dev)
        return h, d

    def back(self, d, like):
        self.torch.cuda.synchronize()
        return d.cpu().numpy()[:like.nbytes].view(like.dtype).reshape(like.shape)

    def same(self, pairs):
        for k, (h, d) in enumerate(pairs):
            got = self.back(d, h)
            assert h.tobytes() == got.tobytes(), (k, h.ravel()[:8], got.ravel()[:8])


@functools.lru_cache(maxsize=None)
def rig(kind):
    return Rig(SIZES if kind == "full" else (0, 0, 0))


KINDS = ("full", "empty")
P = lambda t: None if t is None else t.data_ptr()


def default(cls, fn, **kw):
    s = cls()
    _lib.check(getattr(_lib.load(), fn)(C.byref(s)))
    for k, v in kw.items():
        setattr(s, k, v)
    return s


# ---------------------------------------------------------------- features, normals
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("scores", (True, False))
def test_features_extract(gpu, kind, scores):
    r = rig(kind)
    spec = default(FeatureSpec, "nhip_feature_spec_default", neighbors_per_side=5, min_neighbors=5, max_planar=8, max_edge=4)
    pi, d_pi = r.out((r.n, 8), np.int32)
    pc, d_pc = r.out(r.n, np.int32)
    ei, d_ei = r.out((r.n, 4), np.int32)
    ec, d_ec = r.out(r.n, np.int32)
    sc, d_sc = r.out(r.np, np.float64)
    assert r.lib.nhip_features_extract(r.st._h, C.byref(spec), ptr(pi), ptr(pc), ptr(ei), ptr(ec), ptr(sc) if scores else None) == 0
    assert r.lib.nhip_features_extract_dev(P(r.d_xy), P(r.d_off), r.n, C.byref(spec), P(d_pi), P(d_pc), P(d_ei), P(d_ec),
                                           P(d_sc) if scores else None, r.sp) == 0
    r.same([(pc, d_pc), (ec, d_ec), (sc, d_sc)])
    assert (pc >= 0).all() and (pc <= 8).all() and (ec >= 0).all() and (ec <= 4).all()
    gpi, gei = r.back(d_pi, pi), r.back(d_ei, ei)
    for s in range(r.n):  # (entries behind a scan's count are not written by the kernel)
        assert np.array_equal(pi[s, :pc[s]], gpi[s, :pc[s]]) and np.array_equal(ei[s, :ec[s]], gei[s, :ec[s]])
    if kind == "full":
        assert pc.sum() + ec.sum() > 0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("info", (True, False))
def test_normals_estimate(gpu, kind, info):
    r = rig(kind)
    spec = default(NormalsSpec, "nhip_normals_spec_default")
    nr, d_nr = r.out((r.np, 2), np.float32)
    inf, d_inf = r.out((r.np, 4), np.int32)
    assert r.lib.nhip_normals_estimate(r.st._h, C.byref(spec), ptr(nr), ptr(inf) if info else None) == 0
    assert r.lib.nhip_normals_estimate_dev(P(r.d_xy), P(r.d_off), r.n, C.byref(spec), P(d_nr), P(d_inf) if info else None, r.sp) == 0
    r.same([(nr, d_nr), (inf, d_inf)])
    if kind == "full":
        assert nr.tobytes() != filled(nr.shape, nr.dtype).tobytes()


# ---------------------------------------------------------------- the map units: vectorize, occupancy, transient
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("max_segments", (16, 0))
def test_vectorize(gpu, kind, max_segments):
    r = rig(kind)
    spec = default(VectorizeSpec, "nhip_vectorize_spec_default", cell_x0=-W // 2, cell_y0=-W // 2, width=W, height=W, min_hits=1,
                   n_theta=30, min_votes=4, min_length=3, max_segments=max_segments)
    max_cells, max_rounds, check_every = 512, 8, 3
    rec, d_rec = r.out((max(max_segments, 1), 10), np.int64)
    st, d_st = r.out(8, np.int32)
    ws = r.lib.nhip_vectorize_workspace_bytes(C.byref(spec), max_cells)
    d_ws = r.torch.empty(ws, dtype=r.torch.uint8, device=r.dev)
    null = max_segments == 0
    assert r.lib.nhip_vectorize(r.st._h, ptr(r.poses), C.byref(spec), max_cells, max_rounds, check_every, None if null else ptr(rec),
                                ptr(st)) == 0
    assert r.lib.nhip_vectorize_dev(P(r.d_xy), P(r.d_off), P(r.d_aff), r.n, C.byref(spec), max_cells, max_rounds, check_every,
                                    None if null else P(d_rec), P(d_st), P(d_ws), ws, r.sp) == 0
    r.same([(st, d_st)])
    k = int(st[1])
    assert 0 <= k <= max_segments and np.array_equal(rec[:k], r.back(d_rec, rec)[:k])
    assert rec[k:].tobytes() == filled(rec[k:].shape, np.int64).tobytes()  # (the handle form downloads the records there are)


def occupancy_spec(flags=0):
    return default(OccupancySpec, "nhip_occupancy_spec_default", cell_x0=-W // 2, cell_y0=-W // 2, width=W, height=W, max_ray_cells=48,
                   flags=flags)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("accumulate", (False, True))
def test_occupancy(gpu, kind, accumulate):
    r = rig(kind)
    spec = occupancy_spec(_lib.NHIP_OCC_ACCUMULATE if accumulate else 0)
    rng = np.random.default_rng(8)
    h0, m0 = rng.integers(0, 5, (W, W)).astype(np.int32), rng.integers(0, 5, (W, W)).astype(np.int32)
    hits, d_hits = r.out((W, W), np.int32)
    miss, d_miss = r.out((W, W), np.int32)
    if accumulate:  # (the planes given are uploaded, added to and returned)
        hits[:], miss[:] = h0, m0
        d_hits, d_miss = r.up(h0), r.up(m0)
    grid, d_grid = r.out((W, W), np.int8)
    st, d_st = r.out(8, np.int64)
    assert r.lib.nhip_occupancy(r.st._h, ptr(r.poses), C.byref(spec), ptr(hits), ptr(miss), ptr(grid), ptr(st)) == 0
    assert r.lib.nhip_occupancy_dev(P(r.d_xy), P(r.d_off), P(r.d_aff), r.n, C.byref(spec), P(d_hits), P(d_miss), P(d_grid), P(d_st),
                                    r.sp) == 0
    r.torch.cuda.synchronize()
    assert hits.tobytes() == d_hits.cpu().numpy().tobytes()[:hits.nbytes] and miss.tobytes() == d_miss.cpu().numpy().tobytes()[:miss.nbytes]
    r.same([(grid, d_grid), (st, d_st)])
    if accumulate:
        assert (hits >= h0).all() and (miss >= m0).all()
    if kind == "full":
        assert hits.sum() > (h0.sum() if accumulate else 0)
    elif accumulate:
        assert np.array_equal(hits, h0) and np.array_equal(miss, m0)


@pytest.mark.parametrize("kind", KINDS)
def test_transient_filter(gpu, kind):
    r = rig(kind)
    # the planes of these scans, so that some returns are seen through
    hits, miss, grid, ost = filled((W, W), np.int32), filled((W, W), np.int32), filled((W, W), np.int8), filled(8, np.int64)
    assert r.lib.nhip_occupancy(r.st._h, ptr(r.poses), C.byref(occupancy_spec()), ptr(hits), ptr(miss), ptr(grid), ptr(ost)) == 0
    spec = default(TransientSpec, "nhip_transient_spec_default", cell_x0=-W // 2, cell_y0=-W // 2, width=W, height=W, min_through=1,
                   transient_permille=100)
    lab, d_lab = r.out(r.np, np.uint8)
    oxy, d_oxy = r.out((r.np, 2), np.float32)
    oo, d_oo = r.out(r.n + 1, np.int32)
    oi, d_oi = r.out(r.np, np.int32)
    st, d_st = r.out(8, np.int64)
    empty = r.np == 0  # (no point: the per-point outputs may be null)
    assert r.lib.nhip_transient_filter(r.st._h, ptr(r.poses), C.byref(spec), ptr(hits), ptr(miss), None if empty else ptr(lab),
                                       None if empty else ptr(oxy), ptr(oo), None if empty else ptr(oi), ptr(st)) == 0
    assert r.lib.nhip_transient_filter_dev(P(r.d_xy), P(r.d_off), r.n, r.np, P(r.d_aff), C.byref(spec), P(r.up(hits)), P(r.up(miss)),
                                           P(d_lab), P(d_oxy), P(d_oo), P(d_oi), P(d_st), r.sp) == 0
    r.same([(lab, d_lab), (oo, d_oo), (st, d_st)])
    kept = int(oo[r.n])
    assert 0 <= kept <= r.np
    assert np.array_equal(oxy[:kept].view(np.int32), r.back(d_oxy, oxy)[:kept].view(np.int32)) and np.array_equal(oi[:kept], r.back(d_oi, oi)[:kept])
    assert oi[kept:].tobytes() == filled(oi[kept:].shape, np.int32).tobytes()  # (the handle form downloads the points kept)


# ---------------------------------------------------------------- the matcher's grids: free space, score volumes
SEARCH = (3, 3, 3)


class GridRig:
    """Tables of every scan: as a handle, and built by nhip_grid_build_dev into a tensor."""

    def __init__(self, r):
        self.r, self.spec = r, csm.grid_spec(3.0, 0.05, 2.0, 1e-10, 8, 16)
        self.ids = np.arange(r.n, dtype=np.int32)
        self.handle = csm.LikelihoodGrids(r.st, self.ids, self.spec)
        t, lib = r.torch, r.lib
        self.d_ids = r.up(self.ids)
        self.d_grids = t.empty(lib.nhip_grids_bytes(C.byref(self.spec), r.n), dtype=t.uint8, device=r.dev)
        self.d_grids[-256:].zero_()
        ws = lib.nhip_grid_workspace_bytes(C.byref(self.spec), r.n)
        d_ws = t.empty(ws, dtype=t.uint8, device=r.dev)
        _lib.check(lib.nhip_grid_build_dev(P(r.d_xy), P(r.d_off), r.n, P(self.d_ids), r.n, C.byref(self.spec), P(self.d_grids), P(d_ws), ws,
                                           r.sp))
        _lib.check(lib.nhip_dev_status(r.sp, None))


@functools.lru_cache(maxsize=None)
def grid_rig(kind):
    return GridRig(rig(kind))


@pytest.mark.parametrize("kind", KINDS)
def test_csm_freespace_twice_on_one_handle(gpu, kind):
    """The first call traces the handle's planes, the second finds them: both return what trace_dev + check_dev return.  With
    and without pair_origin; no pairs is a call that returns at once."""
    g = grid_rig(kind)
    r, lib = g.r, g.r.lib
    search, fs = csm.search_spec(*SEARCH), default(FreespaceSpec, "nhip_freespace_spec_default")
    src = np.array([0, 1, 2, 2, 1], np.int32)
    slot = np.array([1, 2, 0, 1, 1], np.int32)
    theta0 = np.array([0.0, 0.1, -0.2, 0.05, 0.0])
    org = np.array([[0, 0], [1, -1], [2, 0], [-1, 1], [0, 3]], np.int32)
    m = np.zeros(5, dtype=csm.MATCH_DTYPE)
    m["itheta"], m["ix"], m["iy"] = [1, 0, 2, -1, 1], [1, 2, 0, -1, 1], [1, 0, 2, -1, 2]  # (one rejected record)
    d_free = r.torch.empty(max(lib.nhip_freespace_planes_bytes(C.byref(g.spec), r.n), 16), dtype=r.torch.uint8, device=r.dev)
    assert lib.nhip_freespace_trace_dev(P(r.d_xy), P(r.d_off), r.n, P(g.d_ids), r.n, C.byref(g.spec), P(g.d_grids), P(d_free), r.sp) == 0
    rot0, delta = csm.rot0_table(theta0), csm.delta_table(search)
    assert lib.nhip_csm_freespace(r.st._h, g.handle._h, None, None, None, None, 0, C.byref(search), None, C.byref(fs), None) == 0
    for origin in (org, None, org):
        cnt, d_cnt = r.out((5, 8), np.int32)
        assert lib.nhip_freespace_check_dev(P(r.d_xy), P(r.d_off), r.n, P(g.d_grids), r.n, C.byref(g.spec), P(r.up(src)), P(r.up(slot)),
                                            P(r.up(rot0)), P(r.up(delta)), None if origin is None else P(r.up(origin)), 5,
                                            C.byref(search), P(d_free), P(r.up(m.view(np.int32))), C.byref(fs), P(d_cnt), r.sp) == 0
        assert lib.nhip_csm_freespace(r.st._h, g.handle._h, ptr(src), ptr(slot), ptr(theta0), None if origin is None else ptr(origin), 5,
                                      C.byref(search), ptr(m), C.byref(fs), ptr(cnt)) == 0
        r.same([(cnt, d_cnt)])
        assert lib.nhip_dev_status(r.sp, None) == 0
        assert (cnt[3] == -1).all() and (cnt[[0, 1, 2, 4], 0] >= 0).all()  # (the rejected record's counts: eight -1)


@pytest.mark.parametrize("kind", KINDS)
def test_csm_scores(gpu, kind):
    g = grid_rig(kind)
    r, lib = g.r, g.r.lib
    search = csm.search_spec(*SEARCH)
    vol, d_vol = r.out(27, np.int32)
    rot0, delta = csm.rot0_table(np.array([0.1])), csm.delta_table(search)
    assert lib.nhip_csm_scores(r.st._h, g.handle._h, 2, 1, 0.1, 1, -1, C.byref(search), ptr(vol)) == 0
    assert lib.nhip_csm_scores_dev(P(r.d_xy), P(r.d_off), r.n, P(g.d_grids), r.n, C.byref(g.spec), 2, 1, P(r.up(rot0)), P(r.up(delta)), 1, -1,
                                   C.byref(search), P(d_vol), r.sp) == 0
    r.same([(vol, d_vol)])
    assert vol.tobytes() != filled(27, np.int32).tobytes()


# ---------------------------------------------------------------- place descriptors
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ids", ((0, 1, 2), ()))
@pytest.mark.parametrize("form", ("single", "single_with_desc", "seq"))
def test_place_candidates(gpu, kind, ids, form):
    seq, want_desc = form == "seq", form == "single_with_desc"  # (the sequence form returns no descriptors)
    r, lib = rig(kind), rig(kind).lib
    spec = default(PlaceSpec, "nhip_place_spec_default", n_rings=4, range_max=2.0, top_k=2, min_separation=0)
    sq = default(PlaceSeqSpec, "nhip_place_seq_spec_default", half_window=0, step=1)
    ids = np.array(ids, np.int32)
    words = 8 if seq else 4
    rec, d_rec = r.out((max(ids.size, 1), 2, words), np.int32)
    st, d_st = r.out(8, np.int64)
    desc, d_desc = r.out((r.n, 4), np.uint64)
    bits, d_bits = r.out(r.n, np.int32)
    if seq:
        ws = lib.nhip_place_seq_workspace_bytes(C.byref(spec), C.byref(sq), r.n, ids.size)
        rc = lib.nhip_place_seq_candidates(r.st._h, ptr(ids) if ids.size else None, ids.size, C.byref(spec), C.byref(sq),
                                           ptr(rec) if ids.size else None, ptr(st))
    else:
        ws = lib.nhip_place_workspace_bytes(C.byref(spec), ids.size)
        rc = lib.nhip_place_candidates(r.st._h, ptr(ids) if ids.size else None, ids.size, C.byref(spec), ptr(rec) if ids.size else None,
                                       ptr(st), ptr(desc) if want_desc else None, ptr(bits) if want_desc else None)
    assert rc == 0 and ws > 0
    d_ws = r.torch.empty(ws, dtype=r.torch.uint8, device=r.dev)
    assert lib.nhip_place_describe_dev(P(r.d_xy), P(r.d_off), r.n, C.byref(spec), P(d_desc), P(d_bits), r.sp) == 0
    if seq:
        assert lib.nhip_place_seq_match_dev(P(d_desc), P(d_bits), r.n, P(r.up(ids)), ids.size, C.byref(spec), C.byref(sq), P(d_rec), P(d_st),
                                            P(d_ws), ws, r.sp) == 0
    else:
        assert lib.nhip_place_match_dev(P(d_desc), P(d_bits), r.n, P(r.up(ids)), ids.size, C.byref(spec), P(d_rec), P(d_st), P(d_ws), ws,
                                        r.sp) == 0
    r.same([(rec, d_rec), (st, d_st)])
    if want_desc:
        r.same([(desc, d_desc), (bits, d_bits)])
    else:
        assert desc.tobytes() == filled(desc.shape, np.uint64).tobytes()
    assert lib.nhip_dev_status(r.sp, None) == 0


# ---------------------------------------------------------------- consistency
@pytest.mark.parametrize("M", (5, 0))
def test_consistency(gpu, M):
    r, lib = rig("full"), rig("full").lib
    spec = default(ConsistencySpec, "nhip_consistency_spec_default")
    rng = np.random.default_rng(4)
    a = rng.uniform(-0.05, 0.05, M)
    # {cw, sw, xw, yw, px, py, la, lb}: small, mutually compatible corrections, one far off
    recs = np.stack([np.cos(a), np.sin(a), rng.uniform(-0.1, 0.1, M), rng.uniform(-0.1, 0.1, M), rng.uniform(-5, 5, M),
                     rng.uniform(-5, 5, M), np.arange(M) * 10.0, np.arange(M) * 10.0 + 200], axis=1) if M else np.zeros((0, 8))
    if M:
        recs[3, 2] = 30.0
    mem, d_mem = r.out(max(M, 1), np.int32)
    nm, d_nm = r.out(1, np.int32)
    st, d_st = r.out(8, np.int64)
    assert lib.nhip_consistency(ptr(recs) if M else None, M, C.byref(spec), ptr(mem) if M else None, ptr(nm), ptr(st)) == 0
    words = (M + 63) // 64
    d_adj = r.torch.empty(max(8 * M * words, 16), dtype=r.torch.uint8, device=r.dev)
    d_deg = r.torch.empty(max(4 * M, 16), dtype=r.torch.uint8, device=r.dev)
    ws = lib.nhip_consistency_workspace_bytes(M)
    d_ws = r.torch.empty(ws, dtype=r.torch.uint8, device=r.dev)
    assert lib.nhip_consistency_adjacency_dev(P(r.up(recs)), M, C.byref(spec), P(d_adj), P(d_deg), P(d_st), r.sp) == 0
    assert lib.nhip_consistency_set_dev(P(d_adj), P(d_deg), M, C.byref(spec), 0, P(d_mem), P(d_nm), P(d_st), P(d_ws), ws, r.sp) == 0
    r.same([(mem, d_mem), (nm, d_nm), (st, d_st)])
    assert 0 <= nm[0] <= M


# ---------------------------------------------------------------- loop-closure gates
@pytest.mark.parametrize("n", (5, 0))
def test_lc_chi_square_gate(gpu, n):
    r, lib = rig("full"), rig("full").lib
    rng = np.random.default_rng(6)
    poses = np.concatenate([rng.uniform(-2, 2, (7, 2)), rng.uniform(-3, 3, (7, 1))], axis=1)
    src, tgt = rng.integers(0, 7, n).astype(np.int32), rng.integers(0, 7, n).astype(np.int32)
    b = rng.normal(size=(n, 2, 2))
    cov = (b @ b.transpose(0, 2, 1) + 1e-3 * np.eye(2)).astype(np.float32)
    sc, d_sc = r.out(max(n, 1), np.float64)
    fl, d_fl = r.out(max(n, 1), np.uint8)
    assert lib.nhip_lc_chi_square_gate(ptr(poses), 7, ptr(src), ptr(tgt), ptr(cov), n, 5.0, ptr(sc), ptr(fl)) == 0
    assert lib.nhip_lc_chi_square_gate_dev(P(r.up(poses)), 7, P(r.up(src)), P(r.up(tgt)), P(r.up(cov)), n, 5.0, P(d_sc), P(d_fl), r.sp) == 0
    r.same([(sc, d_sc), (fl, d_fl)])
    assert n == 0 or sc.tobytes() != filled(sc.shape, np.float64).tobytes()


@pytest.mark.parametrize("kind", KINDS)
def test_lc_scatter_scores(gpu, kind):
    r = rig(kind)
    sc, d_sc = r.out(r.n, np.float64)
    assert r.lib.nhip_lc_scatter_scores(r.st._h, ptr(sc)) == 0
    assert r.lib.nhip_lc_scatter_scores_dev(P(r.d_xy), P(r.d_off), r.n, P(d_sc), r.sp) == 0
    r.same([(sc, d_sc)])
    assert kind == "empty" or sc.tobytes() != filled(sc.shape, np.float64).tobytes()


@pytest.mark.parametrize("n", (5, 0))
def test_lc_pair_gate(gpu, n):
    r, lib = rig("full"), rig("full").lib
    rng = np.random.default_rng(7)
    poses = np.concatenate([rng.uniform(-2, 2, (9, 2)), rng.uniform(-3, 3, (9, 1))], axis=1)
    cand = np.sort(rng.choice(9, n, replace=False)).astype(np.int32)
    fl, d_fl = r.out(max(n * n, 1), np.uint8)
    assert lib.nhip_lc_pair_gate(ptr(poses), 9, ptr(cand), n, 2.5, 1, ptr(fl)) == 0
    assert lib.nhip_lc_pair_gate_dev(P(r.up(poses)), 9, P(r.up(cand)), n, 2.5, 1, P(d_fl), r.sp) == 0
    r.same([(fl, d_fl)])
    assert n == 0 or fl.tobytes() != filled(fl.shape, np.uint8).tobytes()


# ---------------------------------------------------------------- residuals on host arrays
@pytest.mark.parametrize("n", (5, 0))
@pytest.mark.parametrize("jac", ((True, True), (True, False), (False, False)))
def test_resid_odometry(gpu, n, jac):
    r, lib = rig("full"), rig("full").lib
    rng = np.random.default_rng(9)
    poses = np.concatenate([rng.uniform(-2, 2, (6, 2)), rng.uniform(-3, 3, (6, 1))], axis=1)
    t, rot = rng.normal(size=(n, 2)).astype(np.float32), rng.normal(size=n).astype(np.float32)
    pi, pj = rng.integers(0, 6, n).astype(np.int32), rng.integers(0, 6, n).astype(np.int32)
    res, d_res = r.out((max(n, 1), 3), np.float64)
    ji, d_ji = r.out((max(n, 1), 9), np.float64)
    jj, d_jj = r.out((max(n, 1), 9), np.float64)
    assert lib.nhip_resid_odometry(ptr(t), ptr(rot), ptr(pi), ptr(pj), n, 2.0, 3.0, ptr(poses), 6, ptr(res), ptr(ji) if jac[0] else None,
                                   ptr(jj) if jac[1] else None) == 0
    assert lib.nhip_resid_odometry_dev(P(r.up(t)), P(r.up(rot)), P(r.up(pi)), P(r.up(pj)), n, 2.0, 3.0, P(r.up(poses)), 6, P(d_res),
                                       P(d_ji) if jac[0] else None, P(d_jj) if jac[1] else None, r.sp) == 0
    r.same([(res, d_res), (ji, d_ji), (jj, d_jj)])
    assert n == 0 or res.tobytes() != filled(res.shape, np.float64).tobytes()


@pytest.mark.parametrize("n", (130, 0))
@pytest.mark.parametrize("jac", ((True, True), (False, True), (False, False)))
def test_resid_point_to_line(gpu, n, jac):
    r, lib = rig("full"), rig("full").lib
    rng = np.random.default_rng(10)
    nb = 5
    poses = np.concatenate([rng.uniform(-2, 2, (4, 2)), rng.uniform(-3, 3, (4, 1))], axis=1)
    lposes = np.concatenate([rng.uniform(-2, 2, (3, 2)), rng.uniform(-3, 3, (3, 1))], axis=1)
    seg, pts = rng.normal(size=(nb, 4)).astype(np.float32), rng.normal(size=(n, 2)).astype(np.float32)
    pb = np.sort(rng.integers(0, nb, n)).astype(np.int32)
    bp, bl = rng.integers(0, 4, nb).astype(np.int32), rng.integers(0, 3, nb).astype(np.int32)
    res, d_res = r.out(max(n, 1), np.float64)
    j0, d_j0 = r.out((max(n, 1), 3), np.float64)
    j1, d_j1 = r.out((max(n, 1), 3), np.float64)
    assert lib.nhip_resid_point_to_line(ptr(seg), ptr(pts), ptr(pb), n, ptr(bp), ptr(bl), nb, ptr(poses), 4, ptr(lposes), 3, ptr(res),
                                        ptr(j0) if jac[0] else None, ptr(j1) if jac[1] else None) == 0
    assert lib.nhip_resid_point_to_line_dev(P(r.up(seg)), P(r.up(pts)), P(r.up(pb)), n, P(r.up(bp)), P(r.up(bl)), nb, P(r.up(poses)), 4,
                                            P(r.up(lposes)), 3, P(d_res), P(d_j0) if jac[0] else None, P(d_j1) if jac[1] else None,
                                            r.sp) == 0
    r.same([(res, d_res), (j0, d_j0), (j1, d_j1)])
    assert n == 0 or res.tobytes() != filled(res.shape, np.float64).tobytes()
