"""The place descriptors on the GPU (K16, nhip_place.hip) against the numpy restatement (tests/place_reference.py), through the
C ABI: descriptors, bit counts, records and stats must be equal byte for byte.  One scene of 130 small scans: the degenerate
ones, the hand-built edge points, duplicates, a mirror image, a scan that is its own half turn, rotated copies, random ones."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from nautilus_amd import _lib, csm, place
from tests import place_reference as R

pytestmark = pytest.mark.gpu
f32 = np.float32
N_SCENE = 130


@functools.lru_cache(maxsize=None)
def scene():
    """(xy, offsets) of N_SCENE scans.  0: no point; 1: one point; 2: 1081 points in one bin; 3: the edge points of
    tests/test_place_cpu.py; 4, 5: the same scan twice; 6: its mirror image; 7: a scan that equals its own half turn; 8..: random
    scans of 1..300 points, every third a rotated copy of an earlier one (by a whole number of sectors, up to rounding)."""
    rng = np.random.default_rng(130)
    nan, inf = float("nan"), float("inf")
    _, dirs = R.make_tables(10, 30.0)
    edge = [(0.0, 0.0), (-1.0, 0.0), (-1.0, -0.0), (1.0, -0.0), (30.0, 0.0), (0.0, -30.0), (float(np.nextafter(f32(30.0), f32(0))), 0.0),
            (18.0, 24.0), (nan, 1.0), (1.0, nan), (inf, 0.0), (0.0, -inf), (1e30, 1.0), (nan, nan)]
    edge += [(3.0 * k, 0.0) for k in range(1, 10)] + [(0.0, 3.0 * k) for k in range(1, 10)]
    edge += [(float(np.nextafter(f32(3.0 * k), f32(0))), 0.0) for k in range(1, 10)]
    edge += [(float(dirs[j, 0] * f32(8.0)), float(dirs[j, 1] * f32(8.0))) for j in range(32)]
    edge += [(-float(dirs[j, 0] * f32(8.0)), -float(dirs[j, 1] * f32(8.0))) for j in range(32)]
    edge += [(float(dirs[8, 0] * f32(8.0)), float(np.nextafter(dirs[8, 1] * f32(8.0), f32(0))))]
    a = rng.uniform(-25, 25, (200, 2))
    half = rng.uniform(-25, 25, (60, 2))
    scans = [np.zeros((0, 2)), np.array([[2.0, 5.0]]), np.tile([[4.01, 1.0]], (1081, 1)) + rng.uniform(0, 0.01, (1081, 2)),
             np.array(edge), a, a.copy(), a * [1.0, -1.0], np.concatenate([half, -half])]
    while len(scans) < N_SCENE:
        if len(scans) % 3 == 0:
            src, k = scans[int(rng.integers(4, len(scans)))], int(rng.integers(1, 64))
            c, s = math.cos(k * 2 * math.pi / 64), math.sin(k * 2 * math.pi / 64)
            scans.append(src @ np.array([[c, s], [-s, c]]))
        else:
            scans.append(rng.uniform(-32, 32, (int(rng.integers(1, 301)), 2)))
    off = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int32)
    return np.concatenate(scans).astype(f32), off


@functools.lru_cache(maxsize=None)
def want_descriptors(n_rings, range_max=30.0):
    xy, off = scene()
    return R.describe(xy, off, *R.make_tables(n_rings, range_max))


@functools.lru_cache(maxsize=None)
def want_match(ids, n_rings, top_k, min_separation, max_permille, flags):
    D, bits = want_descriptors(n_rings)
    return R.match(D, bits, np.array(ids, dtype=np.int64), top_k, min_separation, max_permille, flags)


class Rig:
    """The scene on the device, torch as the allocator; every call ends with nhip_dev_status."""

    def __init__(self, device="cuda:0"):
        import torch
        self.torch, self.lib, self.dev = torch, _lib.load(), torch.device(device)
        xy, off = scene()
        self.t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self.d_xy, self.d_off = self.t(xy), self.t(np.append(off, off[-1]).astype(np.int32))  # (one offset more than needed)
        self.sp = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def status(self):
        info = (C.c_int32 * 4)()
        return self.lib.nhip_dev_status(self.sp, info), list(info)

    def describe(self, n_scans, spec, d_off=None):
        d_desc, d_bits = place.describe_on_device(self.d_xy, self.d_off if d_off is None else d_off, n_scans, spec)
        return d_desc, d_bits, self.status()

    def match(self, d_desc, d_bits, n_scans, ids, spec, workspace=None):
        d_ids = self.t(np.asarray(ids, dtype=np.int32)) if len(ids) else self.torch.zeros(1, dtype=self.torch.int32, device=self.dev)
        d_rec, d_stats = place.match_on_device(d_desc, d_bits, n_scans, d_ids, len(ids), spec, workspace)
        rc = self.status()
        return d_rec.cpu().numpy(), d_stats.cpu().numpy(), rc


@functools.lru_cache(maxsize=None)
def rig():
    return Rig()


def u64(d_desc):
    return d_desc.cpu().numpy().view(np.uint64)


def run_case(ids, n_scans=N_SCENE, workspace=None, **kw):
    """describe + match of the first n_scans scans on the device, compared with the restatement; returns what the device gave"""
    sp = place.spec(**kw)
    d_desc, d_bits, st = rig().describe(n_scans, sp)
    assert st[0] == _lib.NHIP_OK
    D, bits = want_descriptors(sp.n_rings)
    assert u64(d_desc).tobytes() == D[:n_scans].tobytes() and d_bits.cpu().numpy().tobytes() == bits[:n_scans].tobytes()
    rec, stats, st = rig().match(d_desc, d_bits, n_scans, ids, sp, workspace)
    assert st[0] == _lib.NHIP_OK, st
    want_rec, want_stats = want_match(tuple(int(i) for i in ids), sp.n_rings, sp.top_k, sp.min_separation, sp.max_permille, sp.flags)
    assert rec.dtype == np.int32 and rec.shape == want_rec.shape and stats.tobytes() == want_stats.tobytes(), (stats, want_stats)
    assert rec.tobytes() == want_rec.tobytes()
    return rec, stats


def test_descriptors_of_the_degenerate_scans_and_the_edge_points(gpu):
    sp = place.default_spec()
    d_desc, d_bits, st = rig().describe(N_SCENE, sp)
    assert st[0] == _lib.NHIP_OK
    D, bits = u64(d_desc), d_bits.cpu().numpy()
    want_D, want_bits = want_descriptors(10)
    assert D.tobytes() == want_D.tobytes() and bits.tobytes() == want_bits.tobytes()
    assert bits[0] == 0 and bits[1] == 1 and bits[2] == 1 and not D[0].any()
    assert D[2, 1] == 1 << 2 and D[1, 1] == 1 << 12  # (4.01, 1): 14 degrees, ring [3, 6); (2, 5): 68.2 degrees, sector 12
    # the edge points, word by word: the origin in sector 31 and (-1, +-0) in 32 of ring 0; the ring edges on both axes ...
    both_axes = (1 << 0) | (1 << 16)
    assert D[3, 0] == (1 << 31) | (1 << 32) | (1 << 0) and D[3, 1] == both_axes
    assert D[3, 2] == 0xFFFFFFFFFFFFFFFF                    # ... every direction at radius 8 (and the point just below dir[8])
    assert D[3, 9] == both_axes and D[3, 8] == both_axes  # (30 - ulp, 0) in the last ring; r2 == edge2[R] dropped
    assert np.all(bits[4:8] > 40) and bits[4] == bits[5] == bits[6]
    # a descriptor may have up to 32 rings (a match up to 15): the widest and the narrowest
    for n_rings in (1, 15, 32):
        d_desc, d_bits, st = rig().describe(N_SCENE, place.spec(n_rings=n_rings))
        want_D, want_bits = want_descriptors(n_rings)
        assert st[0] == _lib.NHIP_OK and u64(d_desc).tobytes() == want_D.tobytes() and d_bits.cpu().numpy().tobytes() == want_bits.tobytes()
    # offsets that are not a scan: treated as empty, reported
    xy, off = scene()
    bad = np.array([0, 5, 3, 8, 8], dtype=np.int32)
    d_desc, d_bits, st = rig().describe(3, sp, rig().t(bad))
    got = u64(d_desc)
    assert st[0] == _lib.NHIP_ERR_ARG and st[1][0] & 16384 and st[1][1:] == [16384, 3, 2]
    want_D, want_bits = R.describe(np.concatenate([xy[0:5], xy[3:8]]), [0, 5, 5, 10], *R.make_tables(10, 30.0))
    assert np.array_equal(got, want_D) and np.array_equal(d_bits.cpu().numpy(), want_bits) and want_bits.tolist() == [2, 0, 1]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 130])
def test_scan_counts_at_the_lane_and_tile_seams(gpu, n):
    rec, stats = run_case(np.arange(n), n_scans=n, min_separation=0)
    assert stats[0] == n and (n < 8 or (rec[4:8, 0, 0] >= 0).all())


@pytest.mark.parametrize("n_rings", [1, 15])
def test_ring_counts(gpu, n_rings):
    run_case(np.arange(N_SCENE), n_rings=n_rings, top_k=3, min_separation=2)


def test_more_rings_than_the_key_admits_are_refused(gpu):
    lib, r = _lib.load(), rig()
    sp = place.spec(n_rings=16)
    d_desc, d_bits, _ = r.describe(4, sp)
    d_out = r.torch.full((64,), -7, dtype=r.torch.int32, device=r.dev)
    rc = lib.nhip_place_match_dev(d_desc.data_ptr(), d_bits.data_ptr(), 4, d_out.data_ptr(), 2, C.byref(sp), d_out.data_ptr(),
                                  d_out.data_ptr(), d_out.data_ptr(), 256, r.sp)
    assert rc == _lib.NHIP_ERR_ARG and b"n_rings" in lib.nhip_last_error() and (d_out.cpu().numpy() == -7).all()


def test_top_k_one_and_padding(gpu):
    one, _ = run_case(np.arange(N_SCENE), top_k=1, min_separation=0)
    five, _ = run_case(np.arange(N_SCENE), top_k=5, min_separation=0)
    assert np.array_equal(one[:, 0], five[:, 0])
    rec, stats = run_case(np.arange(20), n_scans=20, top_k=32, min_separation=0)
    assert (rec[5, :18, 0] >= 0).all() and (rec[5, 18:] == -1).all() and (rec[0] == -1).all() and stats[3] == 19 * 18


def test_separation(gpu):
    rec, stats = run_case(np.arange(N_SCENE), min_separation=0)
    assert rec[4, 0].tolist()[:3] == [5, 0, 0] and rec[5, 0].tolist()[:3] == [4, 0, 0]  # the duplicate, nobody else at distance 0
    rec, stats = run_case(np.arange(N_SCENE), min_separation=20)
    assert (np.abs(rec[:, :, 0] - np.arange(N_SCENE)[:, None])[rec[:, :, 0] >= 0] > 20).all()
    for sep in (N_SCENE - 1, N_SCENE, 1 << 30):
        rec, stats = run_case(np.arange(N_SCENE), min_separation=sep)
        assert (rec == -1).all() and stats.tolist() == [N_SCENE, 0, 0, 0, N_SCENE, 1, 0, 0]


def test_past_only_and_the_permille_gate(gpu):
    both, _ = run_case(np.arange(N_SCENE), min_separation=1)
    past, pstats = run_case(np.arange(N_SCENE), min_separation=1, flags=place.NHIP_PLACE_PAST_ONLY)
    assert (past[:, :, 0] < np.arange(N_SCENE)[:, None]).all() and (both[:, :, 0] > np.arange(N_SCENE)[:, None]).any()
    assert (past[:3] == -1).all()
    # 0 permille keeps only descriptors that are identical under some rotation: the duplicated scan first
    rec, stats = run_case(np.arange(N_SCENE), min_separation=0, max_permille=0, top_k=32)
    D, bits = want_descriptors(10)
    assert rec[4, 0].tolist() == [5, 0, 0, bits[5]] and rec[5, 0].tolist() == [4, 0, 0, bits[4]]
    assert (rec[:, :, 2][rec[:, :, 0] >= 0] == 0).all() and 2 <= stats[2] == stats[3] < stats[1] // 10
    mid, mstats = run_case(np.arange(N_SCENE), min_separation=0, max_permille=700)
    assert 0 < mstats[2] < mstats[1] and (1000 * mid[:, :, 2] <= 700 * (mid[:, :, 3] + bits[:, None]))[mid[:, :, 0] >= 0].all()


def test_ties_go_by_j_then_by_the_smallest_shift(gpu):
    D, bits = want_descriptors(10)
    # duplicates: from any third scan, 4 and 5 are equally far: 4 comes first
    ids = [3, 4, 5, 6, 7, 20, 21]
    rec, _ = run_case(ids, top_k=32, min_separation=0)
    for a in (0, 3, 4, 5):
        js = rec[a, :, 0].tolist()
        assert js.index(5) == js.index(4) + 1 and rec[a, js.index(4), 1:3].tolist() == rec[a, js.index(5), 1:3].tolist()
    # the scan that is its own half turn: every distance to it is met at s and s + 32; the record has the smaller
    all_d = R.dist_all(D[4], D[[7]])[0]
    assert np.array_equal(all_d[:32], all_d[32:])
    row = rec[1, rec[1, :, 0].tolist().index(7)]
    assert row[1] == all_d.argmin() < 32 and row[2] == all_d.min()
    # a scan against its mirror image
    row = rec[1, rec[1, :, 0].tolist().index(6)]
    all_d = R.dist_all(D[4], D[[6]])[0]
    assert row[1] == int(np.flatnonzero(all_d == all_d.min())[0]) and row[2] == all_d.min()


def test_a_list_that_skips_scans(gpu):
    ids = [1, 2, 4, 5, 6, 9, 40, 41, 77, 129]
    rec, stats = run_case(ids, top_k=4, min_separation=1)
    assert np.isin(rec[rec >= 0].reshape(-1, 4)[:, 0], ids).all() and stats[0] == len(ids)
    run_case([129], top_k=2, min_separation=0)
    run_case([], top_k=2, min_separation=0)


def test_chunked_query_rows_equal_one_chunk(gpu):
    sp = place.spec(min_separation=0)
    row = 2 * 192  # bytes of a row of 130 candidates
    assert place.workspace_bytes(sp, N_SCENE) == 144 * row
    whole = run_case(np.arange(N_SCENE), min_separation=0)
    for rows in (16, 64, 128):  # 9, 3 and 2 chunks; the last one partial
        part = run_case(np.arange(N_SCENE), workspace=rows * row + 17, min_separation=0)
        assert part[0].tobytes() == whole[0].tobytes() and part[1].tobytes() == whole[1].tobytes()
    r = rig()
    d_desc, d_bits, _ = r.describe(N_SCENE, sp)
    with pytest.raises(_lib.NhipError, match="workspace"):
        r.match(d_desc, d_bits, N_SCENE, np.arange(N_SCENE), sp, workspace=15 * row)


def test_the_same_call_twice_gives_the_same_bytes(gpu):
    r, sp = rig(), place.spec(min_separation=3, top_k=7)
    runs = []
    for _ in range(2):
        d_desc, d_bits, _ = r.describe(N_SCENE, sp)
        rec, stats, st = r.match(d_desc, d_bits, N_SCENE, np.arange(N_SCENE), sp)
        runs.append(u64(d_desc).tobytes() + d_bits.cpu().numpy().tobytes() + rec.tobytes() + stats.tobytes())
    assert st[0] == _lib.NHIP_OK and runs[0] == runs[1]


def test_the_host_form_equals_the_dev_form_and_checks_its_list(gpu):
    xy, off = scene()
    st = csm.ScanTable(xy, off)
    try:
        for ids, kw in ((np.arange(N_SCENE), dict(min_separation=2)), ([3, 4, 5, 6, 7, 100, 129], dict(min_separation=0, top_k=3, flags=1)),
                        ([], dict())):
            sp = place.spec(**kw)
            rec, stats, D, bits = place.candidates(st, ids, sp, descriptors=True)
            dev_rec, dev_stats = run_case(ids, **kw)
            want_D, want_bits = want_descriptors(10)
            assert rec.tobytes() == dev_rec.tobytes() and stats.tobytes() == dev_stats.tobytes()
            assert D.tobytes() == want_D.tobytes() and bits.tobytes() == want_bits.tobytes()
        # a list that does not ascend strictly, or leaves the scans: NHIP_ERR_ARG with a message, nothing launched or written
        lib, sp = _lib.load(), place.default_spec()
        for bad, word in (([5, 4], b"ascend"), ([4, 4], b"ascend"), ([0, N_SCENE], b"outside"), ([-1, 2], b"outside")):
            ids = np.array(bad, dtype=np.int32)
            rec, stats = np.full((2, 5, 4), -7, np.int32), np.full(8, -7, np.int64)
            rc = lib.nhip_place_candidates(st._h, _lib.ptr(ids), 2, C.byref(sp), _lib.ptr(rec), _lib.ptr(stats), None, None)
            assert rc == _lib.NHIP_ERR_ARG and word in lib.nhip_last_error() and (rec == -7).all() and (stats == -7).all()
        assert lib.nhip_dev_status(None, None) == _lib.NHIP_OK
    finally:
        st.close()


def test_an_id_beyond_the_scans_sets_the_status_word(gpu):
    """The _dev form reads its list from device memory: id == n_scans is never dereferenced (the descriptor and offset buffers are
    a row longer than needed, so even a missing check would stay inside them), it is a scan without bits, and it is reported."""
    r, n = rig(), 40
    sp = place.spec(min_separation=0, top_k=3)
    d_desc, d_bits, st = r.describe(n + 1, sp)  # (a row more than the n the match is told about)
    assert st[0] == _lib.NHIP_OK
    ids = [0, 4, 5, 9, 17, 39, n]
    rec, stats, st = r.match(d_desc, d_bits, n, ids, sp)
    assert st[0] == _lib.NHIP_ERR_ARG and st[1] == [65536, 65536, n, 6] and b"nhip_place_match_dev" in _lib.load().nhip_last_error()
    want_rec, want_stats = want_match(tuple(ids[:-1]), 10, 3, 0, 1000, 0)
    assert np.array_equal(rec[:-1], want_rec) and (rec[-1] == -1).all()
    assert stats.tolist() == [7, want_stats[1], want_stats[2], want_stats[3], want_stats[4] + 1, want_stats[5] + 1, 0, 0]
    assert r.status()[0] == _lib.NHIP_OK  # (the report was consumed)
