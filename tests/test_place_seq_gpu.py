"""The place sequences on the GPU (K16b, nhip_place_seq.hip) against the numpy restatement (tests/place_seq_reference.py), through
the C ABI: records and stats must be equal byte for byte.  The descriptors are uploaded directly as uint64 words (the crafted sets
of tests/place_seq_cases.py); one case goes through describe on real clouds.  Every call is followed by nhip_dev_status."""
import ctypes as C
import functools

import numpy as np
import pytest

from nautilus_amd import _lib, csm, hostside, place, posegraph
from tests import place_reference as R
from tests import place_seq_cases as cases
from tests import place_seq_reference as Q

pytestmark = pytest.mark.gpu


def specs(kw):
    kw = dict(kw)
    seq = place.seq_spec(half_window=kw.pop("half_window"), step=kw.pop("step"))
    return place.spec(**kw), seq


class Rig:
    """Descriptor sets on the device, torch as the allocator; every call ends with nhip_dev_status."""

    def __init__(self, device="cuda:0"):
        import torch
        self.torch, self.lib, self.dev = torch, _lib.load(), torch.device(device)
        self.t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self.sp = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)
        self.sets = {}

    def status(self):
        info = (C.c_int32 * 4)()
        return self.lib.nhip_dev_status(self.sp, info), list(info)

    def upload(self, key):
        """(d_desc, d_bits) of a set, a row longer than the set (an id == n_scans would stay inside even without its check)"""
        if key not in self.sets:
            D, bits = cases.SETS[key]()[:2]
            D = np.concatenate([D, np.zeros((1, D.shape[1]), dtype=np.uint64)])
            self.sets[key] = (self.t(D.view(np.int64)), self.t(np.append(bits, 0).astype(np.int32)), len(bits))
        return self.sets[key]

    def ids(self, ids):
        return self.t(np.asarray(ids, dtype=np.int32)) if len(ids) else self.torch.zeros(1, dtype=self.torch.int32, device=self.dev)

    def sequence(self, key, ids, sp, sq, workspace=None, n_scans=None):
        d_desc, d_bits, n = self.upload(key)
        d_rec, d_stats = place.sequence_match_on_device(d_desc, d_bits, n if n_scans is None else n_scans, self.ids(ids), len(ids), sp, sq,
                                                        workspace)
        st = self.status()
        return d_rec.cpu().numpy(), d_stats.cpu().numpy(), st

    def single(self, key, ids, sp):
        d_desc, d_bits, n = self.upload(key)
        d_rec, d_stats = place.match_on_device(d_desc, d_bits, n, self.ids(ids), len(ids), sp)
        st = self.status()
        return d_rec.cpu().numpy(), d_stats.cpu().numpy(), st


@functools.lru_cache(maxsize=None)
def rig():
    return Rig()


def run_case(key, ids, kw, workspace=None):
    """the set `key` on the device, compared with the restatement; returns what the device gave"""
    sp, sq = specs(kw)
    rec, stats, st = rig().sequence(key, ids, sp, sq, workspace)
    assert st[0] == _lib.NHIP_OK, st
    want_rec, want_stats = cases.want(key, tuple(int(i) for i in ids), **kw)
    assert rec.dtype == np.int32 and rec.shape == want_rec.shape and stats.tobytes() == want_stats.tobytes(), (stats, want_stats)
    assert rec.tobytes() == want_rec.tobytes()
    return rec, stats


@pytest.mark.parametrize("name,key,ids,kw", cases.cases(), ids=[c[0] for c in cases.cases()])
def test_the_device_equals_the_restatement(gpu, name, key, ids, kw):
    """Lane, wave and workgroup seams with windows over both ends; direction; frames without bits; the gate on the window; lists
    whose window frames are not entries; PAST_ONLY; top_k 1 and 32; the largest admitted sums (what each set is crafted for is
    asserted on the restatement in tests/test_place_seq_cpu.py)."""
    rec, stats = run_case(key, ids, kw)
    if name == "largest":
        assert rec[:, :, 2].max() == 959 and rec[:, :, 5].max() == 16303 and rec[50, -1].tolist()[2:] == [959, 960, 16303, 16303, 17, 0]
    if name == "halves-reversed":
        assert rec[50, 0].tolist() == [29, 5, 0, rec[50, 0, 3], 0, 0, 5, 1]


def test_half_window_zero_is_the_single_scan_kernels_answer(gpu):
    """W = 0 against nhip_place_match_dev, which tests/test_place_gpu.py pins: fields 0..3 and stats 0..5 byte for byte."""
    for ids, kw in ((np.arange(130), dict(top_k=5, min_separation=0)), (np.arange(130), dict(top_k=3, min_separation=2, flags=R.PAST_ONLY)),
                    (np.arange(0, 130, 3), dict(top_k=32, min_separation=1, max_permille=700))):
        rec, stats = run_case("identity", ids, dict(kw, half_window=0, step=1))
        one, one_stats, st = rig().single("identity", ids, place.spec(**kw))
        assert st[0] == _lib.NHIP_OK
        assert rec[:, :, :4].tobytes() == one.tobytes() and stats[:6].tobytes() == one_stats[:6].tobytes() and stats[6] == stats[7] == 0
        filled = rec[:, :, 0] >= 0
        assert np.array_equal(rec[:, :, 4], rec[:, :, 2]) and np.array_equal(rec[:, :, 5], rec[:, :, 2])
        assert (rec[:, :, 6][filled] == 1).all() and (rec[:, :, 7][filled] == 0).all()
    run_case("identity", [129], dict(top_k=2, min_separation=4, half_window=2, step=1))
    run_case("identity", [], dict(top_k=2, min_separation=4, half_window=2, step=1))


def test_chunked_query_scans_equal_one_chunk(gpu):
    """257 scans, W = 8, step 3: the halo is 24 scans on either side, chunk borders fall inside windows"""
    kw = cases.seam(257, 8, 3)[3]
    sp, sq = specs(kw)
    ids = np.arange(257)
    row = 2 * 320  # bytes of a row of 257 keys
    full = place.seq_workspace_bytes(sp, sq, 257, 257)
    least = 16 * 2 * row + 48 * row
    assert full == 257 * 2 * row
    whole = run_case("seam-257", ids, kw)
    for ws in (least, least + 2 * row, least + 2 * row + 17, 100 * 2 * row + 48 * row, full - 1):  # 17, 16, 16, 3 and 2 chunks
        part = run_case("seam-257", ids, kw, workspace=ws)
        assert part[0].tobytes() == whole[0].tobytes() and part[1].tobytes() == whole[1].tobytes()
    again = run_case("seam-257", ids, kw)  # the same call twice gives the same bytes
    assert again[0].tobytes() == whole[0].tobytes() and again[1].tobytes() == whole[1].tobytes()
    with pytest.raises(_lib.NhipError, match="workspace"):
        rig().sequence("seam-257", ids, sp, sq, workspace=least - 1)
    # a list that skips scans, chunked: the entries of a chunk are those whose scan ids it holds
    lkw = dict(top_k=4, min_separation=12, half_window=2, step=3)
    run_case("list", cases.list_ids(), lkw, workspace=16 * (2 * 256 + 2 * 64) + 12 * 2 * 256)  # (200 scans, 32 entries: 13 chunks)


def test_more_rings_than_the_key_admits_and_windows_that_touch_are_refused(gpu):
    lib, r = _lib.load(), rig()
    d_desc, d_bits, n = r.upload("identity")
    d_out = r.torch.full((64,), -7, dtype=r.torch.int32, device=r.dev)
    for sp, sq, word in ((place.spec(n_rings=16), place.default_seq_spec(), b"n_rings"),
                         (place.spec(min_separation=3), place.default_seq_spec(), b"min_separation"),
                         (place.spec(), place.seq_spec(half_window=9), b"half_window"), (place.spec(), place.seq_spec(step=0), b"step")):
        rc = lib.nhip_place_seq_match_dev(d_desc.data_ptr(), d_bits.data_ptr(), 4, d_out.data_ptr(), 2, C.byref(sp), C.byref(sq),
                                          d_out.data_ptr(), d_out.data_ptr(), d_out.data_ptr(), 256, r.sp)
        assert rc == _lib.NHIP_ERR_ARG and word in lib.nhip_last_error() and (d_out.cpu().numpy() == -7).all()
    assert r.status()[0] == _lib.NHIP_OK


def test_an_id_beyond_the_scans_sets_the_status_word(gpu):
    """The _dev form reads its list from device memory: id == n_scans is never dereferenced (the buffers are a row longer than
    needed, so even a missing check would stay inside them), it is a scan without bits, and it is reported.  A window frame beyond
    the scans is no error: the entries next to the end have such frames."""
    r, n = rig(), 130
    kw = dict(top_k=3, min_separation=4, half_window=2, step=1)
    sp, sq = specs(kw)
    ids = [0, 4, 5, 9, 17, 39, 128, 129, n]
    rec, stats, st = r.sequence("identity", ids, sp, sq)
    assert st[0] == _lib.NHIP_ERR_ARG and st[1] == [65536, 65536, n, 8] and b"nhip_place_seq_match_dev" in _lib.load().nhip_last_error()
    want_rec, want_stats = cases.want("identity", tuple(ids[:-1]), **kw)
    assert np.array_equal(rec[:-1], want_rec) and (rec[-1] == -1).all()
    assert stats.tolist() == [9, want_stats[1], want_stats[2], want_stats[3], want_stats[4] + 1, want_stats[5] + 1, want_stats[6], want_stats[7]]
    assert r.status()[0] == _lib.NHIP_OK  # (the report was consumed)
    # the restatement treats such an entry the same way
    full_rec, full_stats = Q.match(*cases.identity_set(), np.array(ids), 3, 4, 1000, 0, 2, 1, tables=cases.tables("identity"))
    assert rec.tobytes() == full_rec.tobytes() and stats.tobytes() == full_stats.tobytes()


N_SCENE = 130


@functools.lru_cache(maxsize=None)
def scene():
    """(xy, offsets) of 130 scans of a walk through a random field of 400 landmarks, seen within 12 m from a pose that moves on by
    0.4 m and turns by 3 degrees a scan; the second half retraces the first backwards.  Scans 20 and 77 are empty."""
    rng = np.random.default_rng(1300)
    marks = rng.uniform(-30, 30, (400, 2))
    k = np.concatenate([np.arange(65), np.arange(64, -1, -1)])
    pos = np.stack([0.4 * k - 13.0, 3.0 * np.sin(0.1 * k)], axis=1)
    heading = np.radians(3.0) * np.arange(N_SCENE)
    scans = []
    for s in range(N_SCENE):
        rel = marks - pos[s] + rng.normal(0, 0.05, marks.shape)
        rel = rel[np.linalg.norm(rel, axis=1) < 12.0]
        c, sn = np.cos(heading[s]), np.sin(heading[s])
        scans.append(np.zeros((0, 2)) if s in (20, 77) else rel @ np.array([[c, -sn], [sn, c]]))
    off = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int32)
    return np.concatenate(scans).astype(np.float32), off


def test_through_describe_the_backend_equals_the_host_path(gpu):
    """Real clouds: HipBackend.place_sequence_candidates uploads the scans of the list AND the window frames the list does not name;
    the handle form equals the _dev form and refuses a list that does not ascend."""
    xy, off = scene()
    backend = posegraph.HipBackend()
    every = np.arange(N_SCENE, dtype=np.int32)
    some = np.unique(np.concatenate([np.arange(0, N_SCENE, 7), [3, 76, 129]])).astype(np.int32)
    for ids, kw in ((every, dict(min_separation=20, flags=place.NHIP_PLACE_PAST_ONLY, half_window=2, step=1)),
                    (some, dict(min_separation=12, top_k=4, half_window=2, step=3)), (some, dict(min_separation=8, top_k=32, max_permille=400,
                                                                                               half_window=1, step=2))):
        sp, sq = specs(kw)
        rec, stats = backend.place_sequence_candidates(xy, off, ids, sp, sq)
        want_rec, want_stats = hostside.place_sequence_candidates(xy, off, ids, sp, sq)
        assert rec.tobytes() == want_rec.tobytes() and stats.tobytes() == want_stats.tobytes()
        assert stats[3] > 0 and (rec[:, :, 6] > 1).any()  # (windows of more than the centre: the frames were uploaded)
    # the second half retraces the first backwards: its best records are the other way round
    rec, stats = backend.place_sequence_candidates(xy, off, every, place.spec(min_separation=20, flags=place.NHIP_PLACE_PAST_ONLY), None)
    assert stats[6] > 0 and (rec[100:125, 0, 7] == 1).sum() > 12
    st = csm.ScanTable(xy, off)
    try:
        sp, sq = specs(dict(min_separation=12, top_k=4, half_window=2, step=3))
        rec, stats = place.sequence_candidates(st, some, sp, sq)
        # the _dev form on the descriptors the library makes of the same clouds
        r = rig()
        d_desc, d_bits = place.describe_on_device(r.t(xy), r.t(off), N_SCENE, sp)
        d_rec, d_stats = place.sequence_match_on_device(d_desc, d_bits, N_SCENE, r.ids(some), len(some), sp, sq)
        assert r.status()[0] == _lib.NHIP_OK
        assert rec.tobytes() == d_rec.cpu().numpy().tobytes() and stats.tobytes() == d_stats.cpu().numpy().tobytes()
        want_rec, want_stats = hostside.place_sequence_candidates(xy, off, some, sp, sq)
        assert rec.tobytes() == want_rec.tobytes() and stats.tobytes() == want_stats.tobytes()
        # a list that does not ascend strictly, or leaves the scans: NHIP_ERR_ARG with a message, nothing launched or written
        lib = _lib.load()
        for bad, word in (([5, 4], b"ascend"), ([4, 4], b"ascend"), ([0, N_SCENE], b"outside"), ([-1, 2], b"outside")):
            ids = np.array(bad, dtype=np.int32)
            out, ostats = np.full((2, 4, 8), -7, np.int32), np.full(8, -7, np.int64)
            rc = lib.nhip_place_seq_candidates(st._h, _lib.ptr(ids), 2, C.byref(sp), C.byref(sq), _lib.ptr(out), _lib.ptr(ostats))
            assert rc == _lib.NHIP_ERR_ARG and word in lib.nhip_last_error() and (out == -7).all() and (ostats == -7).all()
        assert lib.nhip_dev_status(None, None) == _lib.NHIP_OK
    finally:
        st.close()
