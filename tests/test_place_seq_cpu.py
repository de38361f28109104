"""Place sequences without a GPU ("Place sequences"; kernel unit K16b): the pure host calls of the library --
defaults, the refused ranges, the workspace rule -- the numpy restatement (tests/place_seq_reference.py) on a case worked by hand,
its W = 0 identity with the place descriptors' restatement, the product's host path against it on the crafted sets of
tests/place_seq_cases.py, and what the window is for: the recall of the definition on the perturbed lap."""
import ctypes as C
import math

import numpy as np
import pytest

from nautilus_amd import _lib, hostside, place, synth
from tests import place_reference as R
from tests import place_seq_cases as cases
from tests import place_seq_reference as Q

ROW_MAX = 64 << 20


def specs(kw):
    kw = dict(kw)
    seq = place.seq_spec(half_window=kw.pop("half_window"), step=kw.pop("step"))
    return place.spec(**kw), seq


def test_defaults_sizes_and_refused_ranges():
    lib = _lib.load()
    seq = place.default_seq_spec()
    assert (seq.half_window, seq.step) == (2, 1) and C.sizeof(_lib.PlaceSeqSpec) == 8 and C.sizeof(_lib.PlaceSpec) == 24
    assert place.SEQ_RECORD_FIELDS[:4] == place.RECORD_FIELDS and len(place.SEQ_RECORD_FIELDS) == 8
    ok = place.spec(min_separation=16)
    assert place.seq_workspace_bytes(ok, place.seq_spec(half_window=8, step=1), 10, 10) > 0
    assert place.seq_workspace_bytes(place.spec(min_separation=0), place.seq_spec(half_window=0, step=16), 10, 10) > 0
    bad = [(ok, dict(half_window=-1), b"half_window"), (ok, dict(half_window=9), b"half_window"), (ok, dict(step=0), b"step"),
           (ok, dict(step=17), b"step"), (ok, dict(half_window=8, step=2), b"min_separation"),
           (place.spec(min_separation=3), dict(half_window=2, step=1), b"min_separation"),
           (place.spec(n_rings=16), dict(), b"n_rings"), (place.spec(top_k=33), dict(), b"top_k"),
           (place.spec(max_permille=1001), dict(), b"max_permille"), (place.spec(flags=2), dict(), b"flags")]
    for sp, kw, word in bad:
        sq = place.seq_spec(**kw)
        with pytest.raises(_lib.NhipError):
            place.seq_workspace_bytes(sp, sq, 10, 10)
        assert word in lib.nhip_last_error()
        # the launching entry points refuse the same specs before they look for a device or at a pointer
        rc = lib.nhip_place_seq_match_dev(None, None, 10, None, 10, C.byref(sp), C.byref(sq), None, None, None, 0, None)
        assert rc == _lib.NHIP_ERR_ARG and word in lib.nhip_last_error()
        rc = lib.nhip_place_seq_candidates(None, None, 0, C.byref(sp), C.byref(sq), None, None)
        assert rc == _lib.NHIP_ERR_ARG and word in lib.nhip_last_error()
    for n_scans, n_ids in ((-1, 0), (0, -1), (0, (1 << 20) + 1)):
        with pytest.raises(_lib.NhipError):
            place.seq_workspace_bytes(ok, seq, n_scans, n_ids)
    assert lib.nhip_place_seq_spec_default(None) == _lib.NHIP_ERR_ARG
    with pytest.raises(TypeError):
        place.seq_spec(window=3)


def test_workspace_bytes_at_the_minimum_and_at_the_cap():
    row = lambda n: 2 * ((max(n, 1) + 63) // 64 * 64)  # bytes of a row of 2-byte keys, rounded up to 64 of them
    sp = place.spec(min_separation=48)
    # everything at once: a plane row and a key row per scan, no halo
    assert place.seq_workspace_bytes(sp, place.seq_spec(half_window=8, step=3), 257, 257) == 257 * (row(257) + row(257))
    assert place.seq_workspace_bytes(sp, place.default_seq_spec(), 300, 44) == 300 * (row(300) + row(44))
    assert place.seq_workspace_bytes(sp, place.default_seq_spec(), 0, 0) == row(1) + row(1)
    # at the cap: as many query scans as fit beside the halo of 2 W step plane rows
    n, seq = 10000, place.seq_spec(half_window=2, step=3)
    per_scan, halo = row(n) + row(n), 12 * row(n)
    assert n * per_scan > ROW_MAX
    fit = (ROW_MAX - halo) // per_scan
    got = place.seq_workspace_bytes(sp, seq, n, n)
    assert fit > 16 and got == fit * per_scan + halo and got <= ROW_MAX < got + per_scan
    # at the minimum: 16 query scans and their halo, though that is more than the cap
    n = 1 << 20
    got = place.seq_workspace_bytes(sp, place.seq_spec(half_window=8, step=3), n, n)
    assert got == 16 * (row(n) + row(n)) + 48 * row(n) and got > ROW_MAX


def test_six_scans_worked_by_hand():
    """One ring.  Words 1, 11, 111 (binary) twice: dist(1, 11) = 1, dist(1, 111) = 2, dist(11, 111) = 1, equal words 0, every
    minimum already at shift 0.  W = 1, separation 2: the pairs are (3, 0), (4, 0), (4, 1), (5, 0), (5, 1), (5, 2) and their
    mirror images.
      (3, 0): + d=-1 absent (b = -1), d=0 0, d=1 (4, 1) 0: sum 0 of 2 frames, score 0.  - d=-1 (2, 1) 1, d=0 0, d=1 absent: 1 of 2,
              score 1*3 div 2 = 1.  Direction 0.
      (4, 1): + (3, 0) 0, (4, 1) 0, (5, 2) 0: sum 0 of 3 frames.
      (4, 0): + d=-1 absent, (4, 0) 1, (5, 1) 1: 2 of 2, score 3.  - (3, 1) 1, (4, 0) 1, d=1 absent: 2 of 2, score 3.  A tie: 0.
      (5, 2): + (4, 1) 0, (5, 2) 0, d=1 absent (a = 6): 0 of 2.
      (5, 1): + (4, 0) 1, (5, 1) 1: 2 of 2, score 3.  - (4, 2) 1, (5, 1) 1: score 3.  A tie: 0.
      (5, 0): + d=-1 absent, (5, 0) 2: 2 of 1 frame, score 6.  - (4, 1) 0, (5, 0) 2: 2 of 2, score 3.  Direction 1."""
    D = np.array([[1], [3], [7], [1], [3], [7]], dtype=np.uint64)
    bits = np.array([1, 2, 3, 1, 2, 3])
    rec, stats = Q.match(D, bits, np.arange(6), 3, 2, 1000, 0, half_window=1, step=1)
    none = [-1] * 8
    assert rec[3].tolist() == [[0, 0, 0, 1, 0, 0, 2, 0], none, none]
    assert rec[4].tolist() == [[1, 0, 0, 2, 0, 0, 3, 0], [0, 0, 1, 1, 3, 2, 2, 0], none]
    assert rec[5].tolist() == [[2, 0, 0, 3, 0, 0, 2, 0], [0, 0, 2, 1, 3, 2, 2, 1], [1, 0, 1, 2, 3, 2, 2, 0]]
    assert stats.tolist() == [6, 12, 12, 12, 0, 0, 2, 10]  # (5, 0) and (0, 5) are the other way round; (4, 1), (1, 4) are full
    # the gate on the window: (4, 0) has sum 2 against norm (2 + 1) + (3 + 2) = 8: kept at 250 permille, dropped at 249
    kept, _ = Q.match(D, bits, np.arange(6), 3, 2, 250, 0, half_window=1, step=1)
    lost, _ = Q.match(D, bits, np.arange(6), 3, 2, 249, 0, half_window=1, step=1)
    assert kept[4, 1].tolist() == [0, 0, 1, 1, 3, 2, 2, 0] and lost[4].tolist() == [[1, 0, 0, 2, 0, 0, 3, 0], none, none]
    got = hostside.place_sequence_candidates(None, None, np.arange(6), place.spec(n_rings=1, top_k=3, min_separation=2),
                                             place.seq_spec(half_window=1), descriptors=(D, bits))
    assert np.array_equal(got[0], rec) and np.array_equal(got[1], stats)


def test_half_window_zero_is_the_single_scan_match():
    D, bits = cases.identity_set()
    for ids, kw in ((np.arange(130), dict(top_k=5, min_separation=0)), (np.arange(130), dict(top_k=3, min_separation=2, flags=R.PAST_ONLY)),
                    (np.arange(0, 130, 3), dict(top_k=32, min_separation=1, max_permille=700))):
        rec, stats = cases.want("identity", tuple(ids.tolist()), half_window=0, step=1, **kw)
        old_rec, old_stats = R.match(D, bits, ids, kw["top_k"], kw["min_separation"], kw.get("max_permille", 1000), kw.get("flags", 0))
        assert np.array_equal(rec[:, :, :4], old_rec) and np.array_equal(stats[:6], old_stats[:6]) and stats[6] == stats[7] == 0
        filled = rec[:, :, 0] >= 0
        assert filled.any() and np.array_equal(rec[:, :, 4], rec[:, :, 2]) and np.array_equal(rec[:, :, 5], rec[:, :, 2])
        assert (rec[:, :, 6][filled] == 1).all() and (rec[:, :, 7][filled] == 0).all()


@pytest.mark.parametrize("name,key,ids,kw", cases.cases(), ids=[c[0] for c in cases.cases()])
def test_the_host_path_equals_the_restatement(name, key, ids, kw):
    want_rec, want_stats = cases.want(key, tuple(int(i) for i in ids), **kw)
    sp, sq = specs(kw)
    rec, stats = hostside.place_sequence_candidates(None, None, ids, sp, sq, descriptors=cases.SETS[key]()[:2])
    assert rec.dtype == np.int32 and stats.dtype == np.int64
    assert np.array_equal(rec, want_rec) and np.array_equal(stats, want_stats)


def test_what_the_crafted_sets_are_crafted_for():
    """The restatement's answers have the properties the cases were built to show (the device is held to the same bytes)."""
    want = lambda name: next(cases.want(key, tuple(int(i) for i in ids), **kw) for n, key, ids, kw in cases.cases() if n == name)
    # the second half reversed: scan 40 + k revisits 39 - k the other way round, at distance 0 over the whole window
    rec, _ = want("halves-reversed")
    for k in range(6, 34):
        assert rec[40 + k, 0].tolist()[:3] == [39 - k, 5, 0] and rec[40 + k, 0].tolist()[4:] == [0, 0, 5, 1]
    rec, _ = want("halves")  # ... not reversed: the same way round
    for k in range(4, 36):
        assert rec[40 + k, 0].tolist()[:3] == [k, 5, 0] and rec[40 + k, 0].tolist()[4:] == [0, 0, 5, 0]
    rec, stats = want("identical")  # every score ties: direction 0, order by j
    assert stats[6] == 0 and (rec[:, :, 4][rec[:, :, 0] >= 0] == 0).all() and rec[40, :, 0].tolist()[:32] == list(range(32))
    assert rec[0, :, 0].tolist() == list(range(5, 37))
    rec, stats = want("empty")  # frames without bits are absent: the centre between two of them stands alone
    assert stats[5] == 20 and 0 < stats[7] < stats[2] and (rec[53, :, 6] == 1).all() and (rec[52] == -1).all()
    assert set(rec[:, :, 6][rec[:, :, 0] >= 0].tolist()) == {1, 2, 3}
    # the gate on the window, against the gate on the centre (W = 0)
    ids = tuple(range(60))
    seq, sstats = want("gate-200")
    one, _ = cases.want("gate", ids, top_k=32, min_separation=8, max_permille=200, half_window=0, step=1)
    assert 10 in one[50, :, 0] and 10 not in seq[50, :, 0]  # (50, 10): the centre alone passes, the window fails
    assert 20 not in one[55, :, 0] and seq[55, 0].tolist()[:1] == [20] and sstats[2] == 2  # (55, 20): the converse (and (20, 55))
    assert want("gate-0")[1][2] == 0 and want("gate-1000")[1][1] == want("gate-1000")[1][2] == sstats[1]
    assert want("gate-0-identical")[1][2] == want("identical")[1][2] > 0
    rec, _ = want("largest")
    assert rec[:, :, 2].max() == 959 and rec[:, :, 5].max() == 16303 and rec[:, :, 4].max() == 16303
    assert rec[50, -1].tolist()[2:] == [959, 960, 16303, 16303, 17, 0]
    rec, stats = want("list")  # windows whose frames are not entries of the list
    assert stats[0] == 32 and 0 < stats[7] < stats[2] and np.isin(rec[:, :, 0][rec[:, :, 0] >= 0], cases.list_ids()).all()
    past, pstats = want("list-past-only")
    assert pstats[1] * 2 == stats[1] and (past[:, :, 0] < cases.list_ids()[:, None]).all()
    assert np.array_equal(want("list-top-1")[0][:, 0], cases.want("list", tuple(cases.list_ids().tolist()), top_k=4, min_separation=4,
                                                                 half_window=2, step=1)[0][:, 0])
    rec, stats = want("list-top-32")
    assert (rec[:, 19:] == -1).all() and stats[3] == stats[2] == 374
    for n in (63, 64, 65, 257):  # every remainder of the scaling division occurs
        rec, _ = want("seam-%d-W8-step1" % n)
        filled = rec[:, :, 0] >= 0
        assert set(range(9, 18)) <= set(rec[:, :, 6][filled].tolist())
        assert np.array_equal(rec[:, :, 4][filled], (rec[:, :, 5][filled] * 17) // rec[:, :, 6][filled])


def test_refused_lists_and_specs_of_the_host_path():
    D, bits = cases.identity_set()
    for ids in ([5, 4], [4, 4], [0, 130], [-1, 2]):
        with pytest.raises(ValueError):
            hostside.place_sequence_candidates(None, None, ids, place.spec(), None, descriptors=(D, bits))
    with pytest.raises(ValueError):
        hostside.place_sequence_candidates(None, None, [1, 2], place.spec(min_separation=3), None, descriptors=(D, bits))
    rec, stats = hostside.place_sequence_candidates(None, None, [], place.spec(), None, descriptors=(D, bits))
    assert rec.shape == (0, 5, 8) and stats.tolist() == [0] * 8
    src, tgt, th = place.pairs([10, 20], np.array([[[7, 0, 3, 9, 5, 5, 3, 0], [-1] * 8], [[2, 33, 0, 1, 0, 0, 5, 1], [-1] * 8]]))
    assert src.tolist() == [10, 20] and tgt.tolist() == [7, 2] and th.tolist() == [0.0, 31 * 2 * math.pi / 64]


def test_recall_of_the_window_on_a_perturbed_lap():
    """The definition alone, on the world, seed, perturbation, queries and separation of
    tests/test_place_cpu.py::test_recall_of_the_descriptor_on_a_perturbed_lap: every scan of the second lap turned by up to +-90
    degrees and moved by up to +-1 m, each on its own.  Ranked by (seq, j) among the scans more than 40 away.  Measured:
      W = 0: recall@1 0.790, @5 0.894, @10 0.935 (the single-scan test's values)
      W = 1: recall@1 0.935, @5 0.986, @10 0.995
      W = 2: recall@1 0.978, @5 1.000, @10 1.000
    A window averages out what disturbs each scan on its own; it does not resolve the rectangle's symmetry."""
    segs, truth = synth.make_world(), synth.loop_trajectory(800)
    rng = np.random.default_rng(5)
    truth2 = truth.copy()
    truth2[392:, 2] += rng.uniform(-math.pi / 2, math.pi / 2, 408)
    truth2[392:, :2] += rng.uniform(-1, 1, (408, 2))
    ranges, _ = synth.raycast(truth2, segs)
    scans = [synth.ranges_to_cloud(r)[0] for r in ranges]
    off = np.concatenate([[0], np.cumsum([len(s) for s in scans])])
    D, bits = R.describe(np.concatenate(scans), off, *R.make_tables(10, 30.0))
    dist, _ = Q.single_distances(D, bits)
    ids = np.arange(800)
    queries = range(433, 800)
    recall = {}
    for W in (0, 1, 2):
        found = {1: 0, 5: 0, 10: 0}
        for i in queries:
            adm = ids[np.abs(ids - i) > 40]
            score = []
            for j in adm.tolist():
                both = [Q.window(dist, bits, i, j, sigma, W, 1) for sigma in (1, -1)]
                score.append(min((total * (2 * W + 1)) // frames for total, _, frames in both))
            top = adm[np.lexsort((adm, np.array(score)))[:10]]
            near = np.linalg.norm(truth2[top, :2] - truth2[i, :2], axis=1) <= 3.5
            for k in found:
                found[k] += bool(near[:k].any())
        recall[W] = {k: v / len(queries) for k, v in found.items()}
        print("W = %d: recall" % W, {k: round(v, 3) for k, v in recall[W].items()})
    assert [round(recall[0][k], 3) for k in (1, 5, 10)] == [0.790, 0.894, 0.935]
    assert recall[2][1] > recall[0][1] and recall[2][10] >= recall[0][10]
