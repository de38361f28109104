"""Preconditions of the scan-normal edge tests (tests/test_normals_edges_gpu.py), without a GPU: every input of
tests/normals_edges.py still reaches, in the numpy restatement, the capacity of nhip_normals.hip it was crafted for, and no
point the GPU test compares is ambiguous.  An edit of the inputs or specs that stops reaching an edge fails HERE, not silently
on the device.  ("Scan normals"; K9.)"""
import os

import numpy as np
import pytest

from tests import normals_edges as E
from tests import normals_reference as R


def _scans(inp):
    xy, off = E.INPUTS[inp]()
    return xy, off, [slice(off[s], off[s + 1]) for s in range(len(off) - 1)]


def test_the_kernel_constants_are_the_ones_the_inputs_were_cut_for():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "nautilus_amd", "csrc", "nhip_normals.hip")) as f:
        src = f.read()
    for line in ("constexpr int NORMALS_LDS_N = %d;" % E.LDS_POINTS, "constexpr int NORMALS_LDS_TAKEN = %d;" % E.LDS_TAKEN,
                 "constexpr int NORMALS_MAX_TAKEN = %d;" % E.MAX_TAKEN, "constexpr int NORMALS_BINS = %d;" % E.LIVE_BINS,
                 "const dim3 grid((uint32_t)n_scans, NORMALS_TILES_Y);"):
        assert line in src, line


def test_each_spec_has_the_limit_it_is_named_for():
    """64: the last row of the LDS taken list; 65: the first limit that sends every scan to the general kernel; 128: the last
    row of the private list; 1."""
    got = {name: R.sample_limit(E.full_spec(name)["mean_distance"]) for name in E.LIMITS}
    assert got == E.LIMITS == {"lds_full": 64, "general_first": 65, "general_full": 128, "one_sample": 1}
    assert E.LIMITS["lds_full"] == E.LDS_TAKEN and E.LIMITS["general_first"] == E.LDS_TAKEN + 1
    assert E.LIMITS["general_full"] == E.MAX_TAKEN
    for name in ("quotients", "quotients_odd"):
        assert R.sample_limit(E.full_spec(name)["mean_distance"]) == 128
    seeds = [E.full_spec(name)["seed"] for name in E.SPECS]
    assert len(set(seeds)) == len(seeds), "the specs have distinct seeds"
    assert {s for s, _ in E.CASES} == set(E.SPECS) and {i for _, i in E.CASES} == set(E.INPUTS)
    assert [E.full_spec(n)["bin_number"] for n in ("general_first", "quotients_odd", "three_bins")] == [63, 5, 3], "the odd counts"
    assert all(i == "lattice_blobs" for s, i in E.CASES if E.full_spec(s)["bin_number"] % 2), "odd bin counts on the lattice only"


@pytest.mark.parametrize("spec,inp", E.CASES, ids=["%s-%s" % c for c in E.CASES])
def test_no_point_the_gpu_test_compares_is_ambiguous(spec, inp):
    """No vote of any compared (spec, input) pair has angle / step within 1e-9 of a half-integer; every batch is small."""
    xy, off, _ = _scans(inp)
    nrm, info, amb = E.expected(spec, inp)
    assert len(xy) < 8000 and len(nrm) == len(info) == len(amb) == len(xy) == off[-1]
    assert not amb.any()
    assert info[:, 2].max() <= E.full_spec(spec)["bin_number"] // 2 < E.LIVE_BINS
    for a in (xy, off, nrm, info, amb):
        assert not a.flags.writeable


def test_odd_bin_counts_are_ambiguous_on_random_blobs_and_not_on_the_lattice():
    """Why the odd bin counts run on the lattice: a vote at exactly pi (nx rounds to -1 while ny > 0) has angle / step = B / 2,
    a half-integer when B is odd.  Random blobs have such pairs; the lattice, whose |dx| is 0 or at least 1/1024, has none."""
    xy, off, scans = _scans("dense_blobs")
    sl = scans[E.BLOB_LENGTHS.index(1057)]
    amb = R.estimate(xy[sl], np.array([0, 1057]), E.SPECS["three_bins"])[2]
    print("3 bins on the random blob of 1057 points: %d ambiguous" % amb.sum())
    assert amb.any()
    lxy, loff, _ = _scans("lattice_blobs")
    d = np.abs(lxy[:, None, 0] - lxy[None, :, 0])
    assert d[d > 0].min() >= 1.0 / 1024


def test_dense_blobs_fill_the_masks_and_the_sample_lists():
    xy, off, scans = _scans("dense_blobs")
    assert tuple(np.diff(off)) == E.BLOB_LENGTHS == (8, 9, 11, 12, 31, 32, 33, 1057, 1087, 1088, 1089)
    assert xy.dtype == np.float32 and np.isfinite(xy).all()
    assert [n % 32 for n in (1057, 1087, 1088)] == [1, 31, 0] and E.LDS_POINTS == 1088, "one bit, 31 bits, a full last word"
    assert 8 * 7 < E.LDS_TAKEN < 9 * 8 and 11 * 10 < E.MAX_TAKEN < 12 * 11
    for name in ("lds_full", "general_full", "quotients", "two_bins", "one_sample"):
        info = E.expected(name, "dense_blobs")[1]
        for n, sl in zip(E.BLOB_LENGTHS, scans):
            assert np.all(info[sl, 0] == n) and np.all(info[sl, 1] == 0), "m == n, no growth: every mask bit of the scan is set"
    for name, exhausted, least in (("lds_full", (8,), 9), ("general_full", (8, 11), 12)):
        info, limit = E.expected(name, "dense_blobs")[1], E.LIMITS[name]
        samples = info[:, 3] >> 16
        assert not E.stopped_early(info, name).any()
        for n, sl in zip(E.BLOB_LENGTHS, scans):
            if n in exhausted:
                assert np.all(samples[sl] == n * (n - 1)), "every ordered pair taken, through the redraw loop"
            elif n >= least:
                assert np.all(samples[sl] == limit), "the list is full"
        assert info[:, 2].max() == 32, "bin 32, the top live bin of B = 64, wins somewhere"
    one = E.expected("one_sample", "dense_blobs")[1]
    assert np.all(one[:, 3] >> 16 == 1) and np.all((one[:, 3] & 0xffff) <= 1)


@pytest.mark.parametrize("spec,inp", [("quotients", "dense_blobs"), ("quotients_odd", "lattice_blobs")])
def test_the_stop_rule_fires_on_integer_quotients_above_one(spec, inp):
    """With B = 4 or 5 and 128 samples `votes / B` runs well past 1: some points stop early with at least 2 B votes in the
    winning bin (at B = 32 the quotients are 0 or 1 only)."""
    info, B = E.expected(spec, inp)[1], E.full_spec(spec)["bin_number"]
    early = E.stopped_early(info, spec)
    votes = info[:, 3] & 0xffff
    print("%s: %d of %d points stop early, up to %d votes in the winning bin; %d run to the limit" % (
        spec, early.sum(), len(info), votes[early].max(), (~early).sum()))
    assert (early & (votes >= 2 * B)).any()
    assert (~early & (info[:, 2] >= 0)).any(), "and some run to their limit"


def test_lattice_blobs_are_exact_and_hold_duplicates():
    xy, off, scans = _scans("lattice_blobs")
    assert tuple(np.diff(off)) == E.LATTICE_LENGTHS == (9, 10, 33, 300, 1088, 1089)
    ij = (xy.astype(np.float64) - np.asarray(E.CENTRE)) * 1024
    assert np.array_equal(ij, np.rint(ij)) and ij.min() >= 0 and ij.max() <= 95, "the float coordinates are the lattice's, exactly"
    assert any(len(np.unique(xy[sl], axis=0)) < sl.stop - sl.start for sl in scans), "duplicates occur"
    for name in ("general_first", "quotients_odd", "three_bins"):
        info = E.expected(name, "lattice_blobs")[1]
        assert np.array_equal(info[:, 0], np.repeat(E.LATTICE_LENGTHS, E.LATTICE_LENGTHS)) and not info[:, 1].any()
    info = E.expected("general_first", "lattice_blobs")[1]
    assert np.all((info[:, 3] >> 16)[off[1]:] == 65), "65 samples on every scan of at least 10 points"


def test_the_grown_radius_is_strict():
    """At exactly the once-grown radius a point is not a neighbour, one ulp closer it is; and the list REBUILT at the grown
    radius leaves out a point at exactly that radius."""
    xy, off, _ = _scans("grown_edge")
    assert E.GROWN == np.float32(0.15 + 0.1) == np.float32(0.25) and off.tolist() == [0, 4, 7]
    assert xy[1, 0] == E.GROWN and xy[3, 0] == np.nextafter(E.GROWN, np.float32(0)) < E.GROWN
    info = E.expected("default", "grown_edge")[1]
    assert [tuple(r[:2]) for r in info[:4]] == [(2, 2), (2, 2), (2, 1), (2, 1)]
    # scan 1: point 0 stops growing at GROWN (0.2 < 0.25) and (0, 0.25) is at exactly GROWN from it
    pts = xy[4:7]
    d = np.sqrt((pts[0, 0] - pts[:, 0]) ** 2 + (pts[0, 1] - pts[:, 1]) ** 2)
    assert d.dtype == np.float32 and d[1] < E.GROWN and d[2] == E.GROWN
    assert [tuple(r[:2]) for r in info[4:7]] == [(2, 1), (2, 1), (3, 2)], "a `<=` at the rebuilt list would give point 0 three neighbours"


def test_tiny_pairs_vote_or_not_by_the_float_length():
    xy, off, scans = _scans("tiny_pairs")
    assert off.tolist() == [0, 11, 22] and E.TINY_ZERO + E.TINY_SUBNORMAL == 11
    tiny, off_diag = np.finfo(np.float32).tiny, ~np.eye(11, dtype=bool)
    for sl in scans:
        pts = xy[sl]
        assert len(np.unique(pts, axis=0)) == 11, "the points are distinct"
        dx, dy = pts[None, :, 0] - pts[:, None, 0], pts[None, :, 1] - pts[:, None, 1]
        sq = dx * dx + dy * dy
        assert sq.dtype == np.float32
        assert (sq[off_diag] == 0).sum() >= 12, "squared lengths that underflow to zero between distinct points"
        assert ((sq[off_diag] > 0) & (sq[off_diag] < tiny)).sum() >= 60, "squared lengths that are subnormal"
        assert sq.max() < 4 * tiny, "the longest pairs (4 and 5 steps of 3e-20) are just normal"
        assert (sq[off_diag] == np.float32(2.0 ** -149)).any(), "the smallest non-zero root there is, 2^-74.5"
    nrm, info, _ = E.expected("default", "tiny_pairs")
    votes, samples = info[:, 3] & 0xffff, info[:, 3] >> 16
    print("default spec: votes %s" % votes.tolist())
    assert np.all(info[:, 0] == 11) and np.all(samples == 49) and np.all(info[:, 2] == 3)
    assert votes[:11].min() >= 33 and votes[:11].max() <= 39, "scan 0: some samples cast no vote and some do"
    assert votes[11:].min() >= 30 and votes[11:].max() < 49
    for name in ("lds_full", "general_full", "two_bins"):
        i = E.expected(name, "tiny_pairs")[1]
        assert np.all(i[:, 0] == 11) and np.all((0 < (i[:, 3] & 0xffff)) & ((i[:, 3] & 0xffff) < (i[:, 3] >> 16)))
    # scan 1: of the pairs of the six closest points that have a length at all, some vote in the winning bin (their
    # directions are coarse: bins 3 and 4)
    six = xy[11:17]
    a, b = np.nonzero(~np.eye(6, dtype=bool))
    ok, _, _, bins = R.votes_of(six[a], six[b], 32)
    assert ok.sum() >= 4 and (bins[ok] == 3).sum() >= 2
    ok0, _, _, bins0 = R.votes_of(xy[a], xy[b], 32)
    assert ok0.sum() >= 4 and not np.any(bins0[ok0] == 3), "scan 0: the same pairs vote in a losing bin"


def test_many_scans_pass_65535():
    xy, off, _ = _scans("many_scans")
    lengths = np.diff(off)
    assert len(lengths) == E.MANY_SCANS == 65600 > 65536 and len(xy) == off[-1] < 3000
    assert 800 < (lengths > 0).sum() < 1000 and lengths.max() == 5 and lengths[lengths > 0].min() == 1
    assert all(lengths[s] > 0 for s in E.MANY_NON_EMPTY) and E.MANY_NON_EMPTY == (65535, 65536, 65599)
    info = E.expected("default", "many_scans")[1]
    assert (info[:, 2] >= 0).any() and (info[:, 1] > 0).any() and (info[:, 0] == 1).any()


def test_the_isolated_points_under_no_growth_and_long_growth():
    (xy, off), marks = E.isolated()
    assert off.tolist() == [0, 44] and sorted(marks.values()) == [40, 41, 42, 43]
    nrm, info, _ = E.expected("no_growth", "isolated")
    for k in marks.values():
        assert tuple(info[k]) == (1, 0, -1, 0) and not nrm[k].any()
    assert np.all(info[:40, 0] >= 2) and not info[:, 1].any()
    nrm, info, _ = E.expected("long_growth", "isolated")
    # 0.15 + k 0.001 summed in double: past 0.2 after 51 growths, past 0.3 after 151; 3.3 m takes more than 1024
    assert [tuple(info[marks[k]][:2]) for k in ("grow1", "grow2", "grow32", "never")] == [(2, 51), (2, 151), (1, 1024), (1, 1024)]
    assert nrm[marks["grow1"]].any() and not nrm[marks["grow32"]].any()
