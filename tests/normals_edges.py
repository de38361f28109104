"""Shared inputs of the scan-normal EDGE tests (tests/test_normals_edges_cpu.py holds their preconditions,
tests/test_normals_edges_gpu.py runs them): scans and specs that reach the capacities of nhip_normals.hip which depend on the
spec or on how dense a scan is, and the expectations by the numpy restatement (tests/normals_reference.py; DESIGN.md section 3,
"Scan normals"), computed once per process and read-only.

  dense_blobs()    n points uniform in a disc of radius 0.05 m: every mutual distance is below 0.15, so m = n for every point and
                   every word of its neighbour mask is full, or is the partial last one.  8 / 9 and 11 / 12 points: m (m - 1)
                   just below / above the sample limits 64 and 128; 1057, 1087, 1088: one bit, 31 bits, a full last word;
                   1089: the general kernel at m = 1089
  lattice_blobs()  points on a 1/1024 lattice (coordinate differences exact in float, duplicates occur): the inputs of the ODD
                   bin counts.  With an odd B a vote at exactly pi sits on a bin boundary (angle / step = B / 2); it comes from
                   a pair whose nx rounds to -1 while ny > 0, which random blobs have and a lattice (|dx| = 0 or >= 1/1024) has not
  grown_edge()     a pair at exactly the once-grown radius float(0.25) and one an ulp closer; and a point that reaches two
                   neighbours at the once-grown radius with a third point at exactly that radius (the list REBUILT there)
  tiny_pairs()     distinct points whose pairs have squared lengths that underflow to zero or are subnormal; the smallest
                   non-zero roots voting in a losing and in the winning bin
  many_scans()     65,600 scans, nearly all empty: the scan index at and past 65,535
  isolated()       the isolated-points scan of normals_reference.crafted_batch(), for the growth specs

SPECS names the specs, CASES the (spec, input) pairs the GPU test compares."""
import functools
import math

import numpy as np

from tests import normals_reference as R

F = np.float32
LDS_TAKEN, MAX_TAKEN, LDS_POINTS, LIVE_BINS = 64, 128, 1088, 34  # nhip_normals.hip: NORMALS_LDS_TAKEN, _MAX_TAKEN, _LDS_N, _BINS
CENTRE = (1.25, -0.75)
BLOB_LENGTHS = (8, 9, 11, 12, 31, 32, 33, 1057, 1087, 1088, 1089)
LATTICE_LENGTHS = (9, 10, 33, 300, 1088, 1089)
MANY_SCANS = 65600
MANY_NON_EMPTY = (65535, 65536, MANY_SCANS - 1)  # scans that have points by construction

SPECS = {
    "default": {},
    "lds_full": dict(mean_distance=0.0883, bin_number=64, seed=11),       # limit 64: the last row of the LDS taken list; bin 32
    "general_first": dict(mean_distance=0.0875, bin_number=63, seed=12),  # limit 65: short scans in the general kernel; odd B
    "general_full": dict(mean_distance=0.0625, bin_number=64, seed=13),   # limit 128: the last row of the private list
    "quotients": dict(mean_distance=0.0625, bin_number=4, seed=14),       # votes / B well above 1: the stop rule fires
    "quotients_odd": dict(mean_distance=0.0625, bin_number=5, seed=15),
    "two_bins": dict(bin_number=2, seed=16),
    "three_bins": dict(bin_number=3, seed=17),
    "one_sample": dict(mean_distance=0.70, seed=18),                      # limit 1
    "no_growth": dict(max_growth_steps=0, seed=19),
    "long_growth": dict(max_growth_steps=1024, neighborhood_step_size=0.001, seed=20),
}
LIMITS = {"lds_full": 64, "general_first": 65, "general_full": 128, "one_sample": 1}
CASES = [("lds_full", "dense_blobs"), ("lds_full", "tiny_pairs"), ("general_first", "lattice_blobs"),
         ("general_full", "dense_blobs"), ("general_full", "tiny_pairs"), ("quotients", "dense_blobs"),
         ("quotients_odd", "lattice_blobs"), ("two_bins", "dense_blobs"), ("two_bins", "tiny_pairs"),
         ("three_bins", "lattice_blobs"), ("one_sample", "dense_blobs"), ("default", "grown_edge"), ("default", "tiny_pairs"),
         ("default", "many_scans"), ("no_growth", "isolated"), ("long_growth", "isolated")]


def full_spec(name):
    """SPECS[name] over the defaults."""
    return dict(R.DEFAULTS, **SPECS[name])


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def _packed(scans):
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int32)
    xy = np.concatenate([np.asarray(s, F).reshape(-1, 2) for s in scans]) if len(scans) else np.zeros((0, 2), F)
    return _frozen(np.ascontiguousarray(xy, F), offsets)


@functools.lru_cache(maxsize=None)
def dense_blobs():
    """(xy, offsets): one scan per BLOB_LENGTHS."""
    rng = np.random.default_rng(20261)
    scans = []
    for n in BLOB_LENGTHS:
        rad, phi = 0.05 * np.sqrt(rng.uniform(0.0, 1.0, n)), rng.uniform(0.0, 2.0 * math.pi, n)
        scans.append(np.stack([CENTRE[0] + rad * np.cos(phi), CENTRE[1] + rad * np.sin(phi)], axis=1).astype(F))
    return _packed(scans)


@functools.lru_cache(maxsize=None)
def lattice_blobs():
    """(xy, offsets): one scan per LATTICE_LENGTHS, points (i, j) / 1024 + CENTRE with i, j random in 0 .. 95."""
    rng = np.random.default_rng(20262)
    scans = []
    for n in LATTICE_LENGTHS:
        ij = rng.integers(0, 96, (n, 2))
        scans.append((np.asarray(CENTRE, np.float64) + ij / 1024.0).astype(F))
    return _packed(scans)


GROWN = F(0.25)  # (float)(0.15 + 0.1): the radius after one growth


@functools.lru_cache(maxsize=None)
def grown_edge():
    """(xy, offsets), two scans.  Scan 0: a pair at exactly GROWN -- no neighbours until the radius has grown twice -- and a
    pair one ulp closer: neighbours after one growth.  Scan 1: (0, 0) has (0.2, 0) inside the once-grown radius, so it stops
    growing there, and (0, 0.25) at exactly that radius: the list rebuilt at GROWN must leave it out."""
    pair = np.array([[0.0, 0.0], [GROWN, 0.0], [0.0, 5.0], [np.nextafter(GROWN, F(0)), 5.0]], F)
    rebuilt = np.array([[0.0, 0.0], [0.2, 0.0], [0.0, GROWN]], F)
    return _packed([pair, rebuilt])


TINY_ZERO, TINY_SUBNORMAL = 6, 5


@functools.lru_cache(maxsize=None)
def tiny_pairs():
    """(xy, offsets), two scans of 11 distinct points.  Scan 0: six points k 1e-23 (0.8, 0.6), k = 0 .. 5, whose pairs have
    squared lengths that underflow (most of them to zero), and five at k 3e-20 (-0.6, 0.8), k = 1 .. 5, whose pairs have
    subnormal squared lengths.  Oblique on purpose: an axis-parallel cluster votes at exactly pi / 2, a bin boundary for B = 2.
    Scan 1: the same with the six along (-0.6, 0.8) too, so that their pairs of one or two ulps of squared length -- the
    smallest roots there are -- vote in the winning bin, where the info words see them."""
    k6, k5 = np.arange(TINY_ZERO)[:, None], np.arange(1, TINY_SUBNORMAL + 1)[:, None]
    b = k5 * 3e-20 * np.array([[-0.6, 0.8]])
    return _packed([np.concatenate([k6 * 1e-23 * np.array([[0.8, 0.6]]), b]).astype(F),
                    np.concatenate([k6 * 1e-23 * np.array([[-0.6, 0.8]]), b]).astype(F)])


@functools.lru_cache(maxsize=None)
def many_scans():
    """(xy, offsets): MANY_SCANS scans; about 900 at random places, and those of MANY_NON_EMPTY, have 1 .. 5 points in a box of
    0.4 m, the rest none."""
    rng = np.random.default_rng(20265)
    lengths = np.zeros(MANY_SCANS, np.int64)
    some = np.unique(np.concatenate([rng.integers(0, MANY_SCANS, 900), MANY_NON_EMPTY]))
    lengths[some] = rng.integers(1, 6, len(some))
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    xy = (rng.uniform(-3.0, 3.0, (MANY_SCANS, 2))[np.repeat(np.arange(MANY_SCANS), lengths)]
          + rng.uniform(-0.2, 0.2, (int(offsets[-1]), 2))).astype(F)
    return _frozen(xy, offsets)


@functools.lru_cache(maxsize=None)
def isolated():
    """((xy, offsets), marks): the scan of crafted_batch() that holds its isolated points (a wall of 40 points and four points
    0.2, 0.3, 3.3 and 85 m from their nearest other point); marks: name -> index in the scan."""
    xy, off, marks = R.crafted_batch()
    s = int(np.searchsorted(off, marks["grow1"], side="right") - 1)
    names = ("grow1", "grow2", "grow32", "never")
    assert all(off[s] <= marks[k] < off[s + 1] for k in names)
    return _packed([xy[off[s]:off[s + 1]]]), {k: int(marks[k] - off[s]) for k in names}


INPUTS = {"dense_blobs": dense_blobs, "lattice_blobs": lattice_blobs, "grown_edge": grown_edge, "tiny_pairs": tiny_pairs,
          "many_scans": many_scans, "isolated": lambda: isolated()[0]}


@functools.lru_cache(maxsize=None)
def expected(spec_name, input_name):
    """(normals, info, ambiguous) of INPUTS[input_name]() under SPECS[spec_name] by the restatement; computed once per process
    and shared, read-only."""
    xy, off = INPUTS[input_name]()
    return _frozen(*R.estimate(xy, off, SPECS[spec_name]))


def stopped_early(info, spec_name):
    """Which points the stop rule ended: fewer samples counted than min(m (m - 1), the spec's limit)."""
    m = info[:, 0].astype(np.int64)
    limit = np.minimum(m * (m - 1), R.sample_limit(full_spec(spec_name)["mean_distance"]))
    return (info[:, 2] >= 0) & ((info[:, 3] >> 16) < limit)
