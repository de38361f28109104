"""Shared inputs of the drop-in call's SEAM tests (tests/test_dropin_seams_cpu.py holds their preconditions,
tests/test_dropin_seams_gpu.py runs them): calls of CorrelativeScanMatcher.GetTransformation that put every flow of
nhip_csm_get_transformation (nhip_dropin.hip) and the values host and device hand each other on a designed input, and what
the CPU oracle gives for them (oracle.two_level_match, the independent restatement of the two-level search; the coarse
level's record by oracle.csm_match), computed once per case and read-only.

The flow a call takes follows from its constructor and its restriction alone; flow() restates the rules from the constants
of the library (the tests of the CPU file hold them against the sources):

  coarse lattice   n_theta1 = 2 floor(restriction / 1 deg) + 1 rotations of side1 x side1 translations, side1 = 2 h1 + 1,
                   h1 = floor(trans_range / low_res).  side1^2 <= 256 (64 lanes x SMALL_PASSES = 4 poses): the kernel whose
                   lanes are poses ("poses").  Else side1 <= 21: every add is asked for, the strip kernels ("strips").  Else
                   branch and bound ("bnb") where the lattice is inside its envelope (ceil(side1 / 8) <= 11 blocks per axis,
                   n_theta1 <= 340), the strip kernels beyond it.  Branch and bound of more than 8 rotations is DEALT over the
                   fewest parts q = 2 .. 8 whose ceil(n_theta1 / q) is odd and at most 8.
  fine lattice     21 rotations of side2 x side2, side2 = 2 ratio + 1, ratio = lround(low_res / high_res): side2^2 <= 256
                   the kernel whose lanes are poses in one tile, side2 <= 256 and 21 * ceil(side2 / floor(256 / side2)) <= 2048
                   the same kernel in tiles of rows (fine_form 2 either way), else the strip kernels (fine_form 1).
  cacheable        reach_max = lround(h1 * low_res / high_res) + ratio + 2 <= 4096 and a target that is not empty.
  chained          cacheable, at most DROPIN_CHAIN_ROT_MAX = 512 coarse rotations, a coarse search in one part.
  fused            chained with both levels "poses": the bridge kernel decodes the coarse key and zeroes the fine keys.

Constructors (scanner_range, trans_range, low_res, high_res) and the flow each is here for:

  WALK     (10, 1, 0.25, 0.1)      9 x 9 coarse, 7 x 7 fine: chained and fused.  low_res / high_res = 2.5: ratio = lround(2.5),
                                   and the coarse translations +-0.25, +-0.75 are exact halves +-2.5, +-7.5 of high_res
  STRIPS   (10, 1, 0.125, 0.05)    17 x 17 coarse in the strip kernels, 7 x 7 fine in the small-plane kernel: chained, not fused
  BNB1     (10, 1.5, 0.125, 0.05)  25 x 25 coarse: branch and bound; at most 8 rotations below 4 deg: ONE part, chained
  DEFAULT  (30, 2, 0.3, 0.01)      13 x 13 coarse, 61 x 61 fine in tiles of rows: chained and fused
  ROT      (10, 3, 0.125, 0.05)    49 x 49 coarse: branch and bound; 41 rotations at 20 deg: 6 parts of 7 (one copy of the last
                                   rotation behind the table), one level after the other; 7 rotations at 3 deg: one part, chained
  NOCACHE  (2, 8.1, 0.21, 0.002)  h1 = 38, ratio = 105, reach_max = 3990 + 105 + 2 = 4097 > 4096: not cacheable, one level after
                                   the other, the fine table built for the call's own coarse optimum -- in the lattice's corner
                                   with max_shift = 3990 + 105 = 4095, inside the 4096 a grid spec admits.  77 x 77 coarse by
                                   branch and bound in one part, 211 x 211 fine in the strip kernels.  (The oracle takes 0.3 s
                                   for a call of it; (3, 4.8, 0.1, 0.00119) -- h1 = floor(47.99..) = 47, reach_max 4036 -- IS
                                   cacheable and took 2 .. 3.4 s, (1, 4.1, 0.1, 0.001) 0.5 s.)
  REFUSED  (2, 8.2, 0.2, 0.002)    h1 = 40, ratio = 100: in the corner max_shift would be 4100, which make_layout refuses
                                   ("max_shift out of range"): the call fails with that error, it returns no wrong pose

Families (Cases by what they are designed for, built once):

  translation_walk(ctor, bits)   the target against itself shifted by (i, j) * low_res: the transform is MINUS the shift.
                                 WALK: every i, j in -h1 - 1 .. h1 + 1 (121 calls); the outermost ring lies beyond the lattice
                                 and the coarse optimum clamps to its border, where the fine search runs at the farthest
                                 centre the cached fine table was sized for.  Other constructors: ring(h1), the 4 corners and
                                 4 edge midpoints of that outermost ring
  rotation_walk(bits)            ROT at 20 deg, the target against itself rotated by -k deg, k = -21 .. 21: the coarse winner is
                                 rotation k + 20 -- every rotation of every part, the first and the last of each, the last of
                                 the table (k = 20: its copy in part 5 ties and must lose) -- and 0 / 40 beyond the range;
                                 "empty": a source without points, every pose of every part ties and rotation 0 wins
  rotation_counts()              WALK at restrictions 0, 0.5, 255.5, 256.5 deg and 2 pi: 1, 1, 511, 513, 721 coarse rotations
  angle_wraps()                  WALK at 3 deg, (rot_a, rot_b) whose difference is at or beyond +-pi, the source turned so that
                                 the match is at the lattice's centre; and one call at 5 deg whose coarse winner's angle
                                 theta0 + k * 1 deg lies beyond +pi
  length_sequence(ctor)          sources of 2049, 7, 2048, 1089, 1088, 1, 0, 5000, 64 points (cuts of concatenated scans), the
                                 restriction alternating 3 / 20 deg: the thread's scratch grows at 2049 (2048 points are its
                                 first size) and 5000 and keeps old points behind every shorter cloud, the kept rotation table
                                 (7 / 41 rotations) is replaced and replaced back, NHIP_SEARCH_SHORT_SCANS is set at 1088 and
                                 below.  ROT alternates one part, chained (3 deg) with six parts (20 deg)
  non_cacheable(ctor)            NOCACHE, REFUSED: a target against itself, and against itself shifted to the (-, -) corner
  cache_targets()                three small targets and one source for the cache-order test (WALK)

Points beyond scanner_range are outside the tables for the oracle and the library alike; SynthBag scans reach 30 m, the thinned
target keeps ~290 of its ~360 points within 10 m."""
import collections
import functools
import math

import numpy as np

from nautilus_amd import synth
from oracle import oracle as O

F = np.float32
DEG = math.pi / 180.0          # coarse_step of nhip_csm_get_transformation; the fine step is a tenth of it
SMALL_LANES_X_PASSES = 256     # nhip_csm_small.hip: 64 * SMALL_PASSES poses of one workgroup
EXHAUSTIVE_SIDE_MAX = 21       # nhip_dropin.hip: (2 * h1 + 1) <= 21 ? NHIP_SEARCH_EXHAUSTIVE : 0
BNB_BLOCK, BNB_BLOCKS_MAX, BNB_ROT_MAX = 8, 11, 340   # BNB_B, NB = BNB_MAX_NB, MAX_ROT
PART_ROT_MAX, PARTS_MAX = 8, 8  # rotations a part holds; DROPIN_PARTS_MAX
CHAIN_ROT_MAX = 512            # DROPIN_CHAIN_ROT_MAX
REACH_CACHE_MAX = 4096         # cacheable = reach_max <= 4096 && n_b > 0
TILED_BLOCKS_MAX = 2048        # SMALL_TILED_MAX_BLOCKS
SCRATCH_FIRST = 2048           # scratch_for: the first capacity of the thread's cloud buffer
SHORT_SCAN = 1088              # NHIP_SHORT_SCAN_POINTS

WALK = (10.0, 1.0, 0.25, 0.1)
STRIPS = (10.0, 1.0, 0.125, 0.05)
BNB1 = (10.0, 1.5, 0.125, 0.05)
DEFAULT = (30.0, 2.0, 0.3, 0.01)
ROT = (10.0, 3.0, 0.125, 0.05)
NOCACHE = (2.0, 8.1, 0.21, 0.002)
REFUSED = (2.0, 8.2, 0.2, 0.002)
MAX_SHIFT_MAX = 4096           # make_layout: spec->max_shift <= 4096

LENGTHS = (2049, 7, 2048, 1089, 1088, 1, 0, 5000, 64)
ROTATION_COUNTS = ((0.0, 1, True), (0.5, 1, True), (255.5, 511, True), (256.5, 513, False), (360.0, 721, False))
WRAP_PAIRS = ((3.0, -3.0), (-3.0, 3.0), (math.pi, 0.0), (0.0, math.pi), (7.0, 0.5), (math.pi - 1e-9, -1e-9))

Case = collections.namedtuple("Case", "name ctor bits a b rot_a rot_b restriction")
Flow = collections.namedtuple("Flow", "h1 side1 n_theta1 coarse parts per ratio side2 fine_form reach_max cacheable chained fused")


def lround(x):
    """C's lround: halves away from zero."""
    return int(math.floor(abs(x) + 0.5)) * (1 if x >= 0 else -1)


def n_theta_of(restriction):
    return 2 * int(math.floor(restriction / DEG)) + 1


def flow(ctor, restriction, n_b=1):
    """The flow nhip_csm_get_transformation takes for this constructor and restriction (radians), restated from csm_plan,
    DropInLevel and the `chained` condition (see the top of the file)."""
    _, trans, low, high = ctor
    h1 = int(math.floor(trans / low))
    side1, n1 = 2 * h1 + 1, n_theta_of(restriction)
    blocks = -(-side1 // BNB_BLOCK)
    if side1 * side1 <= SMALL_LANES_X_PASSES:
        coarse = "poses"
    elif side1 <= EXHAUSTIVE_SIDE_MAX or blocks > BNB_BLOCKS_MAX or n1 > BNB_ROT_MAX:
        coarse = "strips"
    else:
        coarse = "bnb"
    parts, per = 1, n1
    if coarse == "bnb" and n1 > PART_ROT_MAX:
        for q in range(2, PARTS_MAX + 1):
            r = -(-n1 // q)
            if r & 1 and r <= PART_ROT_MAX:
                parts, per = q, r
                break
    ratio = lround(low / high)
    side2 = 2 * ratio + 1
    if side2 * side2 <= SMALL_LANES_X_PASSES:
        fine_form = 2
    elif side2 <= SMALL_LANES_X_PASSES and 21 * -(-side2 // min(side2, SMALL_LANES_X_PASSES // side2)) <= TILED_BLOCKS_MAX:
        fine_form = 2
    else:
        fine_form = 1
    reach_max = lround(h1 * low / high) + ratio + 2
    cacheable = reach_max <= REACH_CACHE_MAX and n_b > 0
    chained = cacheable and n1 <= CHAIN_ROT_MAX and parts == 1
    return Flow(h1, side1, n1, coarse, parts, per, ratio, side2, fine_form, reach_max, cacheable, chained,
                chained and coarse == "poses" and fine_form == 2)


def flow_of(case):
    return flow(case.ctor, case.restriction, len(case.b))


def _frozen(a):
    a = np.ascontiguousarray(a, dtype=F).reshape(-1, 2)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def bag():
    """The suite's SynthBag(48) (conftest.py's small_bag holds the same scans)."""
    return synth.SynthBag(48)


@functools.lru_cache(maxsize=None)
def target():
    return _frozen(bag().scans[15][::3])


def shifted(p, dx, dy):
    return _frozen(p + np.array([dx, dy], F))


def rotated(p, angle):
    c, s = math.cos(angle), math.sin(angle)
    return _frozen(np.stack([c * p[:, 0] - s * p[:, 1], s * p[:, 0] + c * p[:, 1]], axis=1))


def ring(h1):
    """The 4 corners and 4 edge midpoints of the ring just beyond a lattice of half-width h1."""
    r = h1 + 1
    return tuple((i, j) for i in (-r, 0, r) for j in (-r, 0, r) if (i, j) != (0, 0))


@functools.lru_cache(maxsize=None)
def translation_walk(ctor=WALK, bits=16, full=True):
    """{(i, j): Case}: the target against itself shifted by (i, j) * low_res, at a 3 degree restriction."""
    h1, low = flow(ctor, 3 * DEG).h1, ctor[2]
    ij = [(i, j) for i in range(-h1 - 1, h1 + 2) for j in range(-h1 - 1, h1 + 2)] if full else ring(h1)
    return {(i, j): Case("walk%s/%d/%+d%+d" % (ctor, bits, i, j), ctor, bits, shifted(target(), i * low, j * low), target(), 0.0, 0.0,
                         3 * DEG) for i, j in ij}


@functools.lru_cache(maxsize=None)
def rotation_walk(bits=16):
    """{k: Case}, k = -21 .. 21: the target against itself rotated by -k degrees, ROT at 20 degrees; {"empty": Case}."""
    out = {k: Case("rot/%d/%+d" % (bits, k), ROT, bits, rotated(target(), -k * DEG), target(), 0.0, 0.0, 20 * DEG)
           for k in range(-21, 22)}
    out["empty"] = Case("rot/%d/empty" % bits, ROT, bits, _frozen(np.zeros((0, 2))), target(), 0.0, 0.0, 20 * DEG)
    return out


@functools.lru_cache(maxsize=None)
def rotation_counts():
    """((Case, coarse rotations, chained), ...): half-degree restrictions, so that floor(restriction / 1 deg) does not hang
    on the last bit of the conversion to radians."""
    b = bag()
    a, rot_a, rot_b = _frozen(b.scans[17][::3]), float(b.odom[17, 2]), float(b.odom[15, 2])
    return tuple((Case("count/%g" % deg, WALK, 16, a, target(), rot_a, rot_b, 2 * math.pi if deg == 360.0 else math.radians(deg)),
                  n, chained) for deg, n, chained in ROTATION_COUNTS)


def angle_diff(rot_a, rot_b):
    """math_util.h:81-89 as the call and the oracle compute it."""
    d = rot_a - rot_b
    return d - 2.0 * math.pi * float(np.rint(d / (2.0 * math.pi)))


@functools.lru_cache(maxsize=None)
def angle_wraps():
    """{(rot_a, rot_b): Case} of WRAP_PAIRS, the source turned by minus their difference (the match is at the centre of the
    coarse lattice), and {"beyond": Case}: theta0 = 3.13 (179.3 degrees), the source turned by -182 degrees, a 5 degree
    restriction -- the coarse winner's angle 3.13 + (2 or 3) * 1 deg lies beyond +pi."""
    out = {(ra, rb): Case("wrap/%r/%r" % (ra, rb), WALK, 16, rotated(target(), -angle_diff(ra, rb)), target(), ra, rb, 3 * DEG)
           for ra, rb in WRAP_PAIRS}
    out["beyond"] = Case("wrap/beyond", WALK, 16, rotated(target(), -182 * DEG), target(), 3.13, 0.0, 5 * DEG)
    return out


@functools.lru_cache(maxsize=None)
def length_sequence(ctor=WALK, bits=16):
    """The calls of one thread, in order: sources of LENGTHS points cut from six concatenated scans (each cut starts 11
    points after the last), one target, the restriction alternating 3 / 20 degrees."""
    b = bag()
    pool = np.concatenate([b.scans[i] for i in (3, 4, 5, 6, 7, 8)])
    assert len(pool) >= max(LENGTHS) + 11 * len(LENGTHS)
    tgt = _frozen(b.scans[8][::3])
    return tuple(Case("len%s/%d/%d" % (ctor, bits, n), ctor, bits, _frozen(pool[11 * i:11 * i + n]), tgt, 0.02, -0.01, (3, 20)[i & 1] * DEG)
                 for i, n in enumerate(LENGTHS))


@functools.lru_cache(maxsize=None)
def non_cacheable(ctor=NOCACHE):
    """{"match", "corner"}: a tenth-scale target (within 3 m) against itself and against itself shifted by +h1 * low_res on
    both axes -- the coarse optimum in the (-, -) corner, the fine table built with max_shift = h1 * low_res / high_res + ratio
    exactly."""
    b = _frozen(target() * F(0.1))
    h1, low = flow(ctor, DEG).h1, ctor[2]
    return {"match": Case("nocache%s/match" % (ctor,), ctor, 16, b, b, 0.0, 0.0, DEG),
            "corner": Case("nocache%s/corner" % (ctor,), ctor, 16, shifted(b, h1 * low, h1 * low), b, 0.0, 0.0, DEG)}


@functools.lru_cache(maxsize=None)
def cache_targets():
    """{"A", "B", "C"}: Case of one source against three targets (WALK, 3 degrees)."""
    b = bag()
    a = _frozen(b.scans[17][::3])
    return {name: Case("cache/" + name, WALK, 16, a, _frozen(b.scans[i][::3]), float(b.odom[17, 2]), float(b.odom[i, 2]), 3 * DEG)
            for name, i in (("A", 15), ("B", 22), ("C", 30))}


_WANT, _COARSE = {}, {}


def want(case):
    """(score, ((tx, ty), theta)) of the oracle's two-level search for this case; computed once."""
    if case.name not in _WANT:
        _WANT[case.name] = O.two_level_match(case.a, case.b, case.rot_a, case.rot_b, case.restriction, *case.ctor, cell_bits=case.bits)
    return _WANT[case.name]


def coarse(case):
    """(itheta, ix, iy, score as float32) of the oracle's coarse level for this case; computed once."""
    if case.name not in _COARSE:
        f = flow_of(case)
        gs = O.grid_spec(case.ctor[0], case.ctor[2], 2.0, 1e-10, case.bits)
        m = O.csm_match(case.a, O.grid_build(case.b, gs), gs, angle_diff(case.rot_a, case.rot_b),
                        O.search_spec(f.n_theta1, f.side1, f.side1, DEG))
        _COARSE[case.name] = (m.itheta, m.ix, m.iy, F(m.score))
    return _COARSE[case.name]

