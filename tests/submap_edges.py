"""Shared inputs of the submap EDGE tests (tests/test_submap_edges_cpu.py holds their preconditions, tests/test_submap_edges_gpu.py
runs them): member lists that make every input-dependent loop of nhip_submap.hip run more than once, and the merged clouds by the
numpy restatement of the spec (hostside.submap_clouds; DESIGN.md section 3, "Submaps"), computed once and read-only.

The MINI BAG: short scans of MINI_LENGTHS points (seeded generator, a few metres), one of 1081, one of 65,535 and one of 65,536
points -- the last two only ever COUNTED (the totals beyond int32), never gathered.  Member affines are random small angles.

  many_members()    one target of 900 members: the member-batch loop (256 members at a time), a whole batch without points,
                    members without points on either side of the 256 seam; a second target so the target seam is inside a chunk
  many_targets()    2,500 targets of 0 .. 2 short members: the offsets kernel's steps of 1024 and their carry, runs of empty
                    targets at the ends and across a step seam, hundreds of targets inside one gather chunk
  grid_stride()     400 targets x 10 members of the 1081-point scan: 4,324,000 points, the smallest cloud at which a gather
                    workgroup takes a second chunk (more than 2048 workgroups x 2048 points)
  beyond_int32()    four member lists whose totals are 2^32 + 1081 (twice), 2^31 and 2^31 - 1: refused, nothing stored
  numeric()         one scan of every pair of special floats plus random exponents under 48 special / extreme affines:
                    subnormal results, signed zeros, overflow from finite inputs, inf x 0

An ACCEPTED cloud near 2^31 points needs a 17 GB buffer and is not tested."""
import functools

import numpy as np

from nautilus_amd import hostside

GATHER_THREADS, GATHER_CHUNK, GATHER_MAX_GRID = 256, 2048, 2048  # nhip_submap.hip: SUB_T, SUB_CHUNK, SUB_MAX_GRID
OFFSETS_STEP = 1024                                              # targets per step of submap_offsets_kernel
MINI_LENGTHS = [0, 1, 2, 3, 5, 8, 13, 21, 34, 40, 64, 1081, 65535, 65536]
EMPTY, S1081, S65535, S65536 = 0, 11, 12, 13                     # scans of the mini bag by what they are used for
INT32_MAX = 2 ** 31 - 1


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def _small_angle_affines(rng, n):
    th = rng.uniform(-0.1, 0.1, n)
    return np.stack([np.cos(th), np.sin(th), rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n)], axis=1).astype(np.float32)


def _lists(lists):
    """(member_scan int32, member_offsets int32) of a list of member lists."""
    member_scan = np.array([m for t in lists for m in t], dtype=np.int32)
    member_offsets = np.concatenate([[0], np.cumsum([len(t) for t in lists])]).astype(np.int32)
    return member_scan, member_offsets


@functools.lru_cache(maxsize=None)
def mini_packed():
    """(xy, offsets) of the mini bag."""
    rng = np.random.default_rng(20241018)
    offsets = np.concatenate([[0], np.cumsum(MINI_LENGTHS)]).astype(np.int32)
    xy = rng.uniform(-4.0, 4.0, (int(offsets[-1]), 2)).astype(np.float32)
    return _frozen(xy, offsets)


def restate(packed, members):
    """(xy, offsets) of the members' merged clouds by the restatement, read-only."""
    return _frozen(*hostside.submap_clouds(*packed, *members))


# ---------------------------------------------------------------------------------------------- 1. many members
MANY_MEMBERS = 900
EMPTY_BATCH = (256, 512)  # members [256, 512): the whole second batch is the 0-point scan
EMPTY_SEAMS = (255, 512)  # ... and so are the last member of batch 0 and the first of batch 2


@functools.lru_cache(maxsize=None)
def many_members():
    """(member_scan, member_affine, member_offsets): target 0 of 900 members drawn from the scans of 1 .. 40 points, target 1
    of four (one of them empty, one of 1081 points)."""
    rng = np.random.default_rng(7)
    first = rng.choice(np.arange(1, 10), MANY_MEMBERS, p=[0.04, 0.04, 0.04, 0.08, 0.1, 0.15, 0.2, 0.2, 0.15])
    first[EMPTY_BATCH[0]:EMPTY_BATCH[1]] = EMPTY
    first[list(EMPTY_SEAMS)] = EMPTY
    member_scan, member_offsets = _lists([first.tolist(), [10, EMPTY, 9, S1081]])
    return _frozen(member_scan, _small_angle_affines(rng, len(member_scan)), member_offsets)


@functools.lru_cache(maxsize=None)
def many_members_merged():
    return restate(mini_packed(), many_members())


def member_starts(member_scan, lengths=MINI_LENGTHS):
    """Output index of every member's first point, and the total (n_members + 1 entries; ids in range)."""
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64)[np.asarray(member_scan)])])


@functools.lru_cache(maxsize=None)
def many_members_bad_ids():
    """many_members() with one member of the third batch (600) replaced by -1 and one of the fourth (800) by n_scans:
    ((members), (first, second)).  Both replaced members had points."""
    member_scan, aff, moff = many_members()
    bad = member_scan.copy()
    first, second = 600, 800
    assert MINI_LENGTHS[bad[first]] > 0 and MINI_LENGTHS[bad[second]] > 0
    bad[first], bad[second] = -1, len(MINI_LENGTHS)
    return (_frozen(bad), aff, moff), (first, second)


# ---------------------------------------------------------------------------------------------- 2. many targets
MANY_TARGETS = 2500
EMPTY_TARGETS = [(0, 5), (1000, 2100), (MANY_TARGETS - 7, MANY_TARGETS)]  # [from, to) runs of targets without members


@functools.lru_cache(maxsize=None)
def many_targets():
    """2,500 targets (steps of 1024, 1024 and 452) of 0 .. 2 members drawn from the scans of 0 .. 8 points."""
    rng = np.random.default_rng(11)
    counts = rng.choice([0, 1, 2], MANY_TARGETS, p=[0.1, 0.35, 0.55])
    for a, b in EMPTY_TARGETS:
        counts[a:b] = 0
    lists = [rng.integers(0, 6, c).tolist() for c in counts]
    member_scan, member_offsets = _lists(lists)
    return _frozen(member_scan, _small_angle_affines(rng, len(member_scan)), member_offsets)


@functools.lru_cache(maxsize=None)
def many_targets_merged():
    return restate(mini_packed(), many_targets())


def first_targets(members, n):
    """The member lists of the first n targets."""
    member_scan, aff, moff = members
    return member_scan[:moff[n]], aff[:moff[n]], moff[:n + 1]


# ---------------------------------------------------------------------------------------------- 3. grid stride
STRIDE_TARGETS, STRIDE_MEMBERS = 400, 10


@functools.lru_cache(maxsize=None)
def grid_stride():
    rng = np.random.default_rng(13)
    member_scan, member_offsets = _lists([[S1081] * STRIDE_MEMBERS] * STRIDE_TARGETS)
    return _frozen(member_scan, _small_angle_affines(rng, len(member_scan)), member_offsets)


@functools.lru_cache(maxsize=None)
def grid_stride_merged():
    return restate(mini_packed(), grid_stride())


# ---------------------------------------------------------------------------------------------- 4. totals beyond int32
BEYOND_CAPACITY = 4096
BEYOND_CASES = ["a", "b", "c", "d"]


@functools.lru_cache(maxsize=None)
def beyond_int32(case):
    """((member_scan, member_affine, member_offsets), total, the value the status words must carry)."""
    if case == "a":    # one target; the total wraps to 1081 <= capacity in 32 bits
        lists, total = [[S65536] * 65536 + [S1081]], 2 ** 32 + 1081
    elif case == "b":  # 2,048 targets; the running sum is 2^31 exactly at the step seam (target 1024)
        lists, total = [[S65536] * 32] * 2047 + [[S65536] * 32 + [S1081]], 2 ** 32 + 1081
    elif case == "c":  # negative as int32
        lists, total = [[S65536] * 32768], 2 ** 31
    elif case == "d":  # fits int32, exceeds the capacity: reported unclamped
        lists, total = [[S65536] * 32767 + [S65535]], 2 ** 31 - 1
    else:
        raise KeyError(case)
    member_scan, member_offsets = _lists(lists)
    aff = np.tile(np.float32([1, 0, 0, 0]), (len(member_scan), 1))
    return _frozen(member_scan, aff, member_offsets), total, min(total, INT32_MAX)


# ---------------------------------------------------------------------------------------------- 5. zero capacity, zero targets
@functools.lru_cache(maxsize=None)
def empty_members():
    """Three targets whose members are all the 0-point scan (the middle one has no member at all)."""
    member_scan, member_offsets = _lists([[EMPTY, EMPTY], [], [EMPTY, EMPTY, EMPTY]])
    return _frozen(member_scan, np.tile(np.float32([1, 0, 0, 0]), (len(member_scan), 1)), member_offsets)


# ---------------------------------------------------------------------------------------------- 6. numeric edges
F = np.float32
FLT_MIN, FLT_MAX, DENORM_MIN = np.finfo(F).tiny, np.finfo(F).max, F(2.0 ** -149)
_POSITIVE = [F(0.0), DENORM_MIN, F(1e-39), FLT_MIN, F(1.0), F(3e38), FLT_MAX, F(np.inf)]
SPECIALS = np.array([v for p in _POSITIVE for v in (p, -p)] + [np.nan], dtype=F)  # 17 values
NUMERIC_MEMBERS = 48


def _random_exponents(rng, shape, lo=-149, hi=127):
    """Floats of random sign, mantissa and exponent lo .. hi (subnormals below -126), as float32."""
    e = rng.integers(lo, hi + 1, shape)
    return (rng.choice([-1.0, 1.0], shape) * rng.uniform(1.0, 2.0, shape) * 2.0 ** e.astype(np.float64)).astype(F)


@functools.lru_cache(maxsize=None)
def numeric_packed():
    """(xy, offsets): ONE scan -- every pair of SPECIALS, then 2,000 points of random exponents."""
    rng = np.random.default_rng(17)
    pairs = np.stack(np.meshgrid(SPECIALS, SPECIALS, indexing="ij"), axis=-1).reshape(-1, 2)
    xy = np.concatenate([pairs, _random_exponents(rng, (2000, 2))]).astype(F)
    return _frozen(xy, np.array([0, len(xy)], dtype=np.int32))


@functools.lru_cache(maxsize=None)
def numeric():
    """One target of 48 members of the numeric scan: 17 affines that take every special value in every slot, the rows
    (1, 0, 0, 0), (0, 1, 0, 0) and (-0, -1, -0, 0), ten with c and s in 2^+-30 and a translation of zeros of either sign, 18
    of random exponents."""
    rng = np.random.default_rng(19)
    k = np.arange(len(SPECIALS))
    special = np.stack([SPECIALS[(k + 4 * j) % len(SPECIALS)] for j in range(4)], axis=1)
    rows = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [-0.0, -1, -0.0, 0]], dtype=F)
    big = np.concatenate([_random_exponents(rng, (10, 2), -30, 30), np.tile(F([[0.0, -0.0], [-0.0, -0.0]]), (5, 1))], axis=1)
    rest = _random_exponents(rng, (NUMERIC_MEMBERS - len(special) - len(rows) - len(big), 4))
    aff = np.concatenate([special, rows, big, rest]).astype(F)
    assert aff.shape == (NUMERIC_MEMBERS, 4)
    member_scan, member_offsets = _lists([[0] * NUMERIC_MEMBERS])
    return _frozen(member_scan, aff, member_offsets)


@functools.lru_cache(maxsize=None)
def numeric_merged():
    return restate(numeric_packed(), numeric())


def flushed(cloud):
    """The cloud a kernel that flushes subnormal RESULTS to zero (sign kept) would store."""
    out = np.array(cloud, dtype=F)
    sub = np.isfinite(out) & (out != 0) & (np.abs(out) < FLT_MIN)
    out[sub] = np.copysign(F(0.0), out[sub])
    return out
