"""The crafted descriptor sets of the place-sequence tests (tests/test_place_seq_cpu.py, tests/test_place_seq_gpu.py): descriptors
given directly as uint64 words, no clouds.  Every case is (D uint64 [n, R], bits int32 [n], ids, keywords of the two specs); the
restatement's answer is computed once per case and shared."""
import functools

import numpy as np

from tests import place_reference as R
from tests import place_seq_reference as Q

FULL = np.uint64(0xFFFFFFFFFFFFFFFF)


def count(D):
    return np.bitwise_count(D).sum(axis=1).astype(np.int32)


def sparse(n, n_rings, seed, density=3):
    """random words, a bit set with probability 2^-density"""
    rng = np.random.default_rng(seed)
    D = np.full((n, n_rings), FULL, dtype=np.uint64)
    for _ in range(density):
        D &= rng.integers(0, 1 << 64, (n, n_rings), dtype=np.uint64)
    return D


def rotl(D, s):
    return np.stack([R.rotl64(row, s) for row in D]) if len(D) else D


def seam(n, W, step):
    """every scan a query at the smallest admitted separation: the windows of the first and last W step scans hang over both ends"""
    D = sparse(n, 4, 1000 + n)
    return D, count(D), np.arange(n), dict(n_rings=4, top_k=5, min_separation=2 * W * step, half_window=W, step=step)


def identity_set():
    """130 random descriptors of 10 rings, a zero-bit scan and duplicates among them"""
    D = sparse(130, 10, 130)
    D[7] = 0
    D[40], D[41], D[100] = D[3], D[3], D[3]
    return D, count(D)


def two_halves(reverse):
    """80 scans; the second half is the first half (reversed or not), every descriptor rotated by 5 sectors"""
    first = sparse(40, 10, 77, density=1)
    D = np.concatenate([first, rotl(first[::-1] if reverse else first, 5)])
    return D, count(D), np.arange(80), dict(top_k=3, min_separation=8, half_window=2, step=2)


def identical():
    D = np.tile(sparse(1, 10, 5), (70, 1))
    return D, count(D), np.arange(70), dict(top_k=32, min_separation=4, half_window=2, step=1)


def empty_frames():
    """every fifth scan empty; 52 and 54 empty beside the centre 53"""
    D = sparse(90, 10, 9)
    D[::5] = 0
    D[52], D[54] = 0, 0
    return D, count(D), np.arange(90), dict(top_k=6, min_separation=6, half_window=1, step=1)


def gate_set():
    """Dense random descriptors: two unrelated ones lie at about 0.45 of bits_i + bits_j.  (50, 10): the centres are identical,
    the frames around them unrelated; (55, 20): the centres unrelated, the frames on both sides identical."""
    D = sparse(60, 10, 31, density=1)
    D[50] = D[10]
    D[54], D[56] = D[19], D[21]
    return D, count(D)


def largest_sums():
    """R = 15: scans 0..29 every bit, scans 30..59 one bit: dist 959, and 17 frames of it are 16,303"""
    D = np.zeros((60, 15), dtype=np.uint64)
    D[:30] = FULL
    D[30:, 0] = np.uint64(1) << (np.arange(30, dtype=np.uint64) % np.uint64(64))
    return D, count(D), np.arange(60), dict(n_rings=15, top_k=32, min_separation=16, half_window=8, step=1)


def list_set():
    D = sparse(200, 10, 200)
    return D, count(D)


def list_ids(n=200):
    return np.unique(np.concatenate([np.arange(0, n, 7), [3, 100, 199]]))


@functools.lru_cache(maxsize=None)
def tables(key):
    """the single distances of a set, by the name the tests give it (computed once)"""
    D, bits = SETS[key]()[:2]
    return Q.single_distances(D, bits)


SETS = {"identity": identity_set, "gate": gate_set, "list": list_set,
        "halves-reversed": lambda: two_halves(True), "halves": lambda: two_halves(False), "identical": identical,
        "empty": empty_frames, "largest": largest_sums}
for _n in (63, 64, 65, 257):
    SETS["seam-%d" % _n] = functools.partial(lambda n: seam(n, 0, 1)[:2], _n)


@functools.lru_cache(maxsize=None)
def want(key, ids, top_k=5, min_separation=20, max_permille=1000, flags=0, half_window=2, step=1, n_rings=10):
    """the restatement's (records, stats) of the set `key` (ids: a tuple)"""
    D, bits = SETS[key]()[:2]
    assert D.shape[1] == n_rings
    return Q.match(D, bits, np.array(ids, dtype=np.int64), top_k, min_separation, max_permille, flags, half_window, step, tables=tables(key))


def cases():
    """(name, set key, ids, keywords) of every case that both the host path and the device must answer as the restatement does"""
    out = []
    for n in (63, 64, 65, 257):
        for W in (1, 2, 8):
            for step in (1, 3):
                out.append(("seam-%d-W%d-step%d" % (n, W, step), "seam-%d" % n, np.arange(n), seam(n, W, step)[3]))
    for key in ("halves-reversed", "halves", "identical", "empty", "largest"):
        D, bits, ids, kw = SETS[key]()
        out.append((key, key, ids, kw))
    gate = dict(top_k=32, min_separation=8, half_window=1, step=1)
    out += [("gate-200", "gate", np.arange(60), dict(gate, max_permille=200)), ("gate-0", "gate", np.arange(60), dict(gate, max_permille=0)),
            ("gate-1000", "gate", np.arange(60), dict(gate, max_permille=1000)),
            ("gate-0-identical", "identical", np.arange(70), dict(identical()[3], max_permille=0))]
    ids = list_ids()
    out += [("list", "list", ids, dict(top_k=4, min_separation=12, half_window=2, step=3)),
            ("list-past-only", "list", ids, dict(top_k=4, min_separation=12, half_window=2, step=3, flags=R.PAST_ONLY)),
            ("list-top-1", "list", ids, dict(top_k=1, min_separation=4, half_window=2, step=1)),
            ("list-top-32", "list", ids[:20], dict(top_k=32, min_separation=4, half_window=2, step=1)),
            ("past-only-all", "identity", np.arange(130), dict(top_k=5, min_separation=4, half_window=2, step=1, flags=R.PAST_ONLY))]
    return out
