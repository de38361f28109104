"""nhip_csm_get_transformation at its flow and lattice seams (nhip_dropin.hip): every case of tests/dropin_seams.py through
CorrelativeScanMatcher.GetTransformation against the CPU oracle's two-level search -- translation and rotation equal as
floats, the score within 2e-7 relative (_same_call of tests/test_csm_gpu.py) -- and, from nhip_csm_get_transformation_info,
the flow the call took, the coarse winner's rotation and the coarse score against the oracle's coarse level.
tests/test_dropin_seams_cpu.py holds the preconditions: each input IS the case its family designed.

The info call does not report the coarse level's form (its double[4] is public ABI).  Each docstring names the form the
plan's rule gives; where that form is branch and bound it is asserted through nhip_csm_last_launch, which reports the calling
thread's last branch-and-bound launch (the fine level never is one here): the pairs of that launch are the parts the
rotations were dealt over, and a thread that never launched it reports none.  A dealt search is never chained."""
import threading

import numpy as np
import pytest

from nautilus_amd import _lib, csm
from tests import dropin_seams as S
from tests.test_csm_gpu import _dropin_info, _same_call

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, scope="module")
def _clean_cache(gpu):
    csm.drop_in_cache_clear()
    csm.drop_in_cache_configure(3 << 30)
    yield
    csm.drop_in_cache_configure(3 << 30)
    csm.drop_in_cache_clear()


def _call(case):
    m = csm.CorrelativeScanMatcher(*case.ctor, cell_bits=case.bits)
    return m.GetTransformation(case.a, case.b, case.rot_a, case.rot_b, case.restriction)


def _check(case):
    """One call against the oracle: the returned tuple, the flow, the coarse level's winner and score."""
    got = _call(case)
    info, want, f, first = _dropin_info(), S.want(case), S.flow_of(case), S.coarse(case)
    assert _same_call(got, want), (case.name, got, want)
    assert info["chained"] is f.chained and info["fine_form"] == f.fine_form, (case.name, info, f)
    assert info["coarse_itheta"] == first[0] and np.float32(info["coarse_score"]) == first[3], (case.name, info, first)
    return got


def _in_fresh_thread(fn):
    """fn() on a new thread -- its scratch, kept rotation tables and last-launch record are new -- and what it returned."""
    box = {}

    def run():
        try:
            box["value"] = fn()
        except BaseException as e:      # (handed to the caller below)
            box["error"] = e
    t = threading.Thread(target=run)
    t.start()
    t.join()
    if "error" in box:
        raise box["error"]
    return box["value"]


def test_translation_walk_over_and_beyond_the_coarse_lattice(gpu):
    """WALK (10, 1, 0.25, 0.1) at 3 degrees: 7 x 9 x 9 coarse and 21 x 7 x 7 fine, both in the kernel whose lanes are poses --
    chained and FUSED: dropin_bridge_kernel decodes the coarse key, computes the coarse score, rounds tx1 / high_res (exact
    halves +-2.5, +-7.5 at the odd coarse translations) and writes the fine level's parameter block.  121 shifts: every coarse
    translation wins, and the outermost ring clamps to the border, the fine search at the cached table's farthest reach."""
    assert S.flow(S.WALK, 3 * S.DEG).fused
    for case in S.translation_walk().values():
        _check(case)


@pytest.mark.parametrize("ctor,bits,coarse,parts", [(S.STRIPS, 16, "strips", 0), (S.BNB1, 16, "bnb", 1), (S.WALK, 8, "poses", 0)],
                         ids=["strips-then-small-plane", "bnb-one-part-chained", "fused-8bit"])
def test_translation_ring_in_the_other_chained_flows(gpu, ctor, bits, coarse, parts):
    """The 4 corners and 4 edge midpoints beyond the lattice, chained in every case.  STRIPS (10, 1, 0.125, 0.05): 17 x 17
    coarse in the strip kernels (finalize decodes its keys, the bridge reads the record), 7 x 7 fine in the small-plane kernel.
    BNB1 (10, 1.5, 0.125, 0.05): 25 x 25 coarse by branch and bound, 7 rotations in ONE part (asserted: the thread's last
    branch-and-bound launch had one pair, a short scan).  WALK with 8-bit cells: fused."""
    f = S.flow(ctor, 3 * S.DEG)
    assert f.chained and f.coarse == coarse and f.fused is (coarse == "poses")

    def ring():
        for case in S.translation_walk(ctor, bits, False).values():
            _check(case)
        return csm.last_launch()
    last = _in_fresh_thread(ring)
    assert last["n_pairs"] == parts and (parts == 0 or last["short_scans"]), last


@pytest.mark.parametrize("ij", S.ring(6), ids=lambda ij: "%+d%+d" % ij)
def test_translation_ring_of_the_default_constructor(gpu, ij):
    """DEFAULT (30, 2, 0.3, 0.01): 13 x 13 coarse in one tile, 61 x 61 fine in tiles of four rows, chained and fused; the
    coarse optimum on the border, the fine search 180 + 30 cells out of the 212 the cached table reaches."""
    assert S.flow(S.DEFAULT, 3 * S.DEG).fused and S.flow(S.DEFAULT, 3 * S.DEG).h1 == 6
    _check(S.translation_walk(S.DEFAULT, 16, False)[ij])


@pytest.mark.parametrize("bits", [16, 8])
def test_rotation_walk_across_the_parts(gpu, bits):
    """ROT (10, 3, 0.125, 0.05) at 20 degrees: 49 x 49 coarse by branch and bound, 41 rotations dealt over 6 parts of 7 with one
    copy of the last rotation behind the table -- one level after the other, dropin_pick between them.  The winner is
    rotation k + 20 inside the range (each part's first and last, and the table's last, whose copy ties and must lose), 0 and
    40 beyond it; an empty source ties everywhere and rotation 0 wins."""
    f = S.flow(S.ROT, 20 * S.DEG)
    assert (f.coarse, f.parts, f.per, f.chained) == ("bnb", 6, 7, False)
    walk = S.rotation_walk(bits)
    for k in range(-21, 22):
        _check(walk[k])
        info = _dropin_info()
        assert info["coarse_itheta"] == min(max(k + 20, 0), 40) and info["chained"] is False, (k, info)
        assert csm.last_launch()["n_pairs"] == 6
    _check(walk["empty"])
    assert _dropin_info()["coarse_itheta"] == 0 and _dropin_info()["chained"] is False


def test_rotation_counts_around_the_chained_forms_table(gpu):
    """WALK with 1, 1, 511, 513 and 721 coarse rotations (restrictions 0, 0.5, 255.5, 256.5 degrees, 2 pi), 9 x 9 coarse in the
    kernel whose lanes are poses: chained and fused up to DROPIN_CHAIN_ROT_MAX = 512 rotations -- half1 = 0 for a single one
    -- and one level after the other beyond."""
    for case, n, chained in S.rotation_counts():
        assert S.flow_of(case).n_theta1 == n and S.flow_of(case).coarse == "poses"
        _check(case)
        assert _dropin_info()["chained"] is chained, (case.name, _dropin_info())


def test_angle_wraps(gpu):
    """WALK, chained and fused: theta0 = rot_a - rot_b wrapped into [-pi, pi] with rint's tie at exactly +-pi ((pi, 0) stays
    +pi, (0, pi) stays -pi), and a coarse winner whose angle the fine level receives beyond +pi, unwrapped."""
    for case in S.angle_wraps().values():
        assert S.flow_of(case).fused
        _check(case)


@pytest.mark.parametrize("ctor,bits", [(S.WALK, 16), (S.ROT, 16), (S.ROT, 8)], ids=["fused", "bnb-16bit", "bnb-8bit"])
def test_source_lengths_and_scratch_reuse_on_one_thread(gpu, ctor, bits):
    """Sources of 2049, 7, 2048, 1089, 1088, 1, 0, 5000, 64 points on ONE new thread, the restriction alternating 3 / 20
    degrees: the scratch's cloud buffer starts at 2049 points, grows at 5000 and keeps old points behind every shorter cloud;
    the kept coarse rotation table (7 / 41 rotations) is replaced and replaced back.  WALK: both levels in the kernel whose lanes
    are poses, fused.  ROT: coarse by branch and bound, one part and chained at 3 degrees, six parts at 20 (asserted per call
    with NHIP_SEARCH_SHORT_SCANS at 1088 points and below).  The same calls in reverse order on another new thread return
    the same tuples."""
    seq = S.length_sequence(ctor, bits)

    def forward():
        out = []
        for case in seq:
            out.append(_check(case))
            if S.flow_of(case).coarse == "bnb":
                last = csm.last_launch()
                assert last["n_pairs"] == S.flow_of(case).parts and last["short_scans"] is (len(case.a) <= S.SHORT_SCAN), (case.name, last)
        return out
    first = _in_fresh_thread(forward)
    again = _in_fresh_thread(lambda: [_check(case) for case in reversed(seq)])
    assert again[::-1] == first


def test_non_cacheable_target_that_is_not_empty(gpu):
    """NOCACHE (2, 8.1, 0.21, 0.002): reach_max = 4097 > 4096, so the target is not cached and the fine table is built for the
    call's own coarse optimum, max_shift = max|origin| + ratio exactly: 105 cells for the matching pair, 3990 + 105 for the
    pair in the corner of the 77 x 77 coarse lattice (branch and bound in one part; 211 x 211 fine in the strip kernels).  One
    level after the other; the cache gains nothing and counts nothing.  REFUSED (2, 8.2, 0.2, 0.002): the matching pair the
    same; in the corner the fine table would need max_shift = 4100, beyond what a grid spec admits -- the call fails with
    that error and returns nothing."""
    csm.drop_in_cache_clear()
    before = csm.drop_in_cache_stats()
    for case in list(S.non_cacheable().values()) + [S.non_cacheable(S.REFUSED)["match"]]:
        f = S.flow_of(case)
        assert not f.cacheable and (f.coarse, f.parts, f.fine_form) == ("bnb", 1, 1)
        _check(case)
        assert _dropin_info()["chained"] is False and _dropin_info()["fine_form"] == 1
        assert csm.last_launch()["n_pairs"] == 1
    with pytest.raises(_lib.NhipError, match="max_shift out of range"):
        _call(S.non_cacheable(S.REFUSED)["corner"])
    assert csm.drop_in_cache_stats() == before and before["entries"] == 0


def test_cache_order_under_a_cap_of_two_targets(gpu):
    """Three targets under a cap of 2.5 entries: a hit moves its entry to the front, an insert drops the LEAST recently used
    one; exactly two entries' bytes hold two, one byte less holds one -- the most recent.  Every call returns its first
    value, the oracle's.  (An entry counts the capacity of the device buffers it holds, and a build may take a larger buffer
    that an earlier handle left in the library's device pool: the pool is emptied first, so that the three entries -- one
    constructor, one layout -- weigh the same.)"""
    t = S.cache_targets()
    first = {}

    def call(name, entries, hit):
        before = csm.drop_in_cache_stats()
        got = _check(t[name])
        st = csm.drop_in_cache_stats()
        assert first.setdefault(name, got) == got, name
        assert (st["entries"], st["hits"] - before["hits"], st["misses"] - before["misses"]) == (entries, int(hit), int(not hit)), (name, before, st)
        return st
    try:
        csm.drop_in_cache_clear()
        csm.drop_in_cache_configure(3 << 30)
        _lib.check(_lib.load().nhip_device_pool_release())
        one = call("A", 1, False)["bytes"]
        assert one > 0
        csm.drop_in_cache_configure(one * 5 // 2)
        assert call("B", 2, False)["bytes"] == 2 * one
        call("A", 2, True)          # A to the front: B is now the least recently used
        call("C", 2, False)         # B is dropped, not A
        call("A", 2, True)
        call("B", 2, False)         # (C is dropped)
        call("A", 2, True)
        csm.drop_in_cache_configure(2 * one)
        assert csm.drop_in_cache_stats()["entries"] == 2
        call("B", 2, True)
        csm.drop_in_cache_configure(2 * one - 1)
        assert csm.drop_in_cache_stats()["entries"] == 1 and csm.drop_in_cache_stats()["bytes"] == one
        call("B", 1, True)          # the survivor is the most recently used
        call("A", 1, False)         # (2 * one - 1 bytes hold one entry: A replaces B)
    finally:
        csm.drop_in_cache_configure(3 << 30)
        csm.drop_in_cache_clear()
