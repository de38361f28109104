"""Preconditions of the step-seam tests (tests/test_step_seams_gpu.py), without a GPU: every scan of tests/step_seams.py's HITL
lists has the membership it was designed for under hostside.hitl_relevant_poses, every arrangement the lists are named for
occurs, and the feature tables reach every count, seam and lane they were cut for.  A precondition that fails means the input
is wrong.  (nhip_hitl.hip hitl_offsets_kernel; nhip_feat.hip feat_offsets_kernel, feat_pack_kernel.)"""
import os

import numpy as np
import pytest

from tests import feature_reference as FR
from tests import step_seams as S


def test_the_kernel_constants_are_the_ones_the_inputs_were_cut_for():
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nautilus_amd", "csrc")
    with open(os.path.join(root, "nhip_hitl.hip")) as f:
        hitl = f.read()
    with open(os.path.join(root, "nhip_feat.hip")) as f:
        feat = f.read()
    assert "base < n_scans; base += %d)" % S.STEP in hitl and "-2 - (carry[1] + sc[1][t] - 1)" in hitl
    assert "base < n_scans; base += %d)" % S.STEP in feat and "constexpr int FT = %d;" % (64 * S.SCANS_PER_WORKGROUP) in feat
    assert "blockIdx.x * (FT / 64) + (threadIdx.x >> 6)" in feat


@pytest.mark.parametrize("name", list(S.HITL_LISTS))
def test_every_scan_has_its_designed_membership(name):
    s, e = S.hitl_list(name), S.hitl_expected(name)
    n = S.HITL_LISTS[name]
    kind = s.kind
    lengths = np.diff(s.offsets)
    assert len(s.scans) == n == len(kind) and lengths.max() <= S.MAX_POINTS and (lengths == 0).any() and (lengths == S.MAX_POINTS).any()
    is_a, is_b = (kind == S.ON_A) | (kind == S.BOTH), kind == S.ON_B
    assert [i for i, _ in e.a_poses] == np.nonzero(is_a)[0].tolist(), "the a-nodes are the scans designed on a or on both"
    assert [i for i, _ in e.b_poses] == np.nonzero(is_b)[0].tolist()
    assert [len(p) for _, p in e.a_poses] == s.on_a[is_a].tolist() and [len(p) for _, p in e.b_poses] == s.on_b[is_b].tolist()
    assert np.all(s.on_a[is_a] >= S.THRESHOLD) and np.all(s.on_a[~is_a] < S.THRESHOLD) and np.all(s.on_b[is_b] >= S.THRESHOLD)
    assert np.all(s.on_b[kind == S.BOTH] >= S.THRESHOLD), "a scan with enough points on both lines goes to a"
    for members, other in ((is_b, s.on_a), (kind == S.ON_A, s.on_b)):
        assert not members.any() or (other[members] > 0).any(), "a member's points on the other line are dropped"
    # the arrangement
    assert S.seam_runs(n) == [(seam - 40, min(seam + 40, n)) for seam in range(1024, n + 40, 1024)] and S.seam_runs(n)
    for lo, hi in S.seam_runs(n):
        assert np.all(kind[lo:hi] == S.NEITHER) and np.all(e.scan_block[lo:hi] == -1)
    if name.startswith("mixed"):
        assert e.n_a > 100 and e.n_b > 100
        assert (kind[:S.STEP] == S.BOTH).any()
    if n > S.STEP + S.SEAM_RUN and not name.startswith("no"):
        first = S.STEP + S.SEAM_RUN
        assert is_a[first:].any() and is_b[:S.STEP].any(), "b-nodes of the first step are renumbered by a-nodes of a later one"
        assert e.scan_block[np.nonzero(is_b)[0][0]] == e.n_a and e.scan_offset[np.nonzero(is_b)[0][0]] == e.block_offsets[e.n_a] > 0
    if name.startswith("no a"):
        assert e.n_a == 0 and e.n_b > 500 and is_b[S.STEP + S.SEAM_RUN:].any()
    if name.startswith("no b"):
        assert e.n_b == 0 and e.n_a > 500
    if name.startswith("late a"):
        assert np.nonzero(is_a)[0][0] >= S.LATE_A_FROM > S.STEP + S.SEAM_RUN and is_b[:S.STEP].sum() > 100 and e.n_a > 100
    assert e.block_offsets[-1] == len(e.points) == s.on_a[is_a].sum() + s.on_b[is_b].sum()
    assert np.array_equal(np.sort(e.scan_block[e.scan_block >= 0]), np.arange(e.n_a + e.n_b))
    print("HITL %s: %d scans, %d a-nodes, %d b-nodes, %d points" % (name, n, e.n_a, e.n_b, len(e.points)))


def test_the_lists_cover_the_step_counts_and_arrangements():
    assert sorted(set(S.HITL_LISTS.values())) == [1023, 1024, 1025, 2049, 2500]
    assert sum(k.startswith("mixed") for k in S.HITL_LISTS) == 5 and {k[:6] for k in S.HITL_LISTS} == {"mixed ", "no a 2", "no b 2", "late a"}
    assert (S.LINE_A, S.LINE_B, S.WIDTH, S.THRESHOLD) == ((0.0, 0.0, 4.0, 3.0), (0.0, 3.0, 4.0, 0.0), 0.05, 3)


@pytest.mark.parametrize("cap", S.FEATURE_CAPS)
@pytest.mark.parametrize("n", S.FEATURE_SCANS)
def test_the_feature_tables(n, cap):
    xy, normals, offsets = S.features_cloud()
    c = S.features_case(n, cap)
    lengths = np.diff(offsets)[:n]
    assert c.idx.shape == (n, cap) and c.idx.dtype == np.int32 and c.count.dtype == np.int32
    assert c.count.min() == 0 and c.count.max() == cap and c.count[0] == cap == c.count[n - 1]
    assert set(np.unique(c.count)) == set(range(cap + 1)) or cap == 64, "every count occurs"
    live = np.arange(cap)[None, :] < c.count[:, None]
    assert np.all(c.idx[~live] == -1) and np.all(c.idx[live] >= 0) and np.all((c.idx < lengths[:, None])[live])
    if cap == 64:
        assert live[:, 63].sum() > 50, "lane 63 is live"
    for lo, hi in S.feature_zero_runs(n):
        assert np.all(c.count[lo:hi] == 0) and hi - lo >= 30, "a long run"
    assert S.feature_zero_runs(n) and n % S.SCANS_PER_WORKGROUP != 0
    exy, enrm, eoff = c.expect[True]
    assert np.array_equal(np.diff(eoff), c.count) and len(exy) == len(enrm) == eoff[-1] == c.count.sum()
    lo, hi = S.feature_zero_runs(n)[0]
    assert lo < S.STEP and 0 < eoff[lo] < eoff[-1] and np.all(eoff[lo:hi + 1] == eoff[lo]), "the carry into the second step is not 0"
    assert n < 2 * S.STEP or (hi > S.STEP and eoff[hi] < eoff[2 * S.STEP - S.SEAM_RUN]), "features between the two seams"
    pxy, poff = c.expect[False]
    assert pxy.tobytes() == exy.tobytes() and np.array_equal(poff, eoff)
    # the reference, spelled out for one scan on either side of the first seam
    for s in (S.STEP - S.SEAM_RUN - 1, min(S.STEP + S.SEAM_RUN, n - 1)):
        want = xy[offsets[s] + c.idx[s, :c.count[s]]]
        assert exy[eoff[s]:eoff[s + 1]].tobytes() == want.tobytes()
    for a in (c.idx, c.count, exy, enrm, eoff):
        assert not a.flags.writeable


def test_the_scan_counts_leave_every_partial_last_workgroup():
    assert sorted({n % S.SCANS_PER_WORKGROUP for n in S.FEATURE_SCANS}) == [1, 2, 3]
    assert FR.clouds(np.zeros((3, 2), np.float32), None, np.array([0, 3]), np.array([[2, 0]]), np.array([2]))[2].tolist() == [0, 2]
