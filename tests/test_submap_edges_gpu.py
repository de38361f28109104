"""The submap gather at its batch, step, stride and int32 edges (kernels nhip_submap.hip, K10; DESIGN.md section 3, "Submaps"):
member lists that make every input-dependent loop of the unit run more than once, each against the numpy restatement
(hostside.submap_clouds) bit for bit -- R.same_cloud: equal bits wherever the expectation is finite, so -0 is not +0 and
subnormals count; out_offsets equal; the canary behind the cloud and the unused tail of the capacity untouched.  No tolerance,
no excluded point.  Inputs: tests/submap_edges.py (tests/test_submap_edges_cpu.py holds their preconditions).

Not tested: an ACCEPTED cloud near 2^31 points (a 17 GB buffer); misaligned xy / output pointers (float2 accesses)."""
import ctypes as C
import math

import numpy as np
import pytest

from nautilus_amd import _lib, csm, hostside
from oracle import oracle as O
from tests import submap_edges as E
from tests import submap_reference as R
from tests.test_submap_gpu import CANARY, Device, small_spec

pytestmark = pytest.mark.gpu

DEG = math.radians(1.0)
OK, ERR_ARG = _lib.NHIP_OK, _lib.NHIP_ERR_ARG
BAD_MEMBER_ID, BAD_SUBMAP_CAPACITY = 512, 1024  # nhip_common.h: the kinds of the status words


class EdgeDevice(Device):
    """tests/test_submap_gpu.py's Device (its gather and build, unchanged) over another bag."""

    def __init__(self, packed):
        import torch
        self.torch, self.dev, self.lib = torch, torch.device("cuda:0"), _lib.load()
        self.sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        xy, off = packed
        self.n_scans = len(off) - 1
        self.d_xy, self.d_off = self.up(xy), self.up(off)

    def gather_equals(self, members, want, capacity=None):
        """One launch over `members`: status clean, offsets and cloud the restatement's, tail and canary untouched."""
        want_xy, want_off = want
        n = len(want_xy)
        rc, info, cloud, off, canary = self.gather(*members, capacity=n if capacity is None else capacity)
        assert rc == OK, info
        assert np.array_equal(off, want_off)
        assert R.same_cloud(cloud[:n], want_xy), \
            "first differing points: %s" % np.nonzero((cloud[:n].view(np.uint32) != want_xy.view(np.uint32)).any(axis=1))[0][:5]
        assert np.all(cloud[n:] == -77.0) and np.all(canary == -77.0)

    def gather_raw(self, d_xy, d_scan, d_aff, d_moff, n_targets, d_out, capacity):
        """The call on the pointers as given (a tensor or None): (rc of the call, rc of nhip_dev_status, info, offsets)."""
        p = lambda t: None if t is None else t.data_ptr()
        d_goff = self.torch.full((n_targets + 1,), -5, dtype=self.torch.int32, device=self.dev)
        rc_call = self.lib.nhip_submaps_gather_dev(p(d_xy), self.d_off.data_ptr(), self.n_scans, p(d_scan), p(d_aff), p(d_moff),
                                                   n_targets, p(d_out), capacity, d_goff.data_ptr(), self.sp)
        rc, info = self.status()
        return rc_call, rc, info, d_goff.cpu().numpy()


@pytest.fixture(scope="module")
def mini(gpu):
    return EdgeDevice(E.mini_packed())


@pytest.fixture(scope="module")
def numeric(gpu):
    return EdgeDevice(E.numeric_packed())


# ------------------------------------------------------------------------------------------------ 1. many members
def test_a_target_of_900_members_runs_the_member_batch_loop(mini):
    """submap_gather_kernel, `for base = mb; base < me; base += SUB_T`: four batches; the carried `run`; `if (b_end > at)` false
    for chunks that begin in the third and fourth batch; a batch whose members are all empty (`all == 0`); empty members on
    either side of the 256 seam; the __syncthreads() before the table is rewritten; a target seam inside a chunk."""
    mini.gather_equals(E.many_members(), E.many_members_merged())


def test_bad_ids_in_the_third_and_fourth_batch_are_empty_members(mini):
    """`member_points` / `flag_bad_id(status, BAD_MEMBER_ID, id, m)` on members only the batch loop reaches: -1 in the third
    batch, n_scans in the fourth -- kind 512, one of the two named, neither dereferenced, the rest of the cloud unchanged."""
    members, (first, second) = E.many_members_bad_ids()
    want_xy, want_off = hostside.submap_clouds(*E.mini_packed(), *members)
    full_xy, full_off = E.many_members_merged()
    dropped = E.MINI_LENGTHS[E.many_members()[0][first]] + E.MINI_LENGTHS[E.many_members()[0][second]]
    assert want_off[-1] == full_off[-1] - dropped and dropped > 0
    rc, info, cloud, off, canary = mini.gather(*members, capacity=len(full_xy))
    assert rc == ERR_ARG and info[0] == BAD_MEMBER_ID and info[1] == BAD_MEMBER_ID, info
    assert (info[2], info[3]) in ((-1, first), (mini.n_scans, second)), info
    assert b"member scan id" in mini.lib.nhip_last_error()
    assert np.array_equal(off, want_off)
    assert R.same_cloud(cloud[:len(want_xy)], want_xy)
    assert np.all(cloud[len(want_xy):] == -77.0) and np.all(canary == -77.0)
    assert mini.status()[0] == OK, "the record was consumed"


# ------------------------------------------------------------------------------------------------ 2. many targets
def test_2500_targets_run_the_offsets_steps_and_the_target_walk(mini):
    """submap_offsets_kernel, `for base = 0; base < n_targets; base += 1024`: three steps, the 64-bit `carry`, a step that adds
    nothing, a ragged last step.  submap_gather_kernel: the bisection of out_offsets and `if (t_end <= at) continue` over runs
    of empty targets (the first 5, 1,100 in the middle, the last 7), hundreds of targets in one chunk.  Then the grid at its
    cap: capacity 2048 * 2048 + 4096 launches all 2,048 workgroups, all but four find `pos >= total` -- same cloud, tail
    untouched."""
    want = E.many_targets_merged()
    mini.gather_equals(E.many_targets(), want)
    capacity = E.GATHER_MAX_GRID * E.GATHER_CHUNK + 4096
    assert -(-capacity // E.GATHER_CHUNK) > E.GATHER_MAX_GRID
    mini.gather_equals(E.many_targets(), want, capacity=capacity)


@pytest.mark.parametrize("n_targets", [E.OFFSETS_STEP, E.OFFSETS_STEP + 1])
def test_a_launch_that_ends_at_a_step_seam_gives_a_prefix(mini, n_targets):
    """submap_offsets_kernel: n_targets == 1024 (one full step, `sc[1023]` is the total) and 1025 (a second step of one lane):
    out_offsets is the prefix of the 2,500-target result, the cloud its first points."""
    full_xy, full_off = E.many_targets_merged()
    want_off = full_off[:n_targets + 1]
    mini.gather_equals(E.first_targets(E.many_targets(), n_targets), (full_xy[:want_off[-1]], want_off))


# ------------------------------------------------------------------------------------------------ 3. grid stride
def test_4324000_points_give_workgroups_a_second_chunk(mini):
    """submap_gather_kernel, `pos += gridDim.x * SUB_CHUNK`: the grid is min(ceil(capacity / 2048), 2048) workgroups, so a
    workgroup takes a second chunk only above 2048 * 2048 = 4,194,304 points.  400 targets x 10 members x 1081 points is
    4,324,000: 2,112 chunks, the last one ragged.  DO NOT SHRINK: below 4,194,305 points this test no longer runs the stride."""
    mini.gather_equals(E.grid_stride(), E.grid_stride_merged())


# ------------------------------------------------------------------------------------------------ 4. totals beyond int32
@pytest.mark.parametrize("case", E.BEYOND_CASES)
def test_a_total_beyond_int32_is_refused_and_nothing_is_stored(mini, case):
    """submap_offsets_kernel, `total <= out_capacity && total <= 0x7fffffff` on 64-bit `len`, `sc` and `carry`; the header's
    "more than 2^31 - 1 points" (Capacity).  a: 2^32 + 1081 in one lane (1081 in 32 bits: it would fit);
    b: the same over 2,048 targets, the carry 2^31 at the step seam; c: 2^31; d: 2^31 - 1, which fits int32 but not the
    capacity.  The call returns NHIP_OK, the status kind 1024 with the needed points clamped to 2^31 - 1 and index
    n_targets; every out_offsets entry 0; buffer and canary untouched; the next gather works.  (An accepted cloud of this
    size needs a 17 GB buffer: out of scope.)"""
    members, total, value = E.beyond_int32(case)
    n_targets = len(members[2]) - 1
    rc, info, cloud, off, canary = mini.gather(*members, capacity=E.BEYOND_CAPACITY)  # (raises unless the call returns NHIP_OK)
    assert rc == ERR_ARG and info[0] == BAD_SUBMAP_CAPACITY and info[1] == BAD_SUBMAP_CAPACITY, info
    assert info[2] == value == min(total, 2 ** 31 - 1) and info[3] == n_targets, info
    assert b"out_capacity" in mini.lib.nhip_last_error()
    assert len(off) == n_targets + 1 and np.all(off == 0)
    assert np.all(cloud == -77.0) and np.all(canary == -77.0)
    assert mini.status()[0] == OK, "the record was consumed"
    full_xy, full_off = E.many_targets_merged()
    mini.gather_equals(E.first_targets(E.many_targets(), 40), (full_xy[:full_off[40]], full_off[:41]))
    assert mini.status() == (OK, [0, 0, 0, 0])


# ------------------------------------------------------------------------------------------------ 5. zero capacity, zero targets
def test_zero_capacity_takes_null_pointers_and_reports_the_total(mini):
    """nhip_submaps_gather_dev, `out_capacity == 0 || (d_xy && d_member_affine && d_out_xy)`, and launch_submap_gather's
    `chunks > 0`: without room no gather is launched and the point, affine and output pointers may be null.  With members
    that have points: kind 1024, value the total, offsets 0.  With members of 0 points only: NHIP_OK, offsets 0."""
    member_scan, _, moff = E.many_members()
    total = int(E.many_members_merged()[1][-1])
    rc_call, rc, info, off = mini.gather_raw(None, mini.up(member_scan), None, mini.up(moff), len(moff) - 1, None, 0)
    assert rc_call == OK and rc == ERR_ARG and info == [BAD_SUBMAP_CAPACITY, BAD_SUBMAP_CAPACITY, total, len(moff) - 1], info
    assert np.all(off == 0)
    member_scan, _, moff = E.empty_members()
    rc_call, rc, info, off = mini.gather_raw(None, mini.up(member_scan), None, mini.up(moff), len(moff) - 1, None, 0)
    assert rc_call == OK and rc == OK and info == [0, 0, 0, 0], info
    assert np.all(off == 0)


def test_zero_targets_take_a_null_member_list(mini):
    """nhip_submaps_gather_dev, `d_member_scan || n_targets == 0`; submap_offsets_kernel with no step to run writes
    out_offsets[0] = 0; launch_submap_gather's `n_targets > 0` launches no gather: the output is untouched."""
    torch = mini.torch
    buf = torch.full((2 * 64 + CANARY,), -77.0, dtype=torch.float32, device=mini.dev)
    d_aff = mini.up(np.float32([[1, 0, 0, 0]]))
    rc_call, rc, info, off = mini.gather_raw(mini.d_xy, None, d_aff, mini.up(np.zeros(1, np.int32)), 0, buf, 64)
    assert rc_call == OK and rc == OK and info == [0, 0, 0, 0], info
    assert off.tolist() == [0]
    assert torch.all(buf == -77.0).item()


def test_affines_four_bytes_past_a_16_byte_boundary(mini):
    """submap_gather_kernel, "four loads: the array need not be 16-byte aligned": member_affine at an address that is 4 modulo 16
    gives the cloud of the aligned call."""
    torch = mini.torch
    member_scan, aff, moff = E.many_members()
    want_xy, want_off = E.many_members_merged()
    longer = torch.zeros(aff.size + 1, dtype=torch.float32, device=mini.dev)
    longer[1:] = mini.up(aff).reshape(-1)
    d_aff = longer[1:]
    assert d_aff.data_ptr() % 16 == 4 and d_aff.is_contiguous()
    n = len(want_xy)
    buf = torch.full((2 * n + CANARY,), -77.0, dtype=torch.float32, device=mini.dev)
    rc_call, rc, info, off = mini.gather_raw(mini.d_xy, mini.up(member_scan), d_aff, mini.up(moff), len(moff) - 1, buf, n)
    assert rc_call == OK and rc == OK, info
    host = buf.cpu().numpy()
    assert np.array_equal(off, want_off) and R.same_cloud(host[:2 * n], want_xy) and np.all(host[2 * n:] == -77.0)


# ------------------------------------------------------------------------------------------------ 6. numeric edges
def test_the_point_transform_at_the_ends_of_float(numeric):
    """submap_gather_kernel, `__fadd_rn(__fadd_rn(__fmul_rn(T.x, p.x), __fmul_rn(-T.y, p.y)), T.z)` (Point
    transform: every operation rounds on its own in float): subnormal products and sums kept, -0 kept apart from +0, overflow
    from finite inputs, inf x 0 and inf - inf NaN, where the restatement has them.  A contracted kernel, one that flushes
    subnormal results or one that loses a zero's sign fails (tests/test_submap_edges_cpu.py)."""
    numeric.gather_equals(E.numeric(), E.numeric_merged())


# ------------------------------------------------------------------------------------------------ 7. tables, the handle form
@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("case", ["many_members", "numeric"])
def test_tables_of_the_gathered_cloud_are_the_tables_of_the_host_merged_cloud(mini, numeric, case, bits):
    """nhip_grid_build_dev reads the gather's out_xy / out_offsets as it reads plain scans: the tables of the gathered cloud of
    900 + 4 members (two targets) and of the numeric target (non-finite, huge and subnormal points: hit_cell drops what
    leaves the grid) are byte-equal to those of the host-merged cloud uploaded as plain scans."""
    device, members, (mxy, moff) = {"many_members": (mini, E.many_members(), E.many_members_merged()),
                                    "numeric": (numeric, E.numeric(), E.numeric_merged())}[case]
    spec = small_spec(bits)
    n = len(moff) - 1
    rc, info, cloud, off, _ = device.gather(*members, capacity=len(mxy))
    assert rc == OK and np.array_equal(off, moff) and R.same_cloud(cloud, mxy), info
    d_gxy, d_goff = device.last
    got, _, _ = device.build(d_gxy, d_goff, n, spec)
    want, _, _ = device.build(device.up(mxy), device.up(moff), n, spec)
    assert got.any() and np.array_equal(got, want)


@pytest.fixture(scope="module")
def scan_table(gpu):
    st = csm.ScanTable(*E.mini_packed())
    yield st
    st.close()


@pytest.mark.parametrize("bits", [16, 8])
def test_handle_form_on_900_members_and_after_a_handle_of_zero_targets(scan_table, bits):
    """nhip_grids_build_submaps on a member list of several batches: interior(t) is the oracle's table of the merged cloud.
    Then `n_targets == 0` (member_offsets == [0]: the offsets kernel alone runs, `InFlight::done()`): a handle that closes
    cleanly, and the same submaps built after it give the same tables."""
    spec, ospec = small_spec(bits), O.grid_spec(R.RANGE_M, R.RES, R.SIGMA, 1e-10, bits)
    mxy, moff = E.many_members_merged()
    assert np.isfinite(mxy).all()
    n = len(moff) - 1
    ogr = O.grid_build_batch(mxy, moff, np.arange(n), ospec)
    grids = csm.LikelihoodGrids.from_submaps(scan_table, *E.many_members(), spec)
    try:
        before = [grids.interior(t).copy() for t in range(n)]
    finally:
        grids.close()
    for t in range(n):
        assert before[t].any() and np.array_equal(before[t], ogr[t]), "slot %d differs from the oracle's table of the merged cloud" % t
    none = csm.LikelihoodGrids.from_submaps(scan_table, np.zeros(0, np.int32), np.zeros((0, 4), np.float32), np.zeros(1, np.int32), spec)
    assert len(none.target_ids) == 0
    none.close()
    again = csm.LikelihoodGrids.from_submaps(scan_table, *E.many_members(), spec)
    try:
        for t in range(n):
            assert np.array_equal(again.interior(t), before[t]), t
    finally:
        again.close()


def test_the_host_entry_refuses_malformed_member_lists(scan_table):
    """nhip_grids_build_submaps: `member_offsets[0] == 0`, "member_offsets not monotone at target", "null member array" and
    the host's own `total <= 0x7fffffff` (case c's 32,768 members of the 65,536-point scan: 2^31 points, refused before
    anything is allocated) -- each NHIP_ERR_ARG with a message, *out not set, the library usable afterwards."""
    lib, spec = _lib.load(), small_spec(16)
    member_scan, aff, moff = (np.array(a) for a in E.many_members())
    shifted = moff.copy()
    shifted[0] = 1
    falling = np.array([0, 5, 3, len(member_scan)], dtype=np.int32)
    (c_scan, c_aff, c_moff), total, _ = E.beyond_int32("c")
    assert total == 2 ** 31 and scan_table.n_scans == len(E.MINI_LENGTHS)
    cases = [("must be 0", member_scan, aff, shifted),
             ("not monotone", member_scan, aff, falling),
             ("null member", None, aff, moff),
             ("int32", np.array(c_scan), np.array(c_aff), np.array(c_moff))]
    SENTINEL = 0x5a5a5a5a
    for words, ms, af, mo in cases:
        out = C.c_void_p(SENTINEL)
        rc = lib.nhip_grids_build_submaps(scan_table._h, _lib.ptr(ms), _lib.ptr(af), _lib.ptr(mo), len(mo) - 1, C.byref(spec), C.byref(out))
        msg = lib.nhip_last_error()
        assert rc == ERR_ARG and len(msg) > 0 and words.encode() in msg, (words, rc, msg)
        assert out.value == SENTINEL, "*out is not set"
    grids = csm.LikelihoodGrids.from_submaps(scan_table, member_scan, aff, moff, spec)
    try:
        ogr = O.grid_build_batch(*E.many_members_merged(), np.arange(2), O.grid_spec(R.RANGE_M, R.RES, R.SIGMA, 1e-10, 16))
        assert np.array_equal(grids.interior(1), ogr[1])
    finally:
        grids.close()


# ------------------------------------------------------------------------------------------------ 8. the backend
@pytest.mark.parametrize("radius", [3, 40])
def test_backend_routes_agree_at_the_ends_of_the_bag(gpu, radius):
    """HipBackend.match(..., submap_radius, poses) where hostside.submap_members clips the window: targets 0, 1, 28 and 29 of a
    30-scan bag at radius 3, and radius 40, where every submap is the whole bag clipped at both ends.  The records are
    byte-equal to the host-merge route (hostside.submap_extra_scans, then match without the keyword)."""
    from nautilus_amd import posegraph, synth
    bag = synth.SynthBag(30)
    xy, off = csm.pack_scans(bag.scans)
    tgt = np.repeat([0, 1, 28, 29], 2).astype(np.int32)
    src = np.array([10, 20, 11, 19, 9, 18, 12, 17], dtype=np.int32)
    a = bag.odom[src, 2] - bag.odom[tgt, 2]
    th0 = a - 2 * math.pi * np.rint(a / (2 * math.pi))
    _, moff = hostside.submap_members(bag.n_scans, np.unique(tgt), radius)
    assert np.diff(moff).tolist() == ([4, 5, 5, 4] if radius == 3 else [30] * 4), "clipped at both ends"
    backend = posegraph.HipBackend()
    m_dev, _, _ = backend.match(xy, off, src, tgt, th0, 16, submap_radius=radius, poses=bag.odom)
    xy_m, off_m, tgt_m = hostside.submap_extra_scans(xy, off, bag.odom, tgt, radius)
    m_host, _, _ = backend.match(xy_m, off_m, src, tgt_m, th0, 16)
    assert m_dev.tobytes() == m_host.tobytes()
    assert (m_dev["itheta"] >= 0).all() and np.isfinite(m_dev["score"]).all()
