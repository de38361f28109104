"""Submaps on the GPU ("Submaps"; kernels nhip_submap.hip): the gather against the numpy restatement bit for
bit, bad member ids and a capacity one point short (status words, nothing dereferenced, nothing stored), the tables built
from the gathered cloud against those built from the host-merged cloud byte for byte, the handle form and HipBackend.match
against the oracle on the merged clouds, and what submaps are for: higher scores and no larger errors on lap-closing pairs.
Inputs: tests/submap_reference.py (tests/test_submap_cpu.py holds their preconditions)."""
import ctypes as C
import math

import numpy as np
import pytest

from nautilus_amd import _lib, csm, hostside
from oracle import oracle as O
from tests import submap_reference as R

pytestmark = pytest.mark.gpu

DEG = math.radians(1.0)
CANARY = 4096  # floats behind the gathered cloud that no call may touch


class Device:
    """The crafted bag on the device and the calls on it (torch's current stream)."""

    def __init__(self):
        import torch
        self.torch, self.dev, self.lib = torch, torch.device("cuda:0"), _lib.load()
        self.sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        xy, off = R.packed()
        self.n_scans = len(off) - 1
        self.d_xy, self.d_off = self.up(xy), self.up(off)

    def up(self, a):
        return self.torch.from_numpy(np.array(a, order="C")).to(self.dev)  # (a copy: the shared inputs are read-only)

    def status(self):
        info = (C.c_int32 * 4)()
        return self.lib.nhip_dev_status(self.sp, info), list(info)

    def gather(self, member_scan, member_affine, member_offsets, capacity):
        """(rc of nhip_dev_status, info, cloud (capacity, 2), offsets, canary) of one launch over all targets."""
        torch = self.torch
        n_targets = len(member_offsets) - 1
        d_scan, d_aff, d_moff = self.up(np.asarray(member_scan, np.int32)), self.up(np.asarray(member_affine, np.float32)), self.up(np.asarray(member_offsets, np.int32))
        buf = torch.full((2 * capacity + CANARY,), -77.0, dtype=torch.float32, device=self.dev)
        d_goff = torch.full((n_targets + 1,), -5, dtype=torch.int32, device=self.dev)
        _lib.check(self.lib.nhip_submaps_gather_dev(self.d_xy.data_ptr(), self.d_off.data_ptr(), self.n_scans, d_scan.data_ptr(),
                                                    d_aff.data_ptr(), d_moff.data_ptr(), n_targets, buf.data_ptr(), capacity,
                                                    d_goff.data_ptr(), self.sp))
        rc, info = self.status()
        host = buf.cpu().numpy()
        self.last = (buf, d_goff)  # (the tables tests build from them)
        return rc, info, host[:2 * capacity].reshape(-1, 2), d_goff.cpu().numpy(), host[2 * capacity:]

    def build(self, d_xy, d_off, n_targets, spec, d_grids=None, d_ws=None, rebuild=False):
        """Raw slots (n_targets, slot_bytes) of nhip_grid_build_dev / _rebuild_dev over targets 0 .. n_targets - 1."""
        torch, lib = self.torch, self.lib
        L = csm.grid_layout(spec)
        nbytes, ws = lib.nhip_grids_bytes(C.byref(spec), n_targets), lib.nhip_grid_workspace_bytes(C.byref(spec), n_targets)
        if d_grids is None:
            d_grids = torch.full((nbytes,), 255, dtype=torch.uint8, device=self.dev)
            d_ws = torch.full((ws,), 255, dtype=torch.uint8, device=self.dev)
        d_ids = torch.arange(n_targets, dtype=torch.int32, device=self.dev)
        fn = lib.nhip_grid_rebuild_dev if rebuild else lib.nhip_grid_build_dev
        _lib.check(fn(d_xy.data_ptr(), d_off.data_ptr(), n_targets, d_ids.data_ptr(), n_targets, C.byref(spec), d_grids.data_ptr(),
                      d_ws.data_ptr(), ws, self.sp))
        rc, info = self.status()
        assert rc == _lib.NHIP_OK, info
        return d_grids[:n_targets * L.slot_bytes].cpu().numpy().reshape(n_targets, L.slot_bytes).copy(), d_grids, d_ws


@pytest.fixture(scope="module")
def device(gpu):
    return Device()


def small_spec(bits):
    return csm.grid_spec(R.RANGE_M, R.RES, R.SIGMA, 1e-10, R.MAX_SHIFT, bits)


# ------------------------------------------------------------------------------------------------ the gather
def test_gather_equals_the_restatement_in_one_launch(device):
    mxy, moff = R.merged()
    rc, info, cloud, off, canary = device.gather(*R.members(), capacity=len(mxy))
    assert rc == _lib.NHIP_OK, info
    assert np.array_equal(off, moff)
    assert R.same_cloud(cloud, mxy), "first differing point: %s" % np.nonzero((cloud.view(np.uint32) != mxy.view(np.uint32)).any(axis=1))[0][:5]
    assert np.all(canary == -77.0)
    # more room than needed: the same cloud, the rest untouched
    rc, info, cloud, off, canary = device.gather(*R.members(), capacity=len(mxy) + 3000)
    assert rc == _lib.NHIP_OK and np.array_equal(off, moff) and R.same_cloud(cloud[:len(mxy)], mxy)
    assert np.all(cloud[len(mxy):] == -77.0) and np.all(canary == -77.0)


def test_bad_member_ids_are_empty_members_and_reported(device):
    member_scan, aff, moff = R.members()
    xy, off = R.packed()
    bad = member_scan.copy()
    first, second = int(moff[2]), int(moff[3] + 4)  # a member of target 2, a member of target 3
    bad[first], bad[second] = -1, device.n_scans
    want_xy, want_off = hostside.submap_clouds(xy, off, bad, aff, moff)
    dropped = R.LENGTHS[member_scan[first]] + R.LENGTHS[member_scan[second]]
    assert want_off[-1] == R.merged()[1][-1] - dropped and dropped > 0
    rc, info, cloud, got_off, canary = device.gather(bad, aff, moff, capacity=len(R.merged()[0]))
    assert rc == _lib.NHIP_ERR_ARG and info[0] == 512 and info[1] == 512
    assert (info[2], info[3]) in ((-1, first), (device.n_scans, second))
    assert b"member scan id" in device.lib.nhip_last_error()
    assert np.array_equal(got_off, want_off)
    assert R.same_cloud(cloud[:len(want_xy)], want_xy), "bad members contribute nothing, every other target is unchanged"
    assert np.all(cloud[len(want_xy):] == -77.0) and np.all(canary == -77.0)
    assert device.status()[0] == _lib.NHIP_OK, "the record was consumed"


def test_a_capacity_one_point_short_stores_nothing(device):
    mxy, _ = R.merged()
    rc, info, cloud, off, canary = device.gather(*R.members(), capacity=len(mxy) - 1)
    assert rc == _lib.NHIP_ERR_ARG and info[0] == 1024 and info[2] == len(mxy), info
    assert b"out_capacity" in device.lib.nhip_last_error()
    assert np.all(off == 0), "every target comes back empty: a table build over the result reads nothing"
    assert np.all(cloud == -77.0) and np.all(canary == -77.0)
    assert device.status()[0] == _lib.NHIP_OK


# ------------------------------------------------------------------------------------------------ the tables
@pytest.mark.parametrize("bits", [16, 8])
def test_tables_of_the_gathered_cloud_are_the_tables_of_the_host_merged_cloud(device, bits):
    spec = small_spec(bits)
    L = csm.grid_layout(spec)
    assert L.side == 128
    mxy, moff = R.merged()
    n = len(moff) - 1
    rc, info, _, _, _ = device.gather(*R.members(), capacity=len(mxy))
    assert rc == _lib.NHIP_OK, info
    d_gxy, d_goff = device.last
    got, d_grids, d_ws = device.build(d_gxy, d_goff, n, spec)
    # the host-merged cloud uploaded as plain scans (non-finite points and all)
    want, _, _ = device.build(device.up(mxy), device.up(moff), n, spec)
    assert got.any() and np.array_equal(got, want)
    # the one-member identity target is the plain build of that scan
    scan8 = R.bag()[0][8]
    plain, _, _ = device.build(device.up(scan8), device.up(np.array([0, len(scan8)], np.int32)), 1, spec)
    assert np.array_equal(got[1], plain[0])
    # ... and the target without members the build of a scan without points
    empty, _, _ = device.build(device.up(np.zeros((1, 2), np.float32)), device.up(np.zeros(2, np.int32)), 1, spec)
    assert np.array_equal(got[0], empty[0])
    # a rebuild over these tables from a second set of submaps gives the fresh build's bytes
    xy, off = R.packed()
    mxy2, moff2 = hostside.submap_clouds(xy, off, *R.second_members())
    rc, info, cloud2, off2, _ = device.gather(*R.second_members(), capacity=len(mxy2))
    assert rc == _lib.NHIP_OK and np.array_equal(off2, moff2) and R.same_cloud(cloud2, mxy2)
    d_gxy2, d_goff2 = device.last
    rebuilt, _, _ = device.build(d_gxy2, d_goff2, n, spec, d_grids, d_ws, rebuild=True)
    fresh, _, _ = device.build(device.up(mxy2), device.up(moff2), n, spec)
    assert np.array_equal(rebuilt, fresh) and not np.array_equal(rebuilt, got)


# ------------------------------------------------------------------------------------------------ handle form
@pytest.mark.parametrize("bits", [16, 8])
def test_handle_form_matches_like_the_oracle_on_the_merged_clouds(gpu, bits):
    spec, ospec = small_spec(bits), O.grid_spec(R.RANGE_M, R.RES, R.SIGMA, 1e-10, bits)
    xy, off = R.packed()
    mxy, moff = R.merged()
    n = len(moff) - 1
    finite = np.isfinite(mxy).all(axis=1)
    # (the oracle's build takes finite points: the non-finite ones hit no cell on either side)
    clouds = [mxy[moff[t]:moff[t + 1]][finite[moff[t]:moff[t + 1]]] for t in range(n)]
    oxy, ooff = csm.pack_scans(clouds)
    ogr = O.grid_build_batch(oxy, ooff, np.arange(n), ospec)
    sources = [8, 11, 14, 7, 5]
    src = np.repeat(sources, n).astype(np.int32)
    slot = np.tile(np.arange(n), len(sources)).astype(np.int32)
    th0 = np.linspace(-0.05, 0.05, len(src))
    want = O.csm_match_batch(xy, off, ogr, ospec, src, slot, th0, O.search_spec(5, 25, 25, DEG))
    assert (want["sum"] > 0).sum() >= len(src) // 2
    st = csm.ScanTable(xy, off)
    grids = csm.LikelihoodGrids.from_submaps(st, *R.members(), spec)
    try:
        for t in (1, 3, 6, 7):
            assert np.array_equal(grids.interior(t), ogr[t]), "slot %d differs from the oracle's table of the merged cloud" % t
        got, sums = csm.match_pairs(st, grids, src, slot, th0, csm.search_spec(5, 25, 25, DEG))
        for f in ("itheta", "ix", "iy"):
            assert np.array_equal(got[f], want[f]), f
        assert np.array_equal(sums, want["sum"])
        vol = csm.score_volume(st, grids, 8, 3, 0.01, csm.search_spec(5, 25, 25, DEG))
        assert vol.max() == O.csm_match(R.bag()[0][8], ogr[3], ospec, 0.01, O.search_spec(5, 25, 25, DEG)).sum
        # ids are validated on the host
        bad = R.members()[0].copy()
        bad[2] = len(off) - 1
        with pytest.raises(_lib.NhipError):
            csm.LikelihoodGrids.from_submaps(st, bad, R.members()[1], R.members()[2], spec)
    finally:
        grids.close()
        st.close()


# ------------------------------------------------------------------------------------------------ the backend
@pytest.fixture(scope="module")
def lap_pairs():
    """SynthBag(480), its 50 lap-closing pairs: sources 380, 382, .. 478, each with a random target within 1.5 m of its
    true pose and more than 20 nodes away (np.random.default_rng(1)); theta0 from the odometry."""
    from nautilus_amd import synth
    bag = synth.SynthBag(480)
    rng = np.random.default_rng(1)
    idx = np.arange(bag.n_scans)
    src, tgt = [], []
    for s in range(380, 480, 2):
        d = np.linalg.norm(bag.truth[:, :2] - bag.truth[s, :2], axis=1)
        cand = idx[(d < 1.5) & (np.abs(idx - s) > 20)]
        src.append(s)
        tgt.append(int(rng.choice(cand)))
    src, tgt = np.array(src, dtype=np.int32), np.array(tgt, dtype=np.int32)
    assert np.all(src - tgt > 20), "a source is never in its target's submap"
    a = bag.odom[src, 2] - bag.odom[tgt, 2]
    xy, off = csm.pack_scans(bag.scans)
    return bag, xy, off, src, tgt, a - 2 * math.pi * np.rint(a / (2 * math.pi))


def test_backend_device_route_equals_host_merge_route(gpu, lap_pairs):
    from nautilus_amd import posegraph
    bag, xy, off, src, tgt, th0 = lap_pairs
    src, tgt, th0 = src[:12], tgt[:12], th0[:12]
    backend = posegraph.HipBackend()
    m_dev, spec, search = backend.match(xy, off, src, tgt, th0, 16, submap_radius=2, poses=bag.odom)
    xy_m, off_m, tgt_m = hostside.submap_extra_scans(xy, off, bag.odom, tgt, 2)
    m_host, _, _ = backend.match(xy_m, off_m, src, tgt_m, th0, 16)
    assert m_dev.tobytes() == m_host.tobytes()
    assert (m_dev["itheta"] >= 0).all() and np.isfinite(m_dev["score"]).all()


def test_submap_radius_zero_is_the_call_without_the_keyword(gpu, lap_pairs):
    from nautilus_amd import posegraph
    bag, xy, off, src, tgt, th0 = lap_pairs
    src, tgt, th0 = src[:12], tgt[:12], th0[:12]
    backend = posegraph.HipBackend()
    plain, _, _ = backend.match(xy, off, src, tgt, th0, 16)
    zero, _, _ = backend.match(xy, off, src, tgt, th0, 16, submap_radius=0, poses=bag.odom)
    none, _, _ = backend.match(xy, off, src, tgt, th0, 16, submap_radius=0)
    assert plain.tobytes() == zero.tobytes() == none.tobytes()
    with pytest.raises(ValueError):
        backend.match(xy, off, src, tgt, th0, 16, submap_radius=2)


def test_submaps_raise_the_scores_of_lap_closing_pairs(gpu, lap_pairs):
    """k = 5 against k = 0 on the 50 pairs: a higher mean score, no larger mean translation error (CPU oracle: -1.10 against
    -2.97, 0.038 m against 0.053 m) -- and the GPU's records are the oracle's on the merged clouds: indices from the backend's
    device route, indices and integer sums from the handle form over the whole bag."""
    from nautilus_amd import posegraph
    bag, xy, off, src, tgt, th0 = lap_pairs
    backend = posegraph.HipBackend()
    gs, ss = O.grid_spec(30.0, 0.05, 2.0, 1e-10, 16), O.search_spec(61, 81, 81, DEG)
    truth = np.array([bag.true_relative(s, t) for s, t in zip(src, tgt)])
    targets = np.unique(tgt)
    slot = np.searchsorted(targets, tgt).astype(np.int32)
    st = csm.ScanTable(xy, off)
    figures = {}
    try:
        for k in (0, 5):
            member_scan, member_offsets = hostside.submap_members(bag.n_scans, targets, k)
            aff = csm.submap_member_affines(bag.odom, np.repeat(targets, np.diff(member_offsets)), member_scan)
            mxy, moff = hostside.submap_clouds(xy, off, member_scan, aff, member_offsets)
            if k == 0:
                assert np.array_equal(moff, np.concatenate([[0], np.cumsum(off[targets + 1] - off[targets])]))
            ogr = O.grid_build_batch(mxy, moff, np.arange(len(targets)), gs)
            want = O.csm_match_batch(np.concatenate([xy, mxy]), np.concatenate([off, off[-1] + moff[1:]]).astype(np.int32), ogr, gs,
                                     src, slot, th0, ss)
            m, spec, search = backend.match(xy, off, src, tgt, th0, 16, submap_radius=k, poses=bag.odom)
            grids = csm.LikelihoodGrids.from_submaps(st, member_scan, aff, member_offsets, csm.grid_spec(30.0, 0.05, 2.0, 1e-10, 40, 16))
            try:
                h, sums = csm.match_pairs(st, grids, src, slot, th0, csm.search_spec(61, 81, 81, DEG))
            finally:
                grids.close()
            for f in ("itheta", "ix", "iy"):
                assert np.array_equal(m[f], want[f]) and np.array_equal(h[f], want[f]), (k, f)
            assert np.array_equal(sums, want["sum"]), k
            assert m.tobytes() == h.tobytes(), k
            tx = (m["ix"].astype(np.float64) - (search.nx - 1) // 2) * spec.res
            ty = (m["iy"].astype(np.float64) - (search.ny - 1) // 2) * spec.res
            th = th0 + (m["itheta"].astype(np.float64) - (search.n_theta - 1) // 2) * search.theta_step
            err_t = np.hypot(tx - truth[:, 0], ty - truth[:, 1])
            err_r = np.degrees(np.abs(th - truth[:, 2]))
            figures[k] = (float(m["score"].mean()), float(err_t.mean()), float(err_t.max()), float(err_r.mean()), int((err_t > 0.1).sum()))
            print("k = %d: mean score %.3f, translation error mean %.4f / max %.4f m, rotation error mean %.3f deg, "
                  "%d pairs worse than 0.1 m" % ((k,) + figures[k]))
    finally:
        st.close()
    assert figures[5][0] > figures[0][0], "mean score"
    assert figures[5][1] <= figures[0][1], "mean translation error"
