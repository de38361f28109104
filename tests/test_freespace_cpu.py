"""The free-space check without a GPU ("Free-space check"): the numpy reference on hand-listed rays and
against the occupancy grid's reference, the host path (hostside.freespace_counts) against it on every crafted case, the
quality the gate's default rests on, the entry points' argument checks, and the example loop's --lc-verify on the CPU backend."""
import ctypes as C
import math

import numpy as np
import pytest

from nautilus_amd import _lib, csm, freespace, hostside, synth
from tests import freespace_reference as R
from tests import occupancy_reference as OR


def test_rdiv_is_a_floor_division_on_hand_listed_rays():
    """Halves round UP on both signs, so the rays to (4, 2) and (-4, -2) are not mirror images."""
    assert R.ray(4, 2) == [(0, 0), (1, 1), (2, 1), (3, 2)]
    assert R.ray(-4, -2) == [(0, 0), (-1, 0), (-2, -1), (-3, -1)]
    assert R.ray(2, 4) == [(0, 0), (1, 1), (1, 2), (2, 3)] and R.ray(-2, -4) == [(0, 0), (0, -1), (-1, -2), (-1, -3)]
    assert R.ray(0, 0) == [] and R.ray(3, 0) == [(0, 0), (1, 0), (2, 0)] and R.ray(0, -2) == [(0, 0), (0, -1)]
    # ... and the plane of those six beams, cell by cell (sensor at (60, 60); an end cell is never free)
    want = {(60, 60), (61, 61), (62, 61), (63, 62), (59, 60), (58, 59), (57, 59), (61, 62), (62, 63), (60, 59), (59, 58), (59, 57),
            (61, 60), (62, 59), (63, 59), (59, 61), (58, 61), (57, 62)}
    got = R.free_plane(R.plane_cases()["sign_asymmetry"], R.SIDE, R.RES)
    ys, xs = np.nonzero(got)
    assert set(zip(xs.tolist(), ys.tolist())) == want


@pytest.mark.parametrize("name", ["bag", "points_1081", "rims_and_corners", "end_on_another_beam"])
def test_free_plane_is_the_occupancy_references_scan_at_the_identity(name, small_bag):
    """One scan's F equals occupancy_reference.scan_sets at the identity pose, cut to the grid, minus the hits (every point of
    these scans lies inside the grid: a point outside it gives no ray here, but a beam there)."""
    if name == "bag":
        pts, side, res = small_bag.scans[7], 1200, 0.05
    else:
        pts, side, res = R.plane_cases()[name], R.SIDE, R.RES
    half = side // 2
    H, F, _ = OR.scan_sets(pts, (1.0, 0.0, 0.0, 0.0), OR.make_spec(res=res, max_ray_cells=4096))
    assert len(H) and (np.abs(H) <= half).all(), "the comparison needs every end cell inside the grid"
    cut = lambda c: c[(c >= -half).all(axis=1) & (c < side - half).all(axis=1)]
    want = np.zeros((side, side), np.uint8)
    f = cut(F)
    want[f[:, 1] + half, f[:, 0] + half] = 1
    h = cut(H)
    want[h[:, 1] + half, h[:, 0] + half] = 0
    assert want.sum() > 0 and np.array_equal(R.free_plane(pts, side, res), want)


@pytest.mark.parametrize("case", R.check_cases(), ids=lambda c: c["name"])
def test_host_path_equals_the_reference(case):
    for fs in case["fs"]:
        want = R.case_counts(case, fs)
        got = R.case_counts(case, fs, hostside.freespace_counts)
        assert got.dtype == np.int32 and np.array_equal(got, want), (case["name"], fs)
        live = want[:, 0] >= 0
        assert (want[live, 1:6].sum(axis=1) == want[live, 0]).all() and (want[~live] == -1).all()
        assert (want[live, 6] <= want[live, 3:6].sum(axis=1)).all() and (want[:, 7][live] == 0).all()


def test_crafted_cases_reach_what_they_are_for():
    """The cases are only worth their name if the reference's answers show the effect they were built for."""
    by = {c["name"]: c for c in R.check_cases()}
    c = by["hit_wins_over_free"]
    r0, r1 = R.case_counts(c, (0, 0))[0], R.case_counts(c, (1, 0))[0]
    assert r0[3] == 1 and r0[4] == 5 and r1[3] == 5 and r1[4] == 2  # the free cells beside the wall turn into hits
    t = by["through_margins"]
    assert [int(R.case_counts(t, fs)[0][6]) for fs in ((0, 0), (0, 3), (0, 64))] == [4, 2, 0]
    s = R.case_counts(by["shift_out_of_the_grid"], (2, 3))
    assert s[0, 2] == 0 and 0 < s[1, 2] < s[3, 2] < 300 and (s[8:, 2] == 300).all() and (s[8:, 3:7] == 0).all()
    o = R.case_counts(by["through_rays_outside"], (0, 0))
    assert o[0, 6] == 1 and o[0, 2] == 5 and o[2, 2] == 7
    d = R.case_counts(by["dropped_and_far"], (2, 3))
    assert d[0, 1] == 3 and d[1, 1] == 4 and d[0, 2] >= 5  # (3.4e38, 3.4e38) overflows only once it is rotated
    b = by["bit_offsets_and_rim"]
    hits = [int(R.case_counts(b, (r, 3))[0][3]) for r in (0, 1, 2, 16)]
    assert hits[0] < hits[1] < hits[2] < hits[3]
    rot = R.case_counts(by["rotations_61"], (2, 3))
    assert len(np.unique(rot, axis=0)) >= 55


def test_spec_defaults_and_argument_checks_need_no_device():
    lib = _lib.load()
    s = freespace.default_spec()
    assert (s.hit_radius, s.end_margin, s.flags, s.reserved) == (2, 3, 0, 0) and C.sizeof(s) == 16
    assert freespace.spec(hit_radius=16, end_margin=0).hit_radius == 16
    with pytest.raises(TypeError):
        freespace.spec(radius=1)
    grid, search = R.small_grid_spec(), csm.search_spec(1, 1, 1)
    L = csm.grid_layout(grid)
    assert freespace.planes_bytes(grid, 3) == 3 * L.hits_bytes and freespace.planes_bytes(grid, 0) == 0
    # side / 2 > 4096: the ray's int32 bound (a grid the matcher itself admits)
    big = csm.grid_spec(41.0, 0.01, 2.0, 1e-10, 8)
    assert csm.grid_layout(big).side == 8200
    with pytest.raises(_lib.NhipError, match="4096"):
        freespace.planes_bytes(big, 1)
    assert freespace.planes_bytes(csm.grid_spec(40.96, 0.01, 2.0, 1e-10, 8), 1) > 0  # side 8192: the largest admitted
    rc = lib.nhip_freespace_trace_dev(None, None, 0, None, 0, C.byref(big), None, None, None)
    assert rc == _lib.NHIP_ERR_ARG and b"4096" in lib.nhip_last_error()
    bad = [dict(hit_radius=-1), dict(hit_radius=17), dict(end_margin=-1), dict(end_margin=65), dict(flags=1), dict(reserved=2)]
    for kw in bad:
        rc = lib.nhip_freespace_check_dev(None, None, 0, None, 0, C.byref(grid), None, None, None, None, None, 0, C.byref(search),
                                          None, None, C.byref(freespace.spec(**kw)), None, None)
        assert rc == _lib.NHIP_ERR_ARG and next(iter(kw)) in lib.nhip_last_error().decode(), kw
        rc = lib.nhip_csm_freespace(None, None, None, None, None, None, 0, C.byref(search), None, C.byref(freespace.spec(**kw)), None)
        assert rc == _lib.NHIP_ERR_ARG, kw
    rc = lib.nhip_freespace_check_dev(None, None, 0, None, 0, C.byref(grid), None, None, None, None, None, 0,
                                      C.byref(csm.search_spec(0, 1, 1)), None, None, C.byref(s), None, None)
    assert rc == _lib.NHIP_ERR_ARG
    with pytest.raises(ValueError):
        hostside.freespace_counts(np.zeros((0, 2)), [0], [], [], [], R.records([]), grid, search, R.make_spec(hit_radius=17))


def test_keep_is_an_integer_gate():
    c = np.array([[100, 0, 0, 80, 10, 10, 10, 0],    # 20 of 100: exactly 200 permille -> kept
                  [100, 0, 0, 80, 10, 10, 11, 0],    # 21 of 100
                  [100, 10, 90, 0, 0, 0, 0, 0],      # nothing inside the grid: nothing contradicts it
                  [-1] * 8,                          # a rejected record is not kept
                  [1000, 0, 0, 0, 1, 999, 199, 0]], np.int32)
    assert freespace.keep(c).tolist() == [True, False, True, False, True]
    assert freespace.keep(c, 210).tolist() == [True, True, True, False, True]
    assert freespace.keep(c, 0).tolist() == [False, False, True, False, False]
    assert freespace.DEFAULT_MAX_PERMILLE == 200
    share = freespace.violation_share(c)
    assert share[0] == 0.2 and share[2] == 0.0 and np.isnan(share[3])
    with pytest.raises(ValueError):
        freespace.keep(c, 1001)


def quality_pairs():
    """SynthBag(320), two sources within 1.5 m of every 16th scan: each pair's truth pose rounded to the 5 cm / 1 degree lattice,
    and the same pose 1 m (in a seeded direction) and 10 degrees (seeded sign) off.  The poses are carried by pair_origin."""
    bag = synth.SynthBag(320)
    src, tgt, th0 = bag.sample_pairs(per_target=2, max_dist=1.5, targets=np.arange(0, 320, 16))
    spec, search = csm.grid_spec(30.0, 0.05, 2.0, 1e-10, 40, 16), csm.search_spec(61, 81, 81, math.radians(1.0))
    rel = np.array([bag.true_relative(s, t) for s, t in zip(src, tgt)])
    rng = np.random.default_rng(5)
    a, sign = rng.uniform(0, 2 * math.pi, len(src)), rng.choice([-10, 10], len(src))
    wrong = rel + np.stack([np.cos(a), np.sin(a), np.zeros(len(a))], axis=1)
    k = np.rint((rel[:, 2] - th0) / search.theta_step).astype(int) + 30
    right_pose = (R.records([(v, 40, 40) for v in k]), np.rint(rel[:, :2] / spec.res).astype(np.int32))
    wrong_pose = (R.records([(v, 40, 40) for v in k + sign]), np.rint(wrong[:, :2] / spec.res).astype(np.int32))
    return csm.pack_scans(bag.scans), src, tgt, th0, spec, search, right_pose, wrong_pose


def test_quality_on_synthetic_bag():
    """What the gate's default rests on, measured on the reference alone: every pair's share of contradicted returns is larger
    at its wrong pose than at its right one, and the two populations do not meet.  Measured: 40 pairs, the largest right share
    0.0574, the smallest wrong share 0.4261 (DESIGN.md records both); the default of 200 permille lies between."""
    (xy, off), src, tgt, th0, spec, search, right_pose, wrong_pose = quality_pairs()
    assert len(src) == 40
    right = R.counts(xy, off, src, tgt, th0, right_pose[0], spec, search, None, right_pose[1])
    wrong = R.counts(xy, off, src, tgt, th0, wrong_pose[0], spec, search, None, wrong_pose[1])
    sr, sw = np.array([R.share(c) for c in right]), np.array([R.share(c) for c in wrong])
    print("largest right share %.4f, smallest wrong share %.4f" % (sr.max(), sw.min()))
    assert (sw > sr).all() and sr.max() < sw.min()
    assert sr.max() < freespace.DEFAULT_MAX_PERMILLE / 1000.0 < sw.min()
    assert abs(sr.max() - 0.0574) < 5e-4 and abs(sw.min() - 0.4261) < 5e-4, "DESIGN.md records these values"
    assert freespace.keep(right).all() and not freespace.keep(wrong).any()
    assert np.array_equal(hostside.freespace_counts(xy, off, src, tgt, th0, right_pose[0], spec, search, None, right_pose[1]), right)


def test_the_loop_verifies_its_records_on_the_cpu_backend():
    """examples/slam_loop.py --lc-verify free-space with a backend whose match() has no `freespace` parameter (the oracle's):
    the records are checked by hostside.freespace_counts; what the check keeps and what it rejects are the unverified run's
    accepted records."""
    import inspect
    import examples.slam_loop as loop
    from oracle.cpu_backend import OracleBackend
    assert "freespace" not in inspect.signature(OracleBackend().match).parameters
    kw = dict(n_scans=32, window=3, spacing=0.06, hitl=False, gate="geometric", iterations=2)
    plain = loop.run(backend=OracleBackend(), **kw)
    assert plain["lc_accepted"] > 20 and "lc_verified" not in plain
    for permille in (None, 5):
        out = loop.run(backend=OracleBackend(), lc_verify="free-space", lc_max_violation=permille, **kw)
        assert out["lc_verify"] == "free-space" and out["lc_max_violation"] == (200 if permille is None else permille)
        assert out["lc_verified"] + out["lc_verify_rejected"] == plain["lc_accepted"] and out["lc_accepted"] == out["lc_verified"]
        if permille is None:
            assert out["lc_verify_rejected"] == 0 and out["lc_verify_rejected_rel_err_m"] is None
            assert out["lc_rel_err_m"] == plain["lc_rel_err_m"]
        else:
            assert 0 < out["lc_verify_rejected"] and out["lc_verify_rejected_rel_err_m"] > 0 and out["lc_rel_err_m"] > 0
    for bad in (dict(lc_verify="free-space", lc_submap=2), dict(lc_verify="free-space", world=2), dict(lc_verify="covariance"),
                dict(lc_verify="free-space", lc_max_violation=1001)):
        with pytest.raises(ValueError):
            loop.run(backend=OracleBackend(), **dict(kw, **bad))
