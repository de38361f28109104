"""Match refinement without a device: the rule's restatement (tests/refine_reference.py) reaches the sub-cell poses the issue
measured, flags the corridor, is told apart from three wrong rules by the case list, and equals the vectorised host form
(hostside.refine_icp) bit for bit; nhip_refine_start_poses equals its Python mirror bit for bit (it needs no device)."""
import ctypes as C
import math

import numpy as np
import pytest

from nautilus_amd import _lib, csm, hostside, refine, synth
from oracle import oracle as O
from tests import refine_reference as R

CASE_NAMES = [c.name for c in R.cases()]


def same_bytes(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@pytest.fixture(scope="module")
def protocol():
    """The issue's protocol: SynthBag(240, dense=True), 60 pairs, the oracle's 16-bit tables, the lattice argmax in the
    9 x 9 x 9 neighbourhood of the truth (the lattice itself anchored at sample_pairs' theta0 and at whole cells), the bag's
    normals.  Returns what the quality test compares."""
    bag = synth.SynthBag(240, dense=True)
    targets = np.arange(0, 240, 8)
    src, tgt, theta0 = bag.sample_pairs(per_target=2, targets=targets)
    assert len(src) == 60
    xy, off = csm.pack_scans(bag.scans)
    normals = np.concatenate(bag.normals).astype(np.float32)
    ospec, step = O.grid_spec(), math.radians(1.0)
    grids = O.grid_build_batch(xy, off, targets, ospec)
    truth = np.array([bag.true_relative(s, t) for s, t in zip(src, tgt)])
    centre = theta0 + np.rint((truth[:, 2] - theta0) / step) * step
    origin = np.rint(truth[:, :2] / 0.05).astype(np.int32)
    search = csm.search_spec(9, 9, 9, step)
    rec = O.csm_match_batch(xy, off, grids, ospec, src, np.searchsorted(targets, tgt), centre, O.search_spec(9, 9, 9, step), pair_origin=origin)
    records = np.zeros(len(src), csm.MATCH_DTYPE)
    for f in ("itheta", "ix", "iy"):
        records[f] = rec[f]
    pose0 = hostside.refine_start_poses(records, centre, csm.grid_spec(), search, origin)
    refined, _ = R.refine(xy, normals, off, src, tgt, pose0)
    return truth, pose0, refined


def errors(truth, c, s, tx, ty):
    dt = np.hypot(tx - truth[:, 0], ty - truth[:, 1])
    dr = np.arctan2(s, c) - truth[:, 2]
    dr = np.abs(dr - 2 * math.pi * np.rint(dr / (2 * math.pi)))
    return math.sqrt(np.mean(dt ** 2)), dt.max(), math.degrees(math.sqrt(np.mean(dr ** 2))), math.degrees(dr.max())


def test_restatement_reaches_sub_cell_poses(protocol):
    truth, pose0, refined = protocol
    assert np.all((refined["flags"] & ~np.uint32(R.NOT_CONVERGED)) == 0), refined["flags"]
    lat = errors(truth, pose0[:, 0], pose0[:, 1], pose0[:, 2], pose0[:, 3])
    ref = errors(truth, refined["c"], refined["s"], refined["tx"], refined["ty"])
    print("lattice: rms %.4f m max %.4f m rms %.3f deg max %.3f deg" % lat)
    print("refined: rms %.4f m max %.4f m rms %.4f deg max %.4f deg" % ref)
    print("iterations min/median/max: %d/%d/%d" % (refined["iterations"].min(), np.median(refined["iterations"]), refined["iterations"].max()))
    assert ref[0] <= lat[0] / 5 and ref[2] <= lat[2] / 5
    assert np.all(refined["n_corr"] >= 30) and np.all(refined["cost"] > 0) and np.all(refined["info"][:, 0] > 0)


def test_corridor_is_singular_and_keeps_pose0():
    cs = R.case("corridor")
    out, trace = R.reference("corridor")
    assert out["flags"][0] == R.SINGULAR and out["iterations"][0] == 0
    assert same_bytes([out["c"][0], out["s"][0], out["tx"][0], out["ty"][0]], cs.pose0[0])
    assert out["n_corr"][0] == 0 and out["cost"][0] == 0 and not out["info"].any() and not trace.any()


def test_every_flag_and_the_plain_end_occur():
    seen = {name: int(R.reference(name)[0]["flags"][0]) for name in
            ("src2048", "tgt2049", "few", "corridor", "equal_normals", "runaway", "skipped", "iter1", "tgt29", "tgt30", "one_update")}
    assert seen["tgt2049"] == R.TARGET_TOO_LONG and seen["few"] == R.FEW and seen["runaway"] == R.RUNAWAY
    assert seen["corridor"] == R.SINGULAR and seen["equal_normals"] == R.SINGULAR and seen["skipped"] == R.SKIPPED
    assert seen["iter1"] == R.NOT_CONVERGED and seen["src2048"] == 0
    assert seen["tgt29"] == R.FEW and seen["tgt30"] in (0, R.NOT_CONVERGED)
    assert np.isnan(R.reference("skipped")[0]["c"][0])
    assert R.reference("one_update")[0]["iterations"][0] == 1 and R.reference("iter16")[0]["iterations"][0] == 16
    assert R.reference("iter8")[0]["iterations"][0] == 8


@pytest.mark.parametrize("name", CASE_NAMES)
def test_host_form_equals_the_restatement(name):
    cs = R.case(name)
    want, want_trace = R.reference(name)
    got, got_trace = hostside.refine_icp(cs.xy, cs.normals, cs.offsets, cs.pair_src, cs.pair_tgt, cs.pose0, cs.fields())
    assert same_bytes(got, want) and same_bytes(got_trace, want_trace)


def _first_evaluation(cs, p):
    """Pair p of a case as K22's first evaluation searches it: (queries, NaN where the source point takes no part; the target
    points that are staged; thr[0]), or None where the kernel ends before it searches (start pose, target length)."""
    s, t = int(cs.pair_src[p]), int(cs.pair_tgt[p])
    src, tgt = cs.xy[cs.offsets[s]:cs.offsets[s + 1]], cs.xy[cs.offsets[t]:cs.offsets[t + 1]]
    if not np.isfinite(cs.pose0[p]).all() or len(tgt) > R.TARGET_MAX:
        return None
    c, s_, tx, ty = (np.float32(v) for v in cs.pose0[p])
    with np.errstate(all="ignore"):
        q = np.stack([(c * src[:, 0] + (-s_) * src[:, 1]) + tx, (s_ * src[:, 0] + c * src[:, 1]) + ty], axis=1)
        q[~(np.abs(src) < np.float32(1.0e6)).all(axis=1)] = np.nan
        staged = tgt[(np.abs(tgt) < np.float32(1.0e6)).all(axis=1)]
    assert q.dtype == np.float32
    return q, staged, cs.fields().thr[0]


def test_the_cases_reach_the_seams_of_the_shared_walk():
    """K22 runs nhip_corr_shared.h's walk with its own staging rule and no gate.  By the path conditions tests/corr_seams.py
    restates, at thr[0] and over the first evaluation of every case: the queries that WALK visit one run (icx & 3 in 1, 2) and
    two runs (0, 3) with icx and icy on both sides of zero at every residue; the list holds hashed targets, a target that is
    searched exhaustively for a point of its own (far_target) and one for a query (far_pose).  A precondition: an edit of the
    cases that stops reaching a seam fails here, not silently on the device."""
    from tests import corr_seams as S
    walked, path = [], {}
    for cs in R.cases():
        for p in range(len(cs.pair_src)):
            ev = _first_evaluation(cs, p)
            if ev is None:
                continue
            q, staged, thr = ev
            is_hashed = S.hashed(staged, thr)
            scans = S.scan_everything_passes(q, staged, thr)
            path.setdefault(cs.name, []).append((is_hashed, scans))
            for k, scan_all in enumerate(scans):
                if not scan_all:
                    part = q[k * S.PASS:(k + 1) * S.PASS]
                    walked.append(S.cells(part[~np.isnan(part).any(axis=1)], thr))
            if is_hashed and len(staged):
                tc = S.cells(staged, thr)
                assert np.all(S.bucket(tc[:, 0], tc[:, 1]) < S.BUCKETS)
    cells = np.concatenate(walked)
    icx, icy, two = cells[:, 0], cells[:, 1], S.two_runs(cells[:, 0])
    assert set(icx[two] & 3) == {0, 3} and set(icx[~two] & 3) == {1, 2}
    for r in range(4):
        at = (icx & 3) == r
        assert (icx[at] < 0).any() and (icx[at] >= 0).any() and (icy[at] < 0).any() and (icy[at] >= 0).any(), r
    assert path["far_target"] == [(False, [True])] and path["far_pose"] == [(True, [True])]
    assert path["src4100"] == [(True, [False] * 3)] and path["tgt2048"] == [(True, [False])] and all(h for h, _ in path["pairs300"])
    assert "tgt2049" not in path and "skipped" not in path
    print("refine cases: %d walked queries, %d two-run, cells x %d..%d y %d..%d; hashed pairs %d, exhaustive by target %d, by query %d" % (
        len(cells), two.sum(), icx.min(), icx.max(), icy.min(), icy.max(), sum(h for v in path.values() for h, _ in v),
        sum(not h for v in path.values() for h, _ in v), sum(h and any(s) for v in path.values() for h, s in v)))


def test_threshold_edge_keeps_the_distance_below_alone():
    """Of the three lone points at 0.25 m minus one float, 0.25 m and 0.25 m plus one float, the first evaluation (identity
    pose: q = p exactly) keeps the first alone."""
    cs = R.case("threshold_edge")
    a, b = cs.offsets[0], cs.offsets[1]
    src, tgt, tgn = cs.xy[a:b], cs.xy[b:], cs.normals[b:]
    _, n_all = R.evaluate(src, tgt, tgn, (1.0, 0.0, 0.0, 0.0), np.float32(0.25))
    _, n_room = R.evaluate(src[:-3], tgt, tgn, (1.0, 0.0, 0.0, 0.0), np.float32(0.25))
    _, n_first = R.evaluate(src[-3:-2], tgt, tgn, (1.0, 0.0, 0.0, 0.0), np.float32(0.25))
    assert n_first == 1 and n_all == n_room + 1


@pytest.mark.parametrize("perturb", [dict(thr_shift=1), dict(ties="highest"), dict(butterfly=False)], ids=["threshold", "ties", "sum"])
def test_a_wrong_rule_leaves_the_reference(perturb):
    """A threshold one table slot off, ties to the highest index and a sequential sum of the lane sums each move a case off
    the reference: the byte comparison of the device is a test of these choices."""
    names = {"thr_shift": ("iter8", "src2048"), "ties": ("duplicates",), "butterfly": ("src2048", "iter8")}[next(iter(perturb))]
    moved = 0
    for name in names:
        cs = R.case(name)
        got, trace = R.refine(cs.xy, cs.normals, cs.offsets, cs.pair_src, cs.pair_tgt, cs.pose0, cs.fields(), **perturb)
        moved += not (same_bytes(got, R.reference(name)[0]) and same_bytes(trace, R.reference(name)[1]))
    assert moved == len(names)


def test_start_poses_in_c_equal_the_python_mirror():
    rng = np.random.default_rng(5)
    n = 500
    records = np.zeros(n, csm.MATCH_DTYPE)
    records["itheta"], records["ix"], records["iy"] = rng.integers(0, 61, n), rng.integers(0, 81, n), rng.integers(0, 81, n)
    records["itheta"][::17] = -1
    theta0 = rng.uniform(-math.pi, math.pi, n)
    origin = rng.integers(-40, 41, (n, 2)).astype(np.int32)
    gspec, search = csm.grid_spec(), csm.search_spec(61, 81, 81, math.radians(1.0))
    for org in (None, origin):
        got = refine.start_poses(records, theta0, gspec, search, org)
        want = hostside.refine_start_poses(records, theta0, gspec, search, org)
        assert same_bytes(got, want)
        assert np.isnan(got[::17]).all() and np.isfinite(np.delete(got, np.s_[::17], axis=0)).all()


def test_loop_on_a_backend_without_the_method_takes_the_host_route():
    """examples/slam_loop.py's lc_refine on the CPU backend (no refine_matches: hostside.refine_matches serves it): every closure
    refined, their relative error a fifth of the lattice's or below, nothing else of the result touched before the closures."""
    import examples.slam_loop as loop
    from oracle.cpu_backend import OracleBackend
    from tests import loss_loop as LL
    assert not hasattr(OracleBackend, "refine_matches")
    plain = loop.run(backend=OracleBackend(), **LL.KW)
    got = loop.run(backend=OracleBackend(), lc_refine="icp", **LL.KW)
    print({k: (plain.get(k), got[k]) for k in ("lc_accepted", "lc_rel_err_m", "err_lc_m", "lc_refined", "lc_refine_flags")})
    assert sorted(set(got) - set(plain)) == ["lc_refine_flags", "lc_refined", "refine_s"]
    assert got["lc_accepted"] == plain["lc_accepted"] == got["lc_refined"] > 5
    assert all(v == 0 for k, v in got["lc_refine_flags"].items() if k != "NOT_CONVERGED")
    assert got["lc_rel_err_m"] <= plain["lc_rel_err_m"] / 5
    for k in ("err_odometry_m", "err_icp_m", "lc_candidates", "icp_correspondences"):
        assert got[k] == plain[k], k
    with pytest.raises(ValueError):
        loop.run(backend=OracleBackend(), lc_refine="icp", world=2, **LL.KW)
    with pytest.raises(ValueError):
        loop.run(backend=OracleBackend(), lc_refine="quadratic", **LL.KW)


def test_spec_defaults_and_struct_sizes():
    s, f = refine.default_spec(), hostside.RefineFields()
    assert C.sizeof(_lib.RefineSpec) == 144 and C.sizeof(_lib.Refined) == 104 == hostside.REFINED_DTYPE.itemsize
    for name in ("thr0", "shrink", "thr_min", "step_tol_m", "step_tol_rad", "min_spread", "max_shift_m", "max_turn_sin",
                 "max_iterations", "min_corr", "flags", "reserved"):
        assert getattr(s, name) == getattr(f, name), name
    assert same_bytes(np.array(list(s.thr), np.float32), f.thr)
    assert list(s.thr)[:5] == [0.25, 0.125, 0.0625, np.float32(0.05), np.float32(0.05)]
    s2 = refine.spec(thr0=0.2, max_iterations=4)
    assert same_bytes(np.array(list(s2.thr), np.float32), hostside.refine_thresholds(0.2, 0.5, 0.05)) and s2.max_iterations == 4
    lib, out = _lib.load(), np.zeros(1, hostside.REFINED_DTYPE)
    for bad in (refine.spec(max_iterations=0), refine.spec(max_iterations=17), refine.spec(min_corr=2), refine.spec(shrink=2.0)):
        rc = lib.nhip_refine_icp_dev(None, None, None, 0, None, None, None, 0, C.byref(bad), _lib.ptr(out), None, None)
        assert rc == _lib.NHIP_ERR_ARG
    t = refine.to_transform(R.reference("src2048")[0])
    assert same_bytes(t, hostside.refined_to_transform(R.reference("src2048")[0]))
