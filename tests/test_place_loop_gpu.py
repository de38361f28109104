"""The appearance gate inside HipBackend and the example loop ("Place descriptors"): the device's records equal
the host path's, the heading they give serves the matcher as well as the odometry's, --lc-gate appearance proposes the same
pairs on the product as on the oracle's CPU backend, and under heading drift it closes loops the pose-based theta0 loses."""
import math

import numpy as np
import pytest

from nautilus_amd import csm, hostside, place, posegraph, synth

pytestmark = pytest.mark.gpu

KW = dict(n_scans=32, window=3, spacing=0.06, hitl=False, gate="geometric", iterations=2)  # (the other loop tests' bag)
SEED = 20201114                                                                           # (run()'s default)


def angle_mod(a):
    return a - 2 * math.pi * np.rint(a / (2 * math.pi))


def test_place_candidates_equal_the_host_path_and_give_the_matcher_its_theta0(gpu):
    bag = synth.SynthBag(KW["n_scans"], dense=True, seed=SEED, spacing=KW["spacing"])
    xy, off = csm.pack_scans(bag.scans)
    backend = posegraph.HipBackend()
    ids = np.arange(KW["n_scans"], dtype=np.int32)
    for kw in (dict(min_separation=20, flags=place.NHIP_PLACE_PAST_ONLY), dict(min_separation=3, top_k=8, max_permille=300)):
        sp = place.spec(**kw)
        rec, stats = backend.place_candidates(xy, off, ids, sp)
        want_rec, want_stats = hostside.place_candidates(xy, off, ids, sp)
        assert rec.tobytes() == want_rec.tobytes() and stats.tobytes() == want_stats.tobytes()
    sub = ids[[0, 3, 4, 9, 25, 30, 31]]  # (only the listed scans are uploaded: the others keep their ids)
    assert backend.place_candidates(xy, off, sub, sp)[0].tobytes() == hostside.place_candidates(xy, off, sub, sp)[0].tobytes()
    # pairs both gates propose: the appearance records among the geometric gate's (every pair of this bag more than 20 apart)
    rec, _ = backend.place_candidates(xy, off, ids, place.spec(min_separation=20, flags=place.NHIP_PLACE_PAST_ONLY))
    src, tgt, th_place = place.pairs(ids, rec)
    near = np.linalg.norm(bag.odom[src, :2] - bag.odom[tgt, :2], axis=1) < 3.5
    assert near.all() and len(src) == 45 and (src - tgt > 20).all()
    th_odom = angle_mod(bag.odom[src, 2] - bag.odom[tgt, 2])
    m_p, spec, search = backend.match(xy, off, src, tgt, th_place, 16)
    m_o, _, _ = backend.match(xy, off, src, tgt, th_odom, 16)
    # Both optima lie inside their windows, so each heading is the lattice point nearest the one optimum: the two lattices (one
    # step wide, offset by the difference of the two theta0) put them within one step of each other.  One step of heading moves
    # a point at range r by r * step: the translations agree to that, at the scan's mean range, plus a cell for each rounding.
    for m in (m_p, m_o):
        assert (np.abs(m["itheta"] - 30) < 30).all() and (np.abs(m["ix"] - 40) < 40).all() and (np.abs(m["iy"] - 40) < 40).all()
    heading_p = th_place + (m_p["itheta"] - 30) * search.theta_step
    heading_o = th_odom + (m_o["itheta"] - 30) * search.theta_step
    steps = np.abs(angle_mod(heading_p - heading_o)) / search.theta_step
    mean_range = np.array([np.linalg.norm(xy[off[s]:off[s + 1]], axis=1).mean() for s in src])
    cells = np.ceil(mean_range * search.theta_step / spec.res) + 2
    print("heading difference in steps: max %.2f; cells: max |dix| %d |diy| %d against %s" % (
        steps.max(), np.abs(m_p["ix"] - m_o["ix"]).max(), np.abs(m_p["iy"] - m_o["iy"]).max(), cells.min()))
    assert (steps <= 1.0 + 1e-9).all()
    assert (np.abs(m_p["ix"] - m_o["ix"]) <= cells).all() and (np.abs(m_p["iy"] - m_o["iy"]) <= cells).all()


def test_the_loop_proposes_on_the_device_what_the_host_path_proposes(gpu):
    import examples.slam_loop as loop
    from oracle.cpu_backend import OracleBackend
    dev = loop.run(lc_gate="appearance", **KW)
    host = loop.run(backend=OracleBackend(), lc_gate="appearance", **KW)
    assert dev["backend"] == "hip" and dev["lc_gate"] == host["lc_gate"] == "appearance" and dev["place_s"] > 0
    assert dev["lc_pairs"] == host["lc_pairs"] and len(dev["lc_pairs"]) == dev["lc_candidates"] == 45
    assert dev["lc_accepted"] == host["lc_accepted"] > 0
    few = loop.run(lc_gate="appearance", lc_top_k=1, **KW)
    assert few["lc_top_k"] == 1 and few["lc_candidates"] == 11 and few["lc_pairs"] == [p for p in dev["lc_pairs"] if p in few["lc_pairs"]]
    with pytest.raises(ValueError):
        loop.run(lc_gate="appearance", lc_top_k=0, **KW)


DRIFTS = (5.0, 10.0, 20.0, 30.0, 45.0)


def test_under_heading_drift_the_appearance_gate_closes_what_the_pose_based_theta0_loses(gpu):
    """What the drift can and cannot do on this bag, found on the CPU from the odometry poses alone:

    synth.odometry_from_truth adds the heading random walk to the HEADINGS only -- positions drift by sigma_t, whatever
    drift_th_deg is -- and all 32 scans of the bag lie within 2 m.  So the geometric gate keeps the same 66 pairs at every
    drift_th_deg: no value empties it, and the condition "the geometric gate keeps no pair" cannot be met on this bag (asserted
    below).  What heading drift does take away is the matcher's question: theta0 is the estimate's heading difference, and the
    window is +-30 degrees around it.  drift_th_deg = 20 is the smallest of 5, 10, 20, 30, 45 at which more than half of the gated
    pairs' odometry heading differences are off by more than those 30 degrees (0.59 of them; 0.17 at 10).  Under it the appearance
    run, whose theta0 comes from the scans, accepts closures and ends with the lower rms trajectory error.  Measured (DESIGN.md
    section 8 item 17): geometric 35 of 66 accepted, 0.341 m; appearance 45 of 45, 0.299 m."""
    import examples.slam_loop as loop
    bag = synth.SynthBag(KW["n_scans"], dense=True, seed=SEED, spacing=KW["spacing"])
    idx = np.arange(KW["n_scans"])

    def gated(drift):
        odom = synth.odometry_from_truth(bag.truth, sigma_t=0.02, sigma_th_deg=drift, seed=SEED)
        odom = odom - odom[0] + bag.truth[0]
        d = np.linalg.norm(odom[:, None, :2] - odom[None, :, :2], axis=2)
        s, t = np.nonzero((d < 3.5) & (idx[:, None] - idx[None, :] > 20))
        off_by = np.degrees(np.abs(angle_mod((odom[s, 2] - odom[t, 2]) - (bag.truth[s, 2] - bag.truth[t, 2]))))
        return list(zip(s.tolist(), t.tolist())), float((off_by > 30.0).mean())
    pairs, _ = gated(0.3)
    shares = {}
    for drift in DRIFTS:
        same, shares[drift] = gated(drift)
        assert same == pairs and len(pairs) == 66
    drift = min(d for d in DRIFTS if shares[d] > 0.5)
    assert drift == 20.0
    geo = loop.run(lc_gate="geometric", drift_th_deg=drift, **KW)
    app = loop.run(lc_gate="appearance", drift_th_deg=drift, **KW)
    print("drift %.0f: geometric %d of %d accepted, err %.4f m; appearance %d of %d, err %.4f m (icp %.4f m)" % (
        drift, geo["lc_accepted"], geo["lc_candidates"], geo["err_lc_m"], app["lc_accepted"], app["lc_candidates"], app["err_lc_m"],
        app["err_icp_m"]))
    assert geo["lc_candidates"] == 66 and app["lc_accepted"] > 0
    assert app["err_lc_m"] < geo["err_lc_m"]
