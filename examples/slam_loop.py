#!/usr/bin/env python3
"""End-to-end loop on one MI355X, or one rank per GPU under `python -m torch.distributed.run
--nproc-per-node N examples/slam_loop.py` (the shape of BASELINE configs[0] / configs[4]):

  synthetic 1081-beam bag
  -> growing-window ICP solve, windows 1..10     Solver::OptimizeOverGrowingWindow   solver.cc:335-356
  -> loop-closure candidates                     LCCandidateFilter (scatter score, GPU) + geometric pair gate
                                                 (lc_candidate_filter.cc:35-81, in place of lc_matcher.cc:28-74),
                                                 or --lc-gate chi-square: LCMatcher's own covariance gate
  -> batched correlative scan matching           GetRelativeTransform                solver.cc:630-649
  -> loop-closure constraints + re-solve         AddLCConstraints (TODO body)         solver.cc:651-673
  -> a HITL message (two segments on one wall)   HitlCallback: GetRelevantPosesForHITL, AddHITLResiduals, SolveSLAM
                                                                                     solver.cc:479-559
and reports trajectory error and wall-clock per stage.  Every evaluation goes through the backend handed to run():
the product's HipBackend by default; tests and bench.py's cpu_baseline inject the oracle's CPU backend to time the
same loop on the CPU restatement."""
import argparse
import inspect
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synthetic_hitl_message(bag, poses, early, late):
    """What a user would draw: ONE piece of the outer wall, once where the scan of node `early` puts it under the
    current estimate and once where the scan of node `late` puts it (the two differ by the accumulated drift).
    Both segments cover the same physical piece: PointToLineResidual measures the distance to the SEGMENT
    (slam_util.h:92-110), so points beyond an end of line a would be pulled along the wall.
    HitlSlamInputMsg fields (msg/HitlSlamInputMsg.msg:1-4)."""
    seg = bag.segs[0]  # bottom wall of the outer rectangle, world frame (x0 y0 x1 y1), along x
    lo = max(min(seg[0], seg[2]), bag.truth[early, 0] - 8.0, bag.truth[late, 0] - 8.0)
    hi = min(max(seg[0], seg[2]), bag.truth[early, 0] + 8.0, bag.truth[late, 0] + 8.0)

    def seen_from(i):
        # true wall piece -> node i's frame (truth) -> world under the estimate of node i
        out = []
        for x, y in ((lo, seg[1]), (hi, seg[3])):
            c, s = math.cos(-bag.truth[i, 2]), math.sin(-bag.truth[i, 2])
            lx, ly = c * (x - bag.truth[i, 0]) - s * (y - bag.truth[i, 1]), s * (x - bag.truth[i, 0]) + c * (y - bag.truth[i, 1])
            c, s = math.cos(poses[i, 2]), math.sin(poses[i, 2])
            out.append((c * lx - s * ly + poses[i, 0], s * lx + c * ly + poses[i, 1], 0.0))
        return out
    a, b = seen_from(early), seen_from(late)
    return {"line_a_start": a[0], "line_a_end": a[1], "line_b_start": b[0], "line_b_end": b[1]}


LC_MIN_SEPARATION = 20  # nodes between the two scans of a loop-closure pair (the pair gate below)


def run(n_scans=320, window=10, seed=20201114, drift_t=0.02, drift_th_deg=0.3, verbose=False, residual="normal",
        rank=0, world=1, device="cuda:0", backend=None, iterations=4, hitl=True, cell_bits=16, gate="scatter",
        min_scatter_score=0.70, csm_score_threshold=-5.0, spacing=0.25, hitl_device=False, normals="bag", lc_submap=0,
        linear_solver="host", lc_gate="geometric", lc_max_score=5000.0, map_output=None, grid_output=None, lc_verify=None,
        lc_max_violation=None, lc_top_k=5, lc_consistency=False, lc_min_set=3, _lc_corrupt=None, lc_sequence=0, lc_sequence_step=1,
        lc_loss=None, lc_loss_scale=1.0, movers=0, drop_transients=False, lc_refine=None, lc_factor=None,
        lc_info_sigma_m=1.0):
    """min_scatter_score: LCCandidateFilter's threshold is 0.70 (lc_candidate_filter.cc:76); scans of the synthetic
    24 m x 16 m room score ~0.4, so callers on that world pass a lower one.
    hitl_device: the HITL constraint's points are selected and packed on the GPU (hitl.select, under the "path" clock) and
    its blocks reduced there to normal equations, instead of hostside.hitl_relevant_poses + per-point evaluation.
    normals: "bag" takes the synthetic world's analytic normals; "device" estimates them from the clouds on the GPU
    (backend.normals: NormalComputation::GetNormals, once, before the first solve, under the "path" clock) -- what a real
    bag, which brings none, needs.
    lc_submap K > 0: every loop-closure target's table is built from its SUBMAP, the scans t - K .. t + K placed in t's frame
    by the current estimate (the poses after the window solve), instead of from scan t alone ("Submaps").
    A backend whose match() takes submap_radius merges the clouds on the device; any other gets the merged clouds as extra
    scans (hostside.submap_extra_scans).  K must stay below the pair gate's minimum separation (20): a source is never in
    its target's submap.  Not with world > 1.
    linear_solver: "host" -- every solve's linear step in scipy on downloaded rows -- or "device": assembled and solved on the
    GPU by block-Jacobi PCG (PoseGraph.solve; needs hitl_device for the HITL phase).
    lc_gate: "geometric" -- the distance-and-separation pair gate -- or "chi-square": LCMatcher's own walk (GetPossibleMatches,
    lc_matcher.cc:59-74), every candidate scan as source against the others by hostside.lc_possible_matches, the covariance
    blocks of all those pairs from ONE PoseGraph.cross_covariances(linear_solver=linear_solver) call and the scores from the
    backend's chi_square_gate; what it keeps is intersected with the geometric gate's separation rule (the later scan is the
    source, more than 20 nodes apart).  Needs gate "scatter".  lc_max_score: the test's threshold (LCMatcher's 5000: on the
    synthetic room, whose dense scans pin every pose to a fraction of a millimetre, that keeps nothing).
    lc_gate "appearance": no pose enters -- every scan of the candidate list (gate "scatter": LCCandidateFilter's; otherwise every
    scan) is compared with the earlier ones by ring descriptor ("Place descriptors"), its lc_top_k nearest more
    than 20 nodes apart become the pairs (src = the query), and the matcher's theta0 is the heading the aligning rotation gives,
    not the estimate's heading difference.  A backend with place_candidates() does it on the device; any other is served by
    hostside.place_candidates.  Everything after that is the same; the result reports lc_gate, lc_top_k, place_s and lc_pairs.
    lc_sequence W > 0 (only with lc_gate "appearance"): the descriptors are compared over a window of 2W + 1 frames, lc_sequence_step
    scans apart, around both scans of a pair and in both directions of travel ("Place sequences"): a backend
    with place_sequence_candidates() does it on the device, any other is served by hostside.place_sequence_candidates.  2 W step
    must stay within the minimum separation (20).  The result also reports lc_sequence, lc_sequence_step, lc_sequence_reverse
    (records of direction 1) and lc_sequence_short (records whose window was cut short).  0: a single scan's descriptor, as before.
    map_output: a path -- the final poses' vector map (Solver::Vectorize, solver.cc:581-624: backend.vectorize, on the GPU)
    is written there as 'x1,y1,x2,y2' lines (hostside.write_map_lines); the result reports map_segments and vectorize_s, and
    keeps the poses the map was made at in "map_poses".
    grid_output: a path stem -- the final poses' occupancy grid (backend.occupancy_grid: every scan ray-traced on the GPU) is
    written as STEM.pgm and STEM.yaml, map_server's pair (hostside.write_occupancy_map); the result reports occupancy_s and
    grid_occupied / grid_free / grid_unknown, and keeps the poses in "grid_poses".
    lc_verify: "free-space" -- every match record is checked against the target's free space ("Free-space
    check"): a record is kept only if the source returns that land in space the target's beams crossed, plus the source beams
    that run through a target hit, are at most lc_max_violation permille (None: freespace.DEFAULT_MAX_PERMILLE) of the returns
    inside the grid.  A backend whose match() takes `freespace` checks on the device inside the call; any other is checked by
    hostside.freespace_counts.  The result reports lc_verified, lc_verify_rejected (they sum to the unverified run's
    lc_accepted) and the rms relative error of either set.  Not with world > 1 or lc_submap.
    lc_refine: "icp" -- every record that passed the score gate is refined from its lattice pose (one cell, one degree) to a
    sub-cell pose by point-to-line ICP against the target scan ("Match refinement"), before lc_verify and
    lc_consistency; a backend with refine_matches() runs it on the device, any other is served by hostside.refine_matches.  A
    pair with any flag other than NOT_CONVERGED keeps its lattice pose.  The result reports lc_refined, lc_refine_flags (a count
    per flag), refine_s, and lc_rel_err_m of the poses actually used.  Not with world > 1.
    lc_consistency: the accepted records -- after the score gate and, with lc_verify, the free-space check -- are judged against
    each other ("Loop-closure consistency"): the cycle two records form with the estimate between their ends
    must close up to the drift the estimate can have gathered, and only the records of a greedily grown set of mutually consistent
    ones become constraints -- none if the set has fewer than lc_min_set members.  A backend with consistent_set() does it on the
    device; any other is served by hostside.consistent_set.  The result reports lc_consistency, lc_consistent, lc_inconsistent
    (they sum to the unfiltered run's lc_accepted), lc_inconsistent_rel_err_m and consistency_s.  Not with world > 1.
    lc_loss: None (or "none"), "huber", "soft-l1" or "cauchy" -- the robust loss of the loop-closure factors (DESIGN.md section 3,
    "Robust loss"; PoseGraph.add_loop_closures(loss=...)) in the closure solve and in the HITL phase's growing-window solve, with
    scale lc_loss_scale in units of the weighted residual: at the closures' weight 10, 1.0 is 0.1 m or 0.1 rad, two cells of the
    matcher's lattice.  The filters in front of the solve are all-or-nothing; the loss weighs what they let through by its own
    residual.  The result then also reports lc_loss, lc_loss_scale and, after the closure solve, lc_weights ([src, tgt, rho'] per
    accepted record), lc_weight_min, lc_downweighted (records with rho' < 0.5), lc_downweighted_pairs and
    lc_downweighted_rel_err_m.  Works with world > 1 (the solve is replicated).
    movers N > 0: N synthetic walkers are added to the bag (synth.add_movers: discs of radius 0.3 m that walk the robot's own loop
    at twice its speed, each starting further ahead); the result reports movers and mover_returns.
    drop_transients: after the growing-window solve, at the solved poses, the scans are traced into the occupancy planes and every
    return is classified by them ("Transient returns"; backend.drop_transients, in-stream on the GPU); the
    clouds without their transient returns are what the loop-closure tables, map_output and grid_output are made from.  The
    result reports transient_stats (transient.STATS_FIELDS), transient_s and, with movers, the shares of the walkers' and of the
    other returns that were flagged.  Not with world > 1.  Both are off by default and change nothing then.
    lc_factor: None (or "world") -- every accepted record becomes the odometry-style factor, frozen in the world frame at the target's
    current heading, at the scalar weights (10, 10) -- or "relative": a relative-pose factor ("Relative-pose
    factors"; PoseGraph.add_loop_closures(information=...)), which measures the source in the target's frame at every evaluation
    and carries its own information: with lc_refine "icp" the Gauss-Newton H of the record's refinement over lc_info_sigma_m^2
    (metres; 1.0 puts a closure on the footing of the ICP blocks), for a record that kept its lattice pose and without lc_refine
    diag(10^2, 10^2, 10^2).  The result then also reports lc_factor, lc_info_from_icp (accepted records that took their H),
    lc_info_sigma_m and lc_info_eig_min / lc_info_eig_max over those records' informations (None without any).  An lc_loss' scale
    is then in standard deviations.  Works with world > 1 (the solve is replicated), both linear solvers and any backend.
    _lc_corrupt: TEST ONLY -- a callable (src, tgt, rel, good) -> rel that replaces the records' transforms before the consistency
    filter and the constraints (tests/test_consistency_loop_gpu.py displaces accepted records with it).
    With world > 1 (one process per GPU under torch.distributed): the window ICP solve is replicated -- its
    consumer, the solver, is host-side -- and the loop-closure pairs are sharded by target across the ranks,
    matched, and all-gathered (nautilus_amd/sharding.py); every rank ends with the same trajectory."""
    from nautilus_amd import _lib, csm, hostside, posegraph, sharding, synth
    if backend is None:
        backend = posegraph.HipBackend(device)
    bag = synth.SynthBag(n_scans, dense=True, seed=seed, spacing=spacing)
    odom = synth.odometry_from_truth(bag.truth, sigma_t=drift_t, sigma_th_deg=drift_th_deg, seed=seed)
    odom = odom - odom[0] + bag.truth[0]  # both tracks start at the same anchor (pose 0 is held constant)
    scans, mover_mask = bag.scans, None
    if int(movers) < 0:
        raise ValueError("run: movers %r must be >= 0" % (movers,))
    if movers:
        ahead = lambda k: (lambda i: tuple(bag.truth[(2 * i + 15 + 40 * k) % n_scans, :2]))
        scans, masks = synth.add_movers(bag.scans, bag.truth, [(ahead(k), 0.3) for k in range(int(movers))])
        mover_mask = np.concatenate(masks)
    if drop_transients and world > 1:
        raise ValueError("run: drop_transients with world > 1 (the filter has no sharded path)")
    xy, off = csm.pack_scans(scans)
    nrm = np.concatenate(bag.normals).astype(np.float32)
    kind = _lib.NHIP_LIDAR_NORMAL if residual == "normal" else _lib.NHIP_LIDAR_POINT
    if residual not in ("normal", "point", "feature"):
        raise ValueError("run: residual %r" % (residual,))
    if normals not in ("bag", "device"):
        raise ValueError("run: normals %r" % (normals,))
    lc_submap = int(lc_submap)
    if lc_gate not in ("geometric", "chi-square", "appearance") or (lc_gate == "chi-square" and gate != "scatter"):
        raise ValueError("run: lc_gate %r (\"geometric\", \"appearance\", or \"chi-square\" with gate \"scatter\")" % (lc_gate,))
    if not 1 <= int(lc_top_k) <= 32:
        raise ValueError("run: lc_top_k %r: 1..32" % (lc_top_k,))
    lc_sequence, lc_sequence_step = int(lc_sequence), int(lc_sequence_step)
    if lc_sequence and lc_gate != "appearance":
        raise ValueError("run: lc_sequence %d needs lc_gate \"appearance\", not %r" % (lc_sequence, lc_gate))
    if not (0 <= lc_sequence <= 8 and 1 <= lc_sequence_step <= 16 and 2 * lc_sequence * lc_sequence_step <= LC_MIN_SEPARATION):
        raise ValueError("run: lc_sequence %d in 0..8, lc_sequence_step %d in 1..16, twice their product at most the minimum "
                         "separation (%d)" % (lc_sequence, lc_sequence_step, LC_MIN_SEPARATION))
    if not 0 <= lc_submap < LC_MIN_SEPARATION:
        raise ValueError("run: lc_submap %d: a submap radius is >= 0 and below the pair gate's minimum separation (%d)"
                         % (lc_submap, LC_MIN_SEPARATION))
    if lc_submap and world > 1:
        raise ValueError("run: lc_submap with world > 1 (sharded matching has no submaps)")
    if lc_verify not in (None, "free-space"):
        raise ValueError("run: lc_verify %r (None or \"free-space\")" % (lc_verify,))
    if lc_verify and (world > 1 or lc_submap):
        raise ValueError("run: lc_verify with world > 1 or lc_submap (the free-space check has no sharded path and no submap targets)")
    if lc_refine not in (None, "icp"):
        raise ValueError("run: lc_refine %r (None or \"icp\")" % (lc_refine,))
    if lc_refine and world > 1:
        raise ValueError("run: lc_refine with world > 1 (the refinement has no sharded path)")
    if lc_consistency and world > 1:
        raise ValueError("run: lc_consistency with world > 1 (the consistent set has no sharded path)")
    if lc_consistency and int(lc_min_set) < 0:
        raise ValueError("run: lc_min_set %r must be >= 0" % (lc_min_set,))
    if lc_max_violation is not None and not 0 <= int(lc_max_violation) <= 1000:
        raise ValueError("run: lc_max_violation %r: permille, 0..1000" % (lc_max_violation,))
    if lc_factor not in (None, "world", "relative"):
        raise ValueError("run: lc_factor %r (None, \"world\" or \"relative\")" % (lc_factor,))
    if lc_factor == "relative" and not (math.isfinite(float(lc_info_sigma_m)) and float(lc_info_sigma_m) > 0.0):
        raise ValueError("run: lc_info_sigma_m %r must be finite and > 0" % (lc_info_sigma_m,))
    loss = None
    if lc_loss not in (None, "none"):
        from nautilus_amd.loss import Loss
        if lc_loss not in ("huber", "soft-l1", "cauchy"):
            raise ValueError("run: lc_loss %r (None, \"none\", \"huber\", \"soft-l1\" or \"cauchy\")" % (lc_loss,))
        loss = Loss(lc_loss.replace("-", "_"), lc_loss_scale)  # (ValueError: a scale that is not finite or is <= 0)
    out = {"backend": backend.name, "n_scans": n_scans, "window": window, "residual": residual,
           "err_odometry_m": posegraph.trajectory_error(odom, bag.truth)}
    posegraph.clock_reset()
    pcg_by_phase, pcg_seen = {}, [0, 0]

    def pcg_phase(name):
        """[solves, PCG iterations] of the phase that just ended (the device linear solver's; zeros with the host's)"""
        now = [posegraph.LINEAR_STATS["solves"], posegraph.LINEAR_STATS["iterations"]]
        pcg_by_phase[name] = [now[0] - pcg_seen[0], now[1] - pcg_seen[1]]
        pcg_seen[:] = now

    if normals == "device":
        t0 = time.perf_counter()
        with posegraph.clocked("path"):
            nrm = backend.normals(xy, off)
        out["t_normals_s"] = time.perf_counter() - t0
        out["normals"] = "device"

    feats = None
    if residual == "feature":
        # the reference's FEATURE mode (the only one SolveSLAM runs, solver.cc:363): <= 20 planar and <= 10 edge points per
        # scan, extracted once per run on the GPU (FeatureExtractor, slam_types.h:66-69)
        t0 = time.perf_counter()
        with posegraph.clocked("path"):
            feats = backend.features(xy, nrm, off)
        out["t_features_s"] = time.perf_counter() - t0
        out["planar_points"], out["edge_points"] = int(feats[0][2][-1]), int(feats[1][2][-1])

    t0 = time.perf_counter()
    pg, poses = posegraph.solve_growing_window(xy, nrm, off, odom, 1, window, iterations=iterations, kind=kind,
                                               device=device, verbose=verbose, backend=backend, features=feats,
                                               linear_solver=linear_solver)
    out["t_icp_solve_s"] = time.perf_counter() - t0
    pcg_phase("icp")
    out["err_icp_m"] = posegraph.trajectory_error(poses, bag.truth)
    out["icp_correspondences"] = pg.icp.n_corr
    if movers:
        out["movers"], out["mover_returns"] = int(movers), int(mover_mask.sum())

    # ---- the clouds the loop-closure tables and the maps are made from: the scans, or the scans without their transient returns
    xy_lc, off_lc = xy, off
    if drop_transients:
        if not hasattr(backend, "drop_transients"):
            raise RuntimeError("run: drop_transients needs a backend with drop_transients(); backend %r has none" % (backend.name,))
        from nautilus_amd import transient
        t0 = time.perf_counter()
        static = backend.drop_transients(poses, xy=xy, offsets=off)  # (outside the stage clocks: not a solve stage)
        out["transient_s"] = time.perf_counter() - t0
        xy_lc, off_lc = static.xy, static.offsets
        out["transient_stats"] = {k: int(v) for k, v in zip(transient.STATS_FIELDS, static.stats)}
        if movers:
            flagged = static.labels == 1
            out["transient_mover_share"] = float(flagged[mover_mask].mean()) if mover_mask.any() else None
            out["transient_other_share"] = float(flagged[~mover_mask].mean())

    def appearance_pairs(ids):
        """lc_gate "appearance": the K nearest earlier scans of every scan of `ids` by ring descriptor (place.py), more than 20
        nodes apart, and the heading each aligning rotation gives.  No pose enters."""
        from nautilus_amd import place
        t1 = time.perf_counter()
        ids = np.asarray(ids, dtype=np.int32)
        pspec = place.spec(top_k=int(lc_top_k), min_separation=LC_MIN_SEPARATION, flags=place.NHIP_PLACE_PAST_ONLY)
        if lc_sequence:  # (the window of frames around both scans, DESIGN.md section 3, "Place sequences")
            qspec = place.seq_spec(half_window=lc_sequence, step=lc_sequence_step)
            if hasattr(backend, "place_sequence_candidates"):
                with posegraph.clocked("path"):
                    rec, _ = backend.place_sequence_candidates(xy, off, ids, pspec, qspec)
            else:
                with posegraph.clocked("marshal"):
                    rec, _ = hostside.place_sequence_candidates(xy, off, ids, pspec, qspec)
            filled = rec[:, :, 0] >= 0
            out["lc_sequence"], out["lc_sequence_step"] = lc_sequence, lc_sequence_step
            out["lc_sequence_reverse"] = int((filled & (rec[:, :, 7] == 1)).sum())
            out["lc_sequence_short"] = int((filled & (rec[:, :, 6] < 2 * lc_sequence + 1)).sum())
        elif hasattr(backend, "place_candidates"):
            with posegraph.clocked("path"):
                rec, _ = backend.place_candidates(xy, off, ids, pspec)
        else:  # (a backend without the method: the plain numpy host path, as freespace_counts is for the free-space check)
            with posegraph.clocked("marshal"):
                rec, _ = hostside.place_candidates(xy, off, ids, pspec)
        out["lc_gate"], out["lc_top_k"], out["place_s"] = lc_gate, int(lc_top_k), time.perf_counter() - t1
        s_, t_, th = place.pairs(ids, rec)
        out["lc_pairs"] = np.stack([s_, t_], axis=1).tolist()
        return s_, t_, th

    # ---- loop-closure candidates
    t0 = time.perf_counter()
    place_theta0 = None
    if gate == "scatter":
        # LCCandidateFilter::GetLCCandidates: scatter-matrix score of every scan (one GPU pass), nodes >= 5 m apart ...
        with posegraph.clocked("path"):
            scores = hostside.scatter_scores(backend, xy, off)
        cand = hostside.lc_candidates_from_scores(poses, scores, min_score=min_scatter_score)
        # ... then the pair gate: |dt| < lc_base_max_range (3.5 m, default_config.lua:122) on the current estimate and
        # more than 20 nodes apart (geometric stand-in for LCMatcher's per-pair ceres::Covariance, lc_matcher.cc:28-74)
        if lc_gate == "geometric":
            with posegraph.clocked("path"):
                src, tgt = hostside.geometric_pair_gate(poses, cand, max_range=3.5, min_separation=LC_MIN_SEPARATION, backend=backend)
        elif lc_gate == "appearance":  # the LCCandidateFilter list is the list of scans that are compared
            src, tgt, place_theta0 = appearance_pairs(cand)
        else:
            t1 = time.perf_counter()
            pairs = [(int(s_), int(c)) for s_ in cand for c in cand if c != s_]
            cov = dict(zip(pairs, pg.cross_covariances(pairs, linear_solver=linear_solver))) if pairs else {}
            cov_fn = lambda ps: np.stack([cov[(int(s_), int(c))] for s_, c in ps])
            kept = []
            for s_ in cand:
                with posegraph.clocked("path"):
                    matches = hostside.lc_possible_matches(s_, cand, poses, cov_fn, max_score=lc_max_score, backend=backend)
                kept += [(s_, c) for c in matches if s_ - c > LC_MIN_SEPARATION]
            src = np.array([p[0] for p in kept], dtype=np.int32)
            tgt = np.array([p[1] for p in kept], dtype=np.int32)
            out["lc_gate"], out["lc_gate_s"], out["lc_gate_pairs"] = lc_gate, time.perf_counter() - t1, len(kept)
            out["lc_gate_pairs_walked"], out["lc_gate_max_score"] = len(pairs), float(lc_max_score)
            if linear_solver == "device":
                its, batches = pg.covariance_stats["iterations"], pg.covariance_stats["batches"]
                out["lc_gate_pcg"] = {"systems": pg.covariance_stats["systems"], "batches": len(batches),
                                      "iterations_min_median_max": [int(np.min(its)), float(np.median(its)), int(np.max(its))] if its else None,
                                      "not_converged": int(sum(f != 0 for f in pg.covariance_stats["flags"])),
                                      "solve_s": float(sum(b[2] for b in batches)),
                                      "us_per_iteration_per_batch": [1e6 * b[2] / max(b[1], 1) for b in batches]}
            pcg_phase("lc_gate")
        out["lc_candidate_scans"] = len(cand)
    elif lc_gate == "appearance":
        src, tgt, place_theta0 = appearance_pairs(np.arange(n_scans))
    else:
        idx = np.arange(n_scans)
        d = np.linalg.norm(poses[:, None, :2] - poses[None, :, :2], axis=2)
        s_, t_ = np.nonzero((d < 3.5) & (np.abs(idx[:, None] - idx[None, :]) > LC_MIN_SEPARATION))
        keep = s_ > t_
        src, tgt = s_[keep].astype(np.int32), t_[keep].astype(np.int32)
    out["t_gate_s"] = time.perf_counter() - t0
    out["lc_candidates"] = int(len(src))
    lc = None
    if len(src):
        t0 = time.perf_counter()
        a = poses[src, 2] - poses[tgt, 2]
        theta0 = a - 2 * math.pi * np.rint(a / (2 * math.pi))
        if place_theta0 is not None:  # (the heading difference the descriptors' aligning rotation gives, not the estimate's)
            theta0 = place_theta0
        if world > 1:
            spec_search = {}

            def match_shard(src_s, slot_s, th_s, ids_s):
                if len(src_s) == 0:
                    return np.zeros(0, dtype=csm.MATCH_DTYPE)
                m_, spec_search["spec"], spec_search["search"] = backend.match(xy_lc, off_lc, src_s, ids_s[slot_s], th_s, cell_bits)
                return m_
            with posegraph.clocked("path"):
                m = sharding.distributed_match(match_shard, src, tgt, theta0, rank, world, device=device)
            spec, search = csm.grid_spec(30.0, 0.05, 2.0, 1e-10, 40, cell_bits), csm.search_spec()
        elif lc_submap and "submap_radius" in inspect.signature(backend.match).parameters:
            with posegraph.clocked("path"):
                m, spec, search = backend.match(xy_lc, off_lc, src, tgt, theta0, cell_bits, submap_radius=lc_submap, poses=poses)
        elif lc_submap:
            with posegraph.clocked("marshal"):
                xy_m, off_m, tgt_m = hostside.submap_extra_scans(xy_lc, off_lc, poses, tgt, lc_submap)
            with posegraph.clocked("path"):
                m, spec, search = backend.match(xy_m, off_m, src, tgt_m, theta0, cell_bits)
        elif lc_verify and "freespace" in inspect.signature(backend.match).parameters:
            from nautilus_amd import freespace
            with posegraph.clocked("path"):
                m, spec, search, fs_counts = backend.match(xy_lc, off_lc, src, tgt, theta0, cell_bits, freespace=freespace.default_spec())
        else:
            with posegraph.clocked("path"):
                m, spec, search = backend.match(xy_lc, off_lc, src, tgt, theta0, cell_bits)
            if lc_verify:  # (a backend without the parameter: the plain numpy host path, as submap_extra_scans is for submaps)
                with posegraph.clocked("marshal"):
                    fs_counts = hostside.freespace_counts(xy_lc, off_lc, src, tgt, theta0, m, spec, search)
        out["t_csm_s"] = time.perf_counter() - t0
        with posegraph.clocked("marshal"):  # (records -> (tx, ty, theta) as consumed at solver.cc:640-644, vectorised)
            rel = np.stack([(m["ix"].astype(np.float64) - (search.nx - 1) // 2) * spec.res,
                            (m["iy"].astype(np.float64) - (search.ny - 1) // 2) * spec.res,
                            theta0 + (m["itheta"].astype(np.float64) - (search.n_theta - 1) // 2) * search.theta_step], axis=1)
            rel = rel.astype(np.float32).astype(np.float64)  # (the reference's floats)
        inside = (np.abs(m["ix"] - 40) < 40) & (np.abs(m["iy"] - 40) < 40) & (np.abs(m["itheta"] - 30) < 30)
        # "Anything above this threshold for CSM is deemed a successful local loop closure"
        # (csm_score_threshold = -5.0, config/default_config.lua:84-85); optima on the lattice border are open-ended
        good = inside & (m["score"] > csm_score_threshold)
        truth_rel = np.array([bag.true_relative(s, t) for s, t in zip(src, tgt)])
        refined_of = None  # with lc_refine: (the records' indices, their refined records)
        if lc_refine:
            # the records that passed the score gate go from their lattice pose to the sub-cell pose of point-to-line ICP against
            # the target SCAN (also where the table was a submap, which has no normals; the scans as ingested, with their normals)
            t1 = time.perf_counter()
            idx = np.nonzero(good)[0]
            args = (xy, nrm, off, src[idx], tgt[idx], theta0[idx], m[idx], spec, search)
            if hasattr(backend, "refine_matches"):
                with posegraph.clocked("path"):
                    refined = backend.refine_matches(*args)
            else:  # (a backend without the method: the numpy host path)
                with posegraph.clocked("marshal"):
                    refined = hostside.refine_matches(*args)
            used = hostside.refine_keeps_pose(refined)  # (any flag but NOT_CONVERGED: the lattice pose stays)
            rel[idx[used]] = hostside.refined_to_transform(refined[used])
            out["lc_refined"], out["refine_s"] = int(used.sum()), time.perf_counter() - t1
            out["lc_refine_flags"] = hostside.refine_flag_counts(refined)
            refined_of = (idx, refined)
        rms = lambda sel: float(np.sqrt(np.mean(np.sum((rel[sel, :2] - truth_rel[sel, :2]) ** 2, axis=1)))) if sel.any() else None
        if lc_verify:
            from nautilus_amd import freespace
            permille = freespace.DEFAULT_MAX_PERMILLE if lc_max_violation is None else int(lc_max_violation)
            verified = freespace.keep(fs_counts, permille)
            out["lc_verify"], out["lc_max_violation"] = lc_verify, permille
            out["lc_verified"], out["lc_verify_rejected"] = int((good & verified).sum()), int((good & ~verified).sum())
            out["lc_verify_rejected_rel_err_m"] = rms(good & ~verified)
            good &= verified
        if _lc_corrupt is not None:
            rel = np.ascontiguousarray(_lc_corrupt(src, tgt, rel.copy(), good.copy()), dtype=np.float64)
        if lc_consistency:
            from nautilus_amd import consistency
            t1 = time.perf_counter()
            idx = np.nonzero(good)[0]
            if hasattr(backend, "consistent_set"):
                with posegraph.clocked("path"):
                    members, n_members, _ = backend.consistent_set(poses, src[idx], tgt[idx], rel[idx])
            else:  # (a backend without the method: the plain numpy host path, as place_candidates is for the appearance gate)
                with posegraph.clocked("marshal"):
                    members, n_members, _ = hostside.consistent_set(consistency.prepare(poses, src[idx], tgt[idx], rel[idx]))
            consistent = np.zeros(len(good), dtype=bool)
            consistent[idx[consistency.keep(members, n_members, len(idx), int(lc_min_set))]] = True
            out["lc_consistency"], out["lc_min_set"], out["consistency_s"] = True, int(lc_min_set), time.perf_counter() - t1
            out["lc_consistent"], out["lc_inconsistent"] = int((good & consistent).sum()), int((good & ~consistent).sum())
            out["lc_inconsistent_rel_err_m"] = rms(good & ~consistent)
            out["lc_consistent_pairs"] = np.stack([src[good & consistent], tgt[good & consistent]], axis=1).tolist()
            out["lc_inconsistent_pairs"] = np.stack([src[good & ~consistent], tgt[good & ~consistent]], axis=1).tolist()
            good &= consistent
        out["lc_accepted"] = int(good.sum())
        out["lc_rel_err_m"] = rms(good)
        lc = (src[good], tgt[good], rel[good])
        if lc_factor == "relative":
            # every record's information and heading (cos, sin): the refinement's H and (c, s) where a record carries a refined
            # pose, the closures' weights and libm's cos / sin of the lattice heading where not
            with posegraph.clocked("marshal"):
                info, took = hostside.relpose_information(None, n=len(src), weights=(10.0, 10.0))
                cs = np.array([(math.cos(t), math.sin(t)) for t in rel[:, 2]], dtype=np.float64).reshape(-1, 2)
                if refined_of is not None:
                    info[refined_of[0]], took[refined_of[0]] = hostside.relpose_information(
                        refined_of[1], sigma_m=float(lc_info_sigma_m), weights=(10.0, 10.0))
                    mine = refined_of[0][took[refined_of[0]]]
                    cs[mine] = np.stack([refined_of[1]["c"], refined_of[1]["s"]], axis=1)[took[refined_of[0]]]
                lc += ({"information": info[good], "rel_cs": cs[good]},)
            eig = np.array([np.linalg.eigvalsh(np.array([[L[0], L[1], L[2]], [L[1], L[3], L[4]], [L[2], L[4], L[5]]]))
                            for L in info[good & took]]).reshape(-1, 3)
            out["lc_factor"], out["lc_info_from_icp"], out["lc_info_sigma_m"] = "relative", int((good & took).sum()), float(lc_info_sigma_m)
            out["lc_info_eig_min"] = float(eig.min()) if eig.size else None
            out["lc_info_eig_max"] = float(eig.max()) if eig.size else None
        elif lc_factor == "world":
            out["lc_factor"] = "world"
        t0 = time.perf_counter()
        with posegraph.clocked("marshal"):
            pg.add_loop_closures(*lc[:3], loss=loss, **(lc[3] if len(lc) > 3 else {}))
        poses, _ = pg.solve(iterations=2 * iterations, verbose=verbose, linear_solver=linear_solver)
        out["t_lc_solve_s"] = time.perf_counter() - t0
        pcg_phase("lc")
        out["err_lc_m"] = posegraph.trajectory_error(poses, bag.truth)
        if loss is not None:
            # what the loss made of every record at the solved poses (outside the stage clocks' t_*: a report, not a solve stage)
            rho1 = pg.closure_weights()[:, 2]
            down = np.zeros(len(good), dtype=bool)
            down[np.nonzero(good)[0][rho1 < 0.5]] = True
            out["lc_loss"], out["lc_loss_scale"] = lc_loss, float(lc_loss_scale)
            out["lc_weights"] = [[int(s), int(t), float(w)] for s, t, w in zip(lc[0], lc[1], rho1)]
            out["lc_weight_min"] = float(rho1.min()) if len(rho1) else None
            out["lc_downweighted"] = int(down.sum())
            out["lc_downweighted_pairs"] = np.stack([src[down], tgt[down]], axis=1).tolist()
            out["lc_downweighted_rel_err_m"] = rms(down)

    # ---- HITL: the user marks the same wall twice; HitlCallback re-solves with the point-to-line blocks
    if hitl:
        t0 = time.perf_counter()
        early, late = n_scans // 20, n_scans - 1 - n_scans // 20
        msg = synthetic_hitl_message(bag, poses, early, late)
        lines = hostside.hitl_segments(msg)
        if hitl_device:
            with posegraph.clocked("path"):
                con = backend.hitl_select(xy, off, poses, lines[0], lines[1])
        else:
            with posegraph.clocked("hitl_select"):
                a_poses, b_poses = hostside.hitl_relevant_poses(poses, scans, lines[0], lines[1])
            with posegraph.clocked("marshal"):
                con = posegraph.HitlConstraint(lines[0], lines[1], a_poses, b_poses)
        out["hitl_line_a_poses"], out["hitl_line_b_poses"] = con.n_a, con.n_b
        out["hitl_points"] = con.n_points if hitl_device else int(sum(len(p) for _, p in con.blocks))
        # state_->problem.odometry_factors = GetSolvedOdomFactors() (solver.cc:535, 406-427): the solved trajectory
        # becomes the odometry; then SolveSLAM() with the constraint (:550): the growing-window solve again, HITL
        # residuals in every pass
        pg, poses = posegraph.solve_growing_window(xy, nrm, off, poses.copy(), max(1, window - 1), window, iterations=iterations, kind=kind,
                                                   device=device, verbose=verbose, backend=backend, initial=poses,
                                                   hitl=[con] if con.n_a + con.n_b else [], loop_closures=lc, features=feats,
                                                   linear_solver=linear_solver, lc_loss=loss)
        out["t_hitl_solve_s"] = time.perf_counter() - t0
        pcg_phase("hitl")
        out["err_hitl_m"] = posegraph.trajectory_error(poses, bag.truth)
        out["hitl_chosen_line_pose"] = [float(v) for v in con.chosen_line_pose]
    if map_output is not None:
        # ---- the vector map of the solved trajectory (Vectorize, solver.cc:581-624)
        if not hasattr(backend, "vectorize"):
            raise RuntimeError("run: map_output needs a backend with vectorize(); backend %r has none" % (backend.name,))
        t0 = time.perf_counter()
        map_lines, _, map_stats = backend.vectorize(poses, xy=xy_lc, offsets=off_lc)  # (outside the stage clocks: not a solve stage)
        out["vectorize_s"] = time.perf_counter() - t0
        if rank == 0:
            hostside.write_map_lines(map_output, map_lines)
        out["map_segments"], out["map_cells"], out["map_rounds"], out["map_flag"] = (int(map_stats[k]) for k in (1, 0, 2, 3))
        out["map_poses"] = [[float(v) for v in p] for p in poses]
    if grid_output is not None:
        # ---- the occupancy grid of the solved trajectory (build-defined: DESIGN.md section 3, "Occupancy grid")
        if not hasattr(backend, "occupancy_grid"):
            raise RuntimeError("run: grid_output needs a backend with occupancy_grid(); backend %r has none" % (backend.name,))
        from nautilus_amd import occupancy
        grid_spec = occupancy.window_spec(poses)
        t0 = time.perf_counter()
        grid, _, _, grid_stats = backend.occupancy_grid(poses, spec=grid_spec, xy=xy_lc, offsets=off_lc)  # (outside the stage clocks)
        out["occupancy_s"] = time.perf_counter() - t0
        if rank == 0:
            hostside.write_occupancy_map(grid_output, grid, grid_spec)
        out["grid_occupied"], out["grid_free"], out["grid_unknown"] = (int(grid_stats[k]) for k in (5, 6, 7))
        out["grid_window"] = [grid_spec.cell_x0, grid_spec.cell_y0, grid_spec.width, grid_spec.height]
        out["grid_poses"] = [[float(v) for v in p] for p in poses]
    out["t_total_s"] = sum(v for k, v in out.items() if k.startswith("t_") and k.endswith("_s"))
    # By owner: the hot path of this repo (every call into the backend: correspondence search, normal equations,
    # gating, scan matching -- "gpu_path_s" with the product's backend, "cpu_path_s" with the oracle's), the sparse
    # solves (the reference's Ceres: out of scope, identical host code under either backend), and the remaining host
    # bookkeeping (assembly of the sparse system in numpy, HITL point selection, the synthetic message).
    key = "gpu_path_s" if backend.name == "hip" else "cpu_path_s"
    out[key] = posegraph.CLOCK["path"]
    out["host_solver_s"] = posegraph.CLOCK["host_solver"]
    out["host_other_s"] = out["t_total_s"] - out[key] - out["host_solver_s"]
    # ... host_other_s by owner (round 5): marshalling at the path's boundary (block lists, the HITL blocks' input arrays,
    # records -> transforms, loop-closure factors); the sparse system's assembly in numpy (the solver stand-in's
    # bookkeeping: Ceres does it inside Solve); GetRelevantPosesForHITL's point selection (host-side HITL curation);
    # and what is left: the harness (ground-truth comparisons, the synthetic HITL message).
    out["marshal_s"] = posegraph.CLOCK["marshal"]
    out["path_setup_s"] = posegraph.CLOCK["path_setup"]  # (of the path seconds: uploads + device allocations of the per-pass batches)
    out["host_assembly_s"] = posegraph.CLOCK["assemble"]
    out["hitl_select_s"] = posegraph.CLOCK["hitl_select"]
    # the linear step: with "host" it is host_solver_s + host_assembly_s; with "device" it is
    # path_linear_s, a part of the path seconds like path_setup_s, and the PCG's counts over all solves
    out["linear_solver"] = linear_solver
    out["path_linear_s"] = posegraph.CLOCK["path_linear"]
    out["pcg_solves"], out["pcg_iterations"] = posegraph.LINEAR_STATS["solves"], posegraph.LINEAR_STATS["iterations"]
    out["pcg_not_converged"] = posegraph.LINEAR_STATS["not_converged"] + posegraph.LINEAR_STATS["breakdowns"]
    out["pcg_by_phase"] = pcg_by_phase  # phase -> [solves, iterations]
    out["hitl_device"] = bool(hitl_device)
    out["lc_submap"] = lc_submap
    out["harness_s"] = out["host_other_s"] - out["marshal_s"] - out["host_assembly_s"] - out["hitl_select_s"]
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=320)
    ap.add_argument("--window", type=int, default=10)
    ap.add_argument("--residual", choices=["point", "normal", "feature"], default="normal",
                    help="LIDARPointResidual on all points (the reference's non-FEATURE mode, solver.cc:308-314), "
                         "LIDARNormalResidual on all points, or the reference's FEATURE mode (solver.cc:297-318): planar "
                         "feature points as LIDARNormalResidual blocks and edge points as LIDARPointResidual blocks")
    ap.add_argument("--hitl-device", action="store_true",
                    help="select the HITL constraint's points and reduce its blocks to normal equations on the GPU")
    ap.add_argument("--normals", choices=["bag", "device"], default="bag",
                    help="the synthetic bag's analytic normals, or normals estimated from the clouds on the GPU")
    ap.add_argument("--lc-submap", type=int, default=0, metavar="K",
                    help="build every loop-closure target's table from the scans t-K .. t+K under the current estimate "
                         "(0: from scan t alone); below %d, the pair gate's minimum separation" % LC_MIN_SEPARATION)
    ap.add_argument("--linear-solver", choices=["host", "device"], default="host",
                    help="the linear step of every solve: scipy on the host, or block-Jacobi PCG on the GPU (with HITL: "
                         "needs --hitl-device)")
    ap.add_argument("--lc-gate", choices=["geometric", "chi-square", "appearance"], default="geometric",
                    help="the loop-closure pair gate: distance and separation, or LCMatcher's chi-square test on the cross-covariance "
                         "blocks of the pose graph (PoseGraph.cross_covariances with --linear-solver's solver), intersected with "
                         "the separation rule, or the nearest earlier scans by ring descriptor (no pose enters; the matcher's "
                         "theta0 comes from the descriptors' aligning rotation)")
    ap.add_argument("--lc-top-k", type=int, default=5, metavar="K", help="with --lc-gate appearance: candidates kept per scan (1..32)")
    ap.add_argument("--lc-sequence", type=int, default=None, metavar="W",
                    help="with --lc-gate appearance: compare the descriptors over a window of 2W + 1 frames around both scans of a "
                         "pair, in both directions of travel (0..8; 0: a single scan's descriptor)")
    ap.add_argument("--lc-sequence-step", type=int, default=None, metavar="S",
                    help="with --lc-sequence: scans between two frames of a window (1..16; 2 W S at most %d)" % LC_MIN_SEPARATION)
    ap.add_argument("--lc-max-score", type=float, default=5000.0, help="the chi-square gate's threshold (lc_matcher.cc:66: 5000)")
    ap.add_argument("--lc-verify", choices=["free-space"], default=None,
                    help="check every match record against the target's free space and drop the contradicted ones "
                         "(not with several ranks or --lc-submap)")
    ap.add_argument("--lc-max-violation", type=int, default=None, metavar="PERMILLE",
                    help="with --lc-verify: the largest share of a source's returns in the target's free space, plus its beams "
                         "through target hits, that is kept (default: freespace.DEFAULT_MAX_PERMILLE)")
    ap.add_argument("--lc-refine", choices=["icp"], default=None,
                    help="refine every match that passed the score gate from its lattice pose to a sub-cell pose by point-to-line "
                         "ICP against the target scan, before --lc-verify and --lc-consistency (not with several ranks)")
    ap.add_argument("--lc-consistency", action="store_true",
                    help="keep only the accepted loop closures of a mutually consistent set (pairwise consistency of the cycles "
                         "they form with the estimate; not with several ranks)")
    ap.add_argument("--lc-min-set", type=int, default=3, metavar="N",
                    help="with --lc-consistency: a consistent set of fewer members is not trusted and no loop closure is kept")
    ap.add_argument("--lc-loss", choices=["none", "huber", "soft-l1", "cauchy"], default="none",
                    help="robust loss of the loop-closure factors in the closure solve and the HITL phase's solve: every record is "
                         "weighed by its own residual instead of entering at full weight")
    ap.add_argument("--lc-loss-scale", type=float, default=1.0, metavar="A",
                    help="with --lc-loss: the loss' scale in units of the weighted residual (at the closures' weight 10, 1.0 is "
                         "0.1 m or 0.1 rad, two cells of the matcher's lattice)")
    ap.add_argument("--lc-factor", choices=["world", "relative"], default="world",
                    help="the loop-closure factor: frozen in the world frame at scalar weights, or relative-pose factors that measure "
                         "the source in the target's frame and carry each match's information (with --lc-refine icp: the refinement's)")
    ap.add_argument("--lc-info-sigma", type=float, default=1.0, metavar="M",
                    help="with --lc-factor relative and --lc-refine icp: the range noise the refinement's H is divided by, squared [m]")
    ap.add_argument("--map-output", metavar="PATH", default=None,
                    help="vectorise the final poses' map on the GPU and write it there, one 'x1,y1,x2,y2' line per wall segment")
    ap.add_argument("--grid-output", metavar="STEM", default=None,
                    help="ray-trace the final poses' occupancy grid on the GPU and write STEM.pgm and STEM.yaml (map_server's pair)")
    ap.add_argument("--movers", type=int, default=0, metavar="N",
                    help="add N synthetic walkers to the bag: discs of radius 0.3 m whose returns replace the walls' behind them")
    ap.add_argument("--drop-transients", action="store_true",
                    help="after the growing-window solve, classify every return by the occupancy planes of all scans on the GPU and "
                         "make the loop-closure tables, --map-output and --grid-output from the scans without their transient returns")
    ap.add_argument("-v", action="store_true")
    a = ap.parse_args()
    if not 0 <= a.lc_submap < LC_MIN_SEPARATION:
        ap.error("--lc-submap %d: the radius must be in [0, %d): a source must never be in its target's submap"
                 % (a.lc_submap, LC_MIN_SEPARATION))
    if (a.lc_sequence is not None or a.lc_sequence_step is not None) and a.lc_gate != "appearance":
        ap.error("--lc-sequence and --lc-sequence-step need --lc-gate appearance")
    if a.lc_sequence_step is not None and a.lc_sequence is None:
        ap.error("--lc-sequence-step needs --lc-sequence")
    seq_w, seq_step = a.lc_sequence or 0, 1 if a.lc_sequence_step is None else a.lc_sequence_step
    if not (0 <= seq_w <= 8 and 1 <= seq_step <= 16 and 2 * seq_w * seq_step <= LC_MIN_SEPARATION):
        ap.error("--lc-sequence %d in 0..8, --lc-sequence-step %d in 1..16, twice their product at most %d"
                 % (seq_w, seq_step, LC_MIN_SEPARATION))
    if a.lc_loss != "none" and not (math.isfinite(a.lc_loss_scale) and a.lc_loss_scale > 0):
        ap.error("--lc-loss-scale %r: finite and > 0" % (a.lc_loss_scale,))
    rank, world, local = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1")), \
        int(os.environ.get("LOCAL_RANK", "0"))
    if a.lc_refine and world > 1:
        ap.error("--lc-refine with several ranks (the refinement has no sharded path)")
    if "RANK" in os.environ:  # python -m torch.distributed.run --nproc-per-node N examples/slam_loop.py ...
        import torch
        import torch.distributed as dist
        from nautilus_amd import _lib
        torch.cuda.set_device(local)
        _lib.check(_lib.load().nhip_set_device(local))
        saved = os.dup(1)
        os.dup2(2, 1)  # RCCL prints its banner on stdout
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        dist.barrier()
        os.dup2(saved, 1)
    res = run(a.scans, a.window, verbose=a.v and rank == 0, residual=a.residual, rank=rank, world=world,
              device="cuda:%d" % local, hitl_device=a.hitl_device, normals=a.normals, lc_submap=a.lc_submap,
              linear_solver=a.linear_solver, lc_gate=a.lc_gate, lc_max_score=a.lc_max_score, map_output=a.map_output,
              grid_output=a.grid_output, lc_verify=a.lc_verify, lc_max_violation=a.lc_max_violation, lc_top_k=a.lc_top_k,
              lc_consistency=a.lc_consistency, lc_min_set=a.lc_min_set, lc_sequence=seq_w, lc_sequence_step=seq_step,
              lc_loss=None if a.lc_loss == "none" else a.lc_loss, lc_loss_scale=a.lc_loss_scale, movers=a.movers,
              drop_transients=a.drop_transients, lc_refine=a.lc_refine, lc_factor=None if a.lc_factor == "world" else a.lc_factor,
              lc_info_sigma_m=a.lc_info_sigma)
    res["world_size"] = world
    if rank == 0 and "transient_stats" in res:
        s = res["transient_stats"]
        print("transients: kept %d of %d returns (static %d, transient %d, unobserved %d, invalid %d); %d of %d scans kept none"
              % (s["points_static"] + s["points_unobserved"], sum(s[k] for k in list(s)[:4]), s["points_static"], s["points_transient"],
                 s["points_unobserved"], s["points_invalid"], s["scans_emptied"], s["scans_processed"]))
    if rank == 0:
        print(json.dumps(res))
    if "RANK" in os.environ:
        dist.destroy_process_group()
