"""Host-side pose-graph driver over the GPU hot path.

The reference hands its residual blocks to Ceres (SPARSE_SCHUR, solver.cc:266-275, 335-356), which
is not installable here; this module is the small caller that lets the whole loop run on the
batched API instead:
  * ICP blocks of the sliding window (solver.cc:321-333): correspondence search (K5) and per-block
    6x6 normal equations on the GPU (nhip_corr_search_dev, nhip_resid_lidar_normal_eq_dev);
  * odometry factors (OdometryResidual, slam_residuals.h:18-40; AddOdomFactors solver.cc:370-387)
    and loop-closure constraints from the scan matcher ("Add Odometry residual using the returned
    relative transform", the TODO at solver.cc:651-660), both evaluated by nhip_resid_odometry_dev;
  * HITL constraints (solver.cc:479-559): PointToLineResidual blocks of the points the user's two
    segments select, every block against line_a and one shared `chosen_line_pose` parameter block
    (AddHITLResiduals, solver.cc:515-532), evaluated by nhip_resid_point_to_line -- or, for a constraint selected on
    the GPU (hitl.select), reduced there to per-block normal equations (nhip_resid_point_to_line_normal_eq_dev);
  * Gauss-Newton with Levenberg damping on the assembled sparse system (scipy.sparse on the
    host: N poses x 3 + 3 per HITL constraint), first pose held constant (solver.cc:384-386) -- or, with
    solve(linear_solver="device"), on the block-sparse system assembled and solved on the GPU (linsolve.py:
    nhip_bsr_assemble_dev, nhip_bsr_pcg_dev), every 28-double row staying there.
By default only the linear solve and the bookkeeping are host work; every residual, Jacobian and nearest
neighbour comes from the backend -- HipBackend (the product: libnautilus_hip) unless a test or the
bench's cpu_baseline leg injects another one (oracle/cpu_backend.py times the same loop on the CPU
restatement; the product never imports it).
"""
import contextlib
import ctypes as C
import math
import time

import numpy as np

from . import _lib
from ._lib import check
from .correspondence import IcpBatch, window_pairs


# Where the loop's wall-clock goes, by owner (seconds since the last reset): "path" = calls into the backend -- the hot
# path of this repo: correspondence search, residuals / normal equations, gating, scan matching (every one returns
# host data, so the device is drained when the clock stops); "host_solver" = the sparse linear solves (Ceres' job in
# the reference: out of scope, the same code whatever the backend); the rest of a run is host bookkeeping.
# "marshal" = host work at the path's boundary: building the block lists and input arrays the backend calls take and
# turning their outputs into what the caller asked for; "assemble" = the sparse system's assembly from the per-block
# normal equations and factor Jacobians (numpy: what Ceres does inside its solve, like "host_solver"); "hitl_select" =
# GetRelevantPosesForHITL's point selection (host-side HITL curation, solver.cc:479-513); "path_linear" = of the path
# seconds, the device linear solver's (structure upload, assembly, PCG: solve(linear_solver="device")).
CLOCK = {"path": 0.0, "host_solver": 0.0, "marshal": 0.0, "assemble": 0.0, "hitl_select": 0.0, "path_setup": 0.0,
         "path_linear": 0.0}
# The device linear solver's solves since the last reset, over every PoseGraph: solves, their PCG iterations, the solves
# that ended at max_iters (flag 1) and the breakdowns (flag 2).  A PoseGraph keeps its own in .linear_stats.
LINEAR_STATS = {"solves": 0, "iterations": 0, "not_converged": 0, "breakdowns": 0}


def clock_reset():
    for k in CLOCK:
        CLOCK[k] = 0.0
    for k in LINEAR_STATS:
        LINEAR_STATS[k] = 0


@contextlib.contextmanager
def clocked(key):
    t0 = time.perf_counter()
    try:
        yield
    finally:
        CLOCK[key] += time.perf_counter() - t0


def compose(pose, rel):
    """pose (x, y, th) o rel (tx, ty, th): the pose of A given B and A-in-B (solver.cc:640-648)."""
    c, s = math.cos(pose[2]), math.sin(pose[2])
    return np.array([pose[0] + c * rel[0] - s * rel[1], pose[1] + s * rel[0] + c * rel[1], pose[2] + rel[2]])


class HipBackend:
    """Every evaluation on the MI355X through the C ABI."""
    name = "hip"

    def __init__(self, device="cuda:0"):
        import torch
        self.torch, self.dev, self.lib = torch, torch.device(device), _lib.load()
        from .correspondence import DeviceArena
        self.arena = DeviceArena()  # the clouds and the work buffers of the ICP batches, kept across problem builds
        self._dedicated = {}        # id(xy) -> (xy, DeviceArena): clouds whose batches do not share `arena` (dedicate())

    def icp(self, xy, normals, offsets, block_src, block_tgt, outlier_threshold):
        arena = self._dedicated.get(id(xy), (None, self.arena))[1]
        return _HipIcp(IcpBatch(xy, normals, offsets, block_src, block_tgt, str(self.dev), outlier_threshold, arena=arena))

    def dedicate(self, xy):
        """Batches on the cloud `xy` (by identity) get an arena of their own from now on.  One batch owns an arena at a time
        (DeviceArena): two batches that are evaluated in turn -- the planar and the edge batch of a FEATURE-mode graph -- would
        take a shared one from each other at every evaluation and search again each time.  Feature clouds are tiny."""
        from .correspondence import DeviceArena
        if id(xy) not in self._dedicated:
            self._dedicated[id(xy)] = (xy, DeviceArena())  # (the reference to xy keeps its id its own)

    def features(self, xy, normals, offsets, spec=None):
        """The planar and the edge points of every scan, extracted on the GPU (features.extract), as the pair of packed clouds
        ((xy_p, nrm_p, off_p), (xy_e, nrm_e, off_e)) that PoseGraph(..., features=) takes."""
        from . import features
        return features.extract(xy, offsets, spec, device=str(self.dev)).clouds(xy, normals, offsets)

    def normals(self, xy, offsets, spec=None):
        """The normals of every point of the packed scans, estimated on the GPU (normals.estimate): float32 (n, 2)."""
        from . import normals
        return normals.estimate(xy, offsets, spec, device=str(self.dev))

    def vectorize(self, poses, spec=None, xy=None, offsets=None):
        """The vector map at `poses`, made on the GPU (vectorize.py: Solver::Vectorize): (lines float32 (n, 4), records,
        stats).  Runs on the clouds the arena already holds (the last ICP problem's upload); with xy and offsets given, on
        those -- uploaded only if they are not the arena's (a FEATURE-mode solve keeps feature clouds there).  spec=None: the
        defaults on the window of every pose +- 30 m."""
        from . import vectorize
        spec = vectorize.window_spec(poses) if spec is None else spec
        held = self.arena.clouds
        if xy is not None and (held is None or held[4][0] is not xy):
            return vectorize.vectorize(xy, offsets, poses, spec, device=str(self.dev))
        if held is None:
            raise RuntimeError("HipBackend.vectorize: no clouds on the device yet (the first icp() batch uploads them): pass xy, offsets")
        return vectorize.vectorize_on_device(held[1], held[3], int(held[3].numel()) - 1, poses, spec)

    def occupancy_grid(self, poses, spec=None, xy=None, offsets=None):
        """The occupancy grid at `poses`, ray-traced on the GPU (occupancy.py): (grid int8 (H, W), hits, misses, stats).  Runs
        on the clouds the arena already holds, or on xy and offsets, exactly as vectorize() chooses.  spec=None: the defaults
        on the window of every pose +- 30 m."""
        from . import occupancy
        spec = occupancy.window_spec(poses) if spec is None else spec
        held = self.arena.clouds
        if xy is not None and (held is None or held[4][0] is not xy):
            return occupancy.occupancy_grid(xy, offsets, poses, spec, device=str(self.dev))
        if held is None:
            raise RuntimeError("HipBackend.occupancy_grid: no clouds on the device yet (the first icp() batch uploads them): pass xy, offsets")
        return occupancy.occupancy_grid_on_device(held[1], held[3], int(held[3].numel()) - 1, poses, spec)

    def drop_transients(self, poses, occ_spec=None, xy=None, offsets=None, **overrides):
        """The scans without their transient returns at `poses` (transient.py): one occupancy trace, then the filter on its
        planes, in-stream -- transient.StaticScans, whose (xy, offsets) stand in for the input's.  Runs on the clouds the
        arena already holds, or on xy and offsets, exactly as vectorize() chooses.  occ_spec=None: the occupancy defaults on
        the window of every pose +- 30 m; overrides: fields of the transient spec (support_radius, min_through,
        transient_permille)."""
        from . import occupancy, transient
        occ_spec = occupancy.window_spec(poses) if occ_spec is None else occ_spec
        held = self.arena.clouds
        if xy is not None and (held is None or held[4][0] is not xy):
            return transient.static_scans(xy, offsets, poses, occ_spec, device=str(self.dev), **overrides)
        if held is None:
            raise RuntimeError("HipBackend.drop_transients: no clouds on the device yet (the first icp() batch uploads them): pass xy, offsets")
        return transient.static_scans_on_device(held[1], held[3], int(held[3].numel()) - 1, poses, occ_spec, **overrides)

    def reserve_icp(self, offsets, window):
        """Work buffers for the largest problem of a growing-window solve (all (i, j), j in [i - window, i)): allocated once."""
        off = np.asarray(offsets, dtype=np.int64)
        per = np.minimum(np.arange(len(off) - 1), int(window))  # blocks whose source is scan i
        self.arena.reserve(self.torch, self.dev, int((np.diff(off) * per).sum()), int(per.sum()))

    def odometry(self, pose_i, pose_j, t_odom, r_odom, tw, rw, poses):
        """OdometryResidual blocks at `poses` (n, 3): residuals (F, 3), Jacobians (F, 3, 3) x 2."""
        n = len(pose_i)
        r, ji, jj = np.empty((n, 3)), np.empty((n, 3, 3)), np.empty((n, 3, 3))
        P = np.ascontiguousarray(poses, dtype=np.float64)
        check(self.lib.nhip_resid_odometry(_lib.ptr(t_odom), _lib.ptr(r_odom), _lib.ptr(pose_i), _lib.ptr(pose_j), n,
                                           float(tw), float(rw), _lib.ptr(P), len(P), _lib.ptr(r), _lib.ptr(ji), _lib.ptr(jj)))
        return r, ji, jj

    def point_to_line(self, segments, points, point_block, block_pose, block_line, poses, line_poses):
        """PointToLineResidual blocks: residuals (n,), d/d pose (n, 3), d/d line_pose (n, 3)."""
        n = len(points)
        r, j0, j1 = np.empty(n), np.empty((n, 3)), np.empty((n, 3))
        P, Lp = np.ascontiguousarray(poses, dtype=np.float64), np.ascontiguousarray(line_poses, dtype=np.float64)
        check(self.lib.nhip_resid_point_to_line(_lib.ptr(segments), _lib.ptr(points), _lib.ptr(point_block), n,
                                                _lib.ptr(block_pose), _lib.ptr(block_line), len(block_pose), _lib.ptr(P), len(P),
                                                _lib.ptr(Lp), len(Lp), _lib.ptr(r), _lib.ptr(j0), _lib.ptr(j1)))
        return r, j0, j1

    def hitl_select(self, xy, offsets, poses, line_a, line_b, line_width=0.05, point_threshold=10):
        """GetRelevantPosesForHITL on the GPU (hitl.select): a DeviceHitlConstraint, its points packed on the device."""
        from . import hitl
        return hitl.select(self, xy, offsets, poses, line_a, line_b, line_width, point_threshold)

    def point_to_line_normal_eq(self, constraint, poses, line_poses, line_index):
        """The normal equations of a DeviceHitlConstraint's blocks at `poses`, every block against line a under
        line_poses[line_index]: (n_blocks, 28) float64 in the layout of the ICP blocks' (nhip_resid_point_to_line_normal_eq_dev)."""
        torch, con = self.torch, constraint
        if con.n_blocks == 0:
            return np.zeros((0, 28))
        P, Lp = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3), np.ascontiguousarray(line_poses, dtype=np.float64).reshape(-1, 3)
        d_out = self.point_to_line_normal_eq_dev(con, torch.from_numpy(P).to(self.dev), torch.from_numpy(Lp).to(self.dev), line_index)
        out = d_out.cpu().numpy()
        check(self.lib.nhip_dev_status(C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream), None))
        return out

    def point_to_line_normal_eq_dev(self, constraint, d_poses, d_line_poses, line_index):
        """The same with everything on the device: d_poses (n, 3) and d_line_poses (m, 3) float64 tensors in, the
        (n_blocks, 28) tensor out; nothing is downloaded and nhip_dev_status is the caller's to check."""
        torch, con = self.torch, constraint
        d_out = torch.empty((con.n_blocks, 28), dtype=torch.float64, device=self.dev)
        if con.n_blocks == 0:
            return d_out
        sp = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)
        check(self.lib.nhip_resid_point_to_line_normal_eq_dev(con.d_segments.data_ptr(), con.d_points.data_ptr(),
                                                              con.d_block_offsets.data_ptr(), con.d_block_pose.data_ptr(),
                                                              con.d_block_line(line_index).data_ptr(), con.n_blocks,
                                                              d_poses.data_ptr(), d_poses.shape[0], d_line_poses.data_ptr(),
                                                              d_line_poses.shape[0], d_out.data_ptr(), sp))
        return d_out

    def odometry_normal_eq_dev(self, factors, d_poses, d_weights=None, loss=None):
        """The normal equations of OdometryFactors at the (n, 3) float64 device tensor d_poses: (F, 28) float64 on the
        device over [pose_i | pose_j] (nhip_resid_odometry_normal_eq_dev).  The factors' arrays go up once.
        Factors that carry a loss (factors.loss, or `loss` in its place) go through nhip_resid_odometry_robust_normal_eq_dev:
        the rows of the reweighted factors, rho in slot 27, and {s, rho, rho', sqrt(rho')} per factor into the (F, 4) float64
        device tensor d_weights if one is given.  Without a loss the call is the plain one."""
        torch, fac = self.torch, factors
        loss = loss if loss is not None else getattr(fac, "loss", None)
        if d_weights is not None and loss is None:
            raise ValueError("odometry_normal_eq_dev: d_weights needs factors with a loss")
        d_out = torch.empty((fac.n, 28), dtype=torch.float64, device=self.dev)
        if fac.n == 0:
            return d_out
        if getattr(fac, "_dev", None) is None or fac._dev[0] != self.dev:
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
            fac._dev = (self.dev, t(fac.t_odom), t(fac.r_odom), t(fac.pose_i), t(fac.pose_j))
        _, d_t, d_r, d_i, d_j = fac._dev
        if loss is not None:
            spec = loss.spec()
            check(self.lib.nhip_resid_odometry_robust_normal_eq_dev(
                d_t.data_ptr(), d_r.data_ptr(), d_i.data_ptr(), d_j.data_ptr(), fac.n, fac.tw, fac.rw, C.byref(spec),
                d_poses.data_ptr(), d_poses.shape[0], d_out.data_ptr(), None if d_weights is None else d_weights.data_ptr(),
                C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)))
            return d_out
        check(self.lib.nhip_resid_odometry_normal_eq_dev(d_t.data_ptr(), d_r.data_ptr(), d_i.data_ptr(), d_j.data_ptr(), fac.n,
                                                         fac.tw, fac.rw, d_poses.data_ptr(), d_poses.shape[0], d_out.data_ptr(),
                                                         C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)))
        return d_out

    def relative_pose(self, z, info, pose_i, pose_j, poses):
        """RelativePoseFactors' arrays at `poses` (n, 3): the whitened residuals (F, 3) and Jacobians (F, 3, 3) x 2
        (nhip_resid_relpose; DESIGN.md section 3, "Relative-pose factors")."""
        n = len(pose_i)
        r, ji, jj = np.empty((n, 3)), np.empty((n, 3, 3)), np.empty((n, 3, 3))
        P = np.ascontiguousarray(poses, dtype=np.float64)
        check(self.lib.nhip_resid_relpose(_lib.ptr(z), _lib.ptr(info), _lib.ptr(pose_i), _lib.ptr(pose_j), n, _lib.ptr(P), len(P),
                                          _lib.ptr(r), _lib.ptr(ji), _lib.ptr(jj), None, None))
        return r, ji, jj

    def relative_pose_normal_eq_dev(self, factors, d_poses, d_weights=None, loss=None):
        """The rows of RelativePoseFactors at the (n, 3) float64 device tensor d_poses: (F, 28) float64 on the device over
        [pose_i | pose_j] (nhip_resid_relpose_normal_eq_dev), under the factors' loss (or `loss` in its place; None: none), and
        {s, rho, rho', sqrt(rho')} per factor into the (F, 4) float64 device tensor d_weights if one is given.  The factors'
        arrays go up once."""
        torch, fac = self.torch, factors
        loss = loss if loss is not None else getattr(fac, "loss", None)
        d_out = torch.empty((fac.n, 28), dtype=torch.float64, device=self.dev)
        if fac.n == 0:
            return d_out
        if getattr(fac, "_dev", None) is None or fac._dev[0] != self.dev:
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
            fac._dev = (self.dev, t(fac.z), t(fac.info), t(fac.pose_i), t(fac.pose_j))
        _, d_z, d_l, d_i, d_j = fac._dev
        spec = None if loss is None else loss.spec()
        check(self.lib.nhip_resid_relpose_normal_eq_dev(
            d_z.data_ptr(), d_l.data_ptr(), d_i.data_ptr(), d_j.data_ptr(), fac.n, None if spec is None else C.byref(spec),
            d_poses.data_ptr(), d_poses.shape[0], d_out.data_ptr(), None if d_weights is None else d_weights.data_ptr(), None,
            C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)))
        return d_out

    def device_system(self, structure, fixed=()):
        """The device arrays of a linsolve.BlockStructure -- values, gradient, x, the PCG workspace -- and its two calls
        (linsolve.DeviceSystem: nhip_bsr_assemble_dev, nhip_bsr_pcg_dev)."""
        from . import linsolve
        return linsolve.DeviceSystem(self, structure, fixed)

    def scatter_scores(self, xy, offsets):
        """LCCandidateFilter's scatter-matrix score of every scan (nhip_lc_scatter_scores)."""
        from . import csm
        st = csm.ScanTable(xy, offsets)
        out = np.empty(st.n_scans)
        check(self.lib.nhip_lc_scatter_scores(st._h, _lib.ptr(out)))
        st.close()
        return out

    def place_candidates(self, xy, offsets, ids, spec=None):
        """Loop-closure candidates by appearance among the scans `ids` (ascending), from no pose at all (place.py:
        nhip_place_candidates): (records int32 (n_ids, K, 4) = {j, shift, dist, bits_j}, stats int64 (8,))."""
        from . import csm, place
        # Only the scans the list names go to the device, as in match(): the others keep their ids as empty scans.
        off = np.asarray(offsets, dtype=np.int64)
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        if len(ids) and (ids.min() < 0 or ids.max() >= len(off) - 1):
            raise ValueError("place_candidates: an id outside the %d scans" % (len(off) - 1))
        lengths = np.zeros(len(off) - 1, dtype=np.int64)
        lengths[ids] = np.diff(off)[ids]
        xy = np.asarray(xy, dtype=np.float32).reshape(-1, 2)
        xy = np.concatenate([xy[off[i]:off[i + 1]] for i in ids]) if len(ids) else xy[:0]
        st = csm.ScanTable(xy, np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32))
        try:
            return place.candidates(st, ids, spec)
        finally:
            st.close()

    def place_sequence_candidates(self, xy, offsets, ids, spec=None, seq=None):
        """Loop-closure candidates by sequence among the scans `ids` (ascending): the appearance match over a window of frames
        around both scans of a pair (place.py: nhip_place_seq_candidates): (records int32 (n_ids, K, 8) = {j, shift, dist,
        bits_j, seq, sum, frames, direction}, stats int64 (8,))."""
        from . import csm, place
        spec = place.default_spec() if spec is None else spec
        seq = place.default_seq_spec() if seq is None else seq
        # The scans the list names AND every window frame ids +- d step inside the scans go to the device: a frame that stayed
        # behind would be a scan without bits.  The others keep their ids as empty scans.
        off = np.asarray(offsets, dtype=np.int64)
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        n = len(off) - 1
        if len(ids) and (ids.min() < 0 or ids.max() >= n):
            raise ValueError("place_sequence_candidates: an id outside the %d scans" % n)
        reach = np.arange(-int(seq.half_window), int(seq.half_window) + 1, dtype=np.int64) * int(seq.step)
        frames = np.unique(ids.astype(np.int64)[:, None] + reach[None, :])
        frames = frames[(frames >= 0) & (frames < n)]
        lengths = np.zeros(n, dtype=np.int64)
        lengths[frames] = np.diff(off)[frames]
        xy = np.asarray(xy, dtype=np.float32).reshape(-1, 2)
        xy = np.concatenate([xy[off[i]:off[i + 1]] for i in frames]) if len(frames) else xy[:0]
        st = csm.ScanTable(xy, np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32))
        try:
            return place.sequence_candidates(st, ids, spec, seq)
        finally:
            st.close()

    def consistent_set(self, poses, src, tgt, rel, spec=None):
        """The mutually consistent set of the loop closures (src, tgt, rel) under the trajectory `poses` (consistency.py:
        nhip_consistency): (members int32 (M,) in pick order, -1 behind them; n_members; stats int64 (8,))."""
        from . import consistency
        return consistency.consistent_set(consistency.prepare(poses, src, tgt, rel), spec)

    def refine_matches(self, xy, normals, offsets, pair_src, pair_tgt, theta0, records, grid_spec, search, spec=None, pair_origin=None):
        """The match records refined on the GPU from their lattice poses by point-to-line ICP against the target scans
        (refine.py: nhip_refine_start_poses, nhip_refine_icp_dev; DESIGN.md section 3, "Match refinement"): the refined array
        (hostside.REFINED_DTYPE), equal to hostside.refine_matches' bit for bit.  pair_tgt are scan ids."""
        from . import refine
        torch = self.torch
        pair_src = np.ascontiguousarray(pair_src, dtype=np.int32).reshape(-1)
        pair_tgt = np.ascontiguousarray(pair_tgt, dtype=np.int32).reshape(-1)
        off = np.ascontiguousarray(offsets, dtype=np.int32)
        n, n_scans = len(pair_src), len(off) - 1
        if len(pair_tgt) != n or (n and (min(pair_src.min(), pair_tgt.min()) < 0 or max(pair_src.max(), pair_tgt.max()) >= n_scans)):
            raise ValueError("refine_matches: pair arrays differ in length or name a scan outside the %d scans" % n_scans)
        pose0 = refine.start_poses(records, theta0, grid_spec, search, pair_origin)
        if n == 0:
            return np.zeros(0, dtype=refine.REFINED_DTYPE)
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(self.dev)
        d_xy, d_nrm = t(np.asarray(xy).reshape(-1, 2), np.float32), t(np.asarray(normals).reshape(-1, 2), np.float32)
        if d_xy.shape != d_nrm.shape or d_xy.shape[0] != int(off[-1]):
            raise ValueError("refine_matches: xy, normals and offsets disagree")
        d_out = refine.icp_on_device(d_xy, d_nrm, t(off, np.int32), n_scans, t(pair_src, np.int32), t(pair_tgt, np.int32),
                                     t(pose0, np.float64), n, spec)
        out = refine.records_from(d_out)
        check(self.lib.nhip_dev_status(C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream), None))
        return out

    def pair_gate(self, poses, candidates, max_range, min_separation):
        P = np.ascontiguousarray(poses, dtype=np.float64)
        cand = np.ascontiguousarray(candidates, dtype=np.int32)
        flags = np.zeros((len(cand), len(cand)), dtype=np.uint8)
        check(self.lib.nhip_lc_pair_gate(_lib.ptr(P), len(P), _lib.ptr(cand), len(cand), float(max_range),
                                         int(min_separation), _lib.ptr(flags)))
        return flags

    def chi_square_gate(self, poses, pair_src, pair_tgt, cov, max_score=5000.0):
        """LCMatcher's chi-square test of n (source, candidate) pairs given their cross-covariance blocks
        (nhip_lc_chi_square_gate; lc_matcher.cc:50-74): (scores float64, flags uint8)."""
        P = np.ascontiguousarray(poses, dtype=np.float64)
        src = np.ascontiguousarray(pair_src, dtype=np.int32)
        tgt = np.ascontiguousarray(pair_tgt, dtype=np.int32)
        cov = np.ascontiguousarray(cov, dtype=np.float32).reshape(-1, 4)
        if not len(cov) == len(src) == len(tgt):
            raise ValueError("chi_square_gate: one covariance block per pair")
        scores, flags = np.zeros(len(src)), np.zeros(len(src), dtype=np.uint8)
        check(self.lib.nhip_lc_chi_square_gate(_lib.ptr(P), len(P), _lib.ptr(src), _lib.ptr(tgt), _lib.ptr(cov), len(src),
                                               float(max_score), _lib.ptr(scores), _lib.ptr(flags)))
        return scores, flags

    def localize(self, xy, offsets, priors, grid, occ_spec, grid_spec=None, search=None, min_score=None, cell_bits=16, **kw):
        """The packed scans localised in a finished occupancy grid from their prior poses, on this backend's device
        (localize.localize; DESIGN.md section 3, "Map windows"): the windows of the grid around the priors gathered on the GPU,
        their tables built, every scan matched against its own.  Returns the dict of poses (n, 3), records, origins, rejected
        and points_per_window."""
        from . import localize
        return localize.localize(xy, offsets, priors, grid, occ_spec, grid_spec=grid_spec, search=search, min_score=min_score,
                                 cell_bits=cell_bits, device=str(self.dev), **kw)

    def global_localize(self, xy, offsets, grid, occ_spec, spec=None, grid_spec=None, search=None, min_score=None, cell_bits=16, **kw):
        """The packed scans localised in a finished occupancy grid from NO prior, on this backend's device
        (relocalize.global_localize; DESIGN.md section 3, "Range signatures"): K proposals per scan from the range signatures of
        the map, every (scan, proposal) entry through localize(), the best-scoring entry per scan.  Returns the dict of poses
        (n, 3), rank, proposals, candidates, anchors, records and stats."""
        from . import relocalize
        return relocalize.global_localize(xy, offsets, grid, occ_spec, spec=spec, grid_spec=grid_spec, search=search, min_score=min_score,
                                          cell_bits=cell_bits, device=str(self.dev), **kw)

    def match(self, xy, offsets, pair_src, pair_tgt, theta0, cell_bits=16, submap_radius=0, poses=None, freespace=None,
              grid_spec=None, search=None):
        """Batched loop-closure scan matching (BASELINE config #2 lattice): (records, spec, search).
        Only the scans the list names go to the device (the candidate scans of a 10,000-scan bag are ~150: 1.3 MB instead
        of the bag's 86 MB, whose upload cost more than matching the 3,275 pairs).
        submap_radius K > 0: every target's table is built from its SUBMAP -- the scans t - K .. t + K placed in t's frame
        by `poses` (n_scans, 3), merged on the device (nhip_submaps_gather_dev) from the same sub-bag, which then holds the
        members too.  0: the tables of the target scans alone; no gather is launched.
        freespace: a freespace.spec() -- the free-space check of every record ("Free-space check") is made
        inside the call, while the tables are on the device: the targets' free planes traced, the records classified where
        the matcher left them; returns (records, spec, search, counts int32 (n, 8)).  None: the three-tuple, no extra launch.
        Not with submap_radius > 0 (a submap's free space needs one ray origin per member).
        grid_spec, search: another table spec / lattice than config #2's (tests on small tables, hostside.localize); None: those."""
        from . import csm, hostside
        if freespace is not None and int(submap_radius) > 0:
            raise ValueError("match: freespace with submap_radius %d: the free-space check has no submap targets" % int(submap_radius))
        spec = csm.grid_spec(30.0, 0.05, 2.0, 1e-10, 40, cell_bits) if grid_spec is None else grid_spec
        search = csm.search_spec(61, 81, 81, math.radians(1.0)) if search is None else \
            _lib.Search(search.n_theta, search.nx, search.ny, search.flags, search.theta_step)  # (a copy: the flags are edited below)
        pair_src, pair_tgt = np.asarray(pair_src), np.asarray(pair_tgt)
        submap_radius = int(submap_radius)
        if submap_radius < 0 or (submap_radius > 0 and poses is None):
            raise ValueError("match: submap_radius %d needs poses and must not be negative" % submap_radius)
        members = None
        if submap_radius > 0 and len(pair_src):
            targets = np.unique(pair_tgt)
            member_scan, member_offsets = hostside.submap_members(len(offsets) - 1, targets, submap_radius)
            member_aff = csm.submap_member_affines(poses, np.repeat(targets, np.diff(member_offsets)), member_scan)
            members = (targets, member_scan, member_aff, member_offsets)
        used = np.unique(np.concatenate([pair_src, pair_tgt] + ([members[1]] if members else [])))
        off = np.asarray(offsets, dtype=np.int64)
        xy2 = np.asarray(xy, dtype=np.float32).reshape(-1, 2)
        sub_xy = np.concatenate([xy2[off[i]:off[i + 1]] for i in used]) if len(used) else np.zeros((0, 2), np.float32)
        sub_off = np.concatenate([[0], np.cumsum(off[used + 1] - off[used])]).astype(np.int32)
        src, tgt = np.searchsorted(used, pair_src).astype(np.int32), np.searchsorted(used, pair_tgt).astype(np.int32)
        ids = np.unique(tgt).astype(np.int32)
        slot = np.searchsorted(ids, tgt).astype(np.int32)
        n, lib, torch, dev = len(src), self.lib, self.torch, self.dev
        if n == 0:
            none = (np.zeros(0, dtype=csm.MATCH_DTYPE), spec, search)
            return none if freespace is None else none + (np.zeros((0, 8), dtype=np.int32),)
        if len(sub_off) > 1 and int(np.diff(sub_off).max()) <= _lib.NHIP_SHORT_SCAN_POINTS:
            search.flags |= _lib.NHIP_SEARCH_SHORT_SCANS
        # Device buffers from torch's caching allocator (the tables of 150 targets are 1.8 GB: a hipMalloc / hipFree pair of
        # that size per call cost several times the match), the device-pointer entry points on torch's current stream.
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        d_xy, d_off, d_ids, d_src, d_slot = t(sub_xy), t(sub_off), t(ids), t(src), t(slot)
        rot0 = np.empty((n, 2))
        check(lib.nhip_csm_rot0(_lib.ptr(np.ascontiguousarray(theta0, dtype=np.float64)), None, n, _lib.ptr(rot0)))
        d_rot0, d_delta = t(rot0), t(csm.delta_table(search))
        # (nhip_grid_build_dev zero-fills the slots itself; only the 256 bytes of read slack behind them are this caller's)
        d_grids = torch.empty(lib.nhip_grids_bytes(C.byref(spec), len(ids)), dtype=torch.uint8, device=dev)
        d_grids[-256:].zero_()
        ws_g = lib.nhip_grid_workspace_bytes(C.byref(spec), len(ids))
        d_ws_g = torch.empty(ws_g, dtype=torch.uint8, device=dev)
        ws_m = lib.nhip_csm_workspace_bytes(n)
        d_ws_m = torch.empty(ws_m, dtype=torch.uint8, device=dev)
        d_keys = torch.empty(n, dtype=torch.int64, device=dev)
        d_out = torch.empty((n, 4), dtype=torch.int32, device=dev)
        sp = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        n_sub = len(sub_off) - 1
        if members:
            # (ids, the sorted distinct targets in sub-bag numbering, are `targets` in the bag's: slot t is target t's submap)
            _, member_scan, member_aff, member_offsets = members
            m_sub = np.searchsorted(used, member_scan).astype(np.int32)
            total = int((sub_off[m_sub + 1] - sub_off[m_sub]).sum())
            d_mscan, d_maff, d_moff = t(m_sub), t(member_aff), t(member_offsets)
            d_gxy = torch.empty((max(total, 1), 2), dtype=torch.float32, device=dev)
            d_goff = torch.empty(len(ids) + 1, dtype=torch.int32, device=dev)
            d_gids = torch.arange(len(ids), dtype=torch.int32, device=dev)
            check(lib.nhip_submaps_gather_dev(d_xy.data_ptr(), d_off.data_ptr(), n_sub, d_mscan.data_ptr(), d_maff.data_ptr(),
                                              d_moff.data_ptr(), len(ids), d_gxy.data_ptr(), total, d_goff.data_ptr(), sp))
            check(lib.nhip_grid_build_dev(d_gxy.data_ptr(), d_goff.data_ptr(), len(ids), d_gids.data_ptr(), len(ids),
                                          C.byref(spec), d_grids.data_ptr(), d_ws_g.data_ptr(), ws_g, sp))
        else:
            check(lib.nhip_grid_build_dev(d_xy.data_ptr(), d_off.data_ptr(), n_sub, d_ids.data_ptr(), len(ids), C.byref(spec),
                                          d_grids.data_ptr(), d_ws_g.data_ptr(), ws_g, sp))
        check(lib.nhip_csm_match_dev(d_xy.data_ptr(), d_off.data_ptr(), n_sub, d_grids.data_ptr(), len(ids), C.byref(spec), d_src.data_ptr(),
                                     d_slot.data_ptr(), d_rot0.data_ptr(), d_delta.data_ptr(), None, n, C.byref(search),
                                     d_keys.data_ptr(), d_out.data_ptr(), None, d_ws_m.data_ptr(), ws_m, sp))
        if freespace is not None:
            from . import freespace as fs
            d_free = fs.trace_on_device(d_xy, d_off, n_sub, d_ids, len(ids), spec, d_grids)
            d_counts = fs.check_on_device(d_xy, d_off, n_sub, d_grids, len(ids), spec, d_src, d_slot, d_rot0, d_delta, None, n,
                                          search, d_free, d_out, freespace)
        m = d_out.cpu().numpy().view(csm.MATCH_DTYPE).reshape(-1).copy()
        if freespace is None:
            return m, spec, search
        counts = d_counts.cpu().numpy()
        check(lib.nhip_dev_status(sp, None))
        return m, spec, search, counts


class _HipIcp:
    def __init__(self, batch):
        self.b = batch
        self.block_src, self.block_tgt = batch.block_src, batch.block_tgt

    def set_poses(self, poses):
        self.b.set_poses(poses)

    def search(self):
        return self.b.search()

    def normal_equations(self, kind):
        return self.b.normal_equations(kind).cpu().numpy()

    def normal_equations_dev(self, kind):
        """(n_blocks, 28) float64 on the device: the batch's own buffer, overwritten by the next evaluation."""
        return self.b.normal_equations(kind)

    @property
    def n_corr(self):
        return self.b.n_corr


class _FeatureIcp:
    """FEATURE mode (Solver::AddLidarResiduals, solver.cc:297-318): per window pair a LIDARNormalResidual block on the planar
    points and a LIDARPointResidual block on the edge points -- two batches over the same pairs, each through
    backend.icp(); their per-block normal equations add."""

    def __init__(self, backend, features, block_src, block_tgt, outlier_threshold):
        (xy_p, nrm_p, off_p), (xy_e, nrm_e, off_e) = features
        if hasattr(backend, "dedicate"):
            backend.dedicate(xy_p)
            backend.dedicate(xy_e)
        self.planar = backend.icp(xy_p, nrm_p, off_p, block_src, block_tgt, outlier_threshold)
        self.edge = backend.icp(xy_e, nrm_e, off_e, block_src, block_tgt, outlier_threshold)
        self.block_src, self.block_tgt = self.planar.block_src, self.planar.block_tgt

    def set_poses(self, poses):
        self.planar.set_poses(poses)
        self.edge.set_poses(poses)

    def search(self):
        return self.planar.search() + self.edge.search()

    def normal_equations(self, kind):
        """(kind is the all-points graph's choice: a FEATURE graph's kinds are fixed by the reference)"""
        return self.planar.normal_equations(_lib.NHIP_LIDAR_NORMAL) + self.edge.normal_equations(_lib.NHIP_LIDAR_POINT)

    def normal_equations_dev(self, kind):
        return self.planar.normal_equations_dev(_lib.NHIP_LIDAR_NORMAL) + self.edge.normal_equations_dev(_lib.NHIP_LIDAR_POINT)

    @property
    def n_corr(self):
        return self.planar.n_corr + self.edge.n_corr


class OdometryFactors:
    """Batched OdometryResidual blocks: r = (w_t (T_i + T_odom - T_j), w_r wrap(th_i + R_odom - th_j)).
    loss: None, or the loss.Loss every factor is reweighted by ("Robust loss"); evaluate() returns the
    plain r and J either way, the linear paths apply the loss."""

    def __init__(self, pose_i, pose_j, t_odom, r_odom, tw=1.0, rw=1.0, loss=None):
        self.loss = loss
        self.n = len(pose_i)
        self.pose_i = np.ascontiguousarray(pose_i, dtype=np.int32)
        self.pose_j = np.ascontiguousarray(pose_j, dtype=np.int32)
        self.t_odom = np.ascontiguousarray(np.reshape(t_odom, (-1, 2)), dtype=np.float32)
        self.r_odom = np.ascontiguousarray(r_odom, dtype=np.float32)
        self.tw, self.rw = float(tw), float(rw)

    def evaluate(self, backend, poses):
        if self.n == 0:
            return np.zeros((0, 3)), np.zeros((0, 3, 3)), np.zeros((0, 3, 3))
        return backend.odometry(self.pose_i, self.pose_j, self.t_odom, self.r_odom, self.tw, self.rw, poses)


    def normal_eq_dev(self, backend, d_poses, d_weights=None, loss=None):
        """The factors' (F, 28) rows on the device (HipBackend.odometry_normal_eq_dev)."""
        return backend.odometry_normal_eq_dev(self, d_poses, d_weights=d_weights, loss=loss)


class RelativePoseFactors:
    """Batched relative-pose factors ("Relative-pose factors"): factor f measures pose_j[f] (a closure's
    source) in the frame of pose_i[f] (its target) as z[f] = (z_x, z_y, c_z, s_z), with the information info[f] =
    (L00 L01 L02 L11 L12 L22) over (x, y, theta).  The residual is whitened by the information's Cholesky factor, so its
    squared norm is a squared Mahalanobis distance.  loss: as OdometryFactors'; evaluate() returns the plain r and J.  A factor
    whose information is not positive definite or whose measurement is not finite contributes zeros (the kernel's flags;
    hostside.relpose_rows returns them)."""

    def __init__(self, pose_i, pose_j, z, info, loss=None):
        self.loss = None if loss is None else loss.pinned()  # (cauchy's log1p as the kernel takes it: loss.log1p_pinned)
        self.n = len(pose_i)
        self.pose_i = np.ascontiguousarray(pose_i, dtype=np.int32).reshape(self.n)
        self.pose_j = np.ascontiguousarray(pose_j, dtype=np.int32).reshape(self.n)
        self.z = np.ascontiguousarray(np.reshape(z, (-1, 4)), dtype=np.float64)
        self.info = np.ascontiguousarray(np.reshape(info, (-1, 6)), dtype=np.float64)
        if len(self.z) != self.n or len(self.info) != self.n:
            raise ValueError("RelativePoseFactors: %d factors, %d measurements, %d informations" % (self.n, len(self.z), len(self.info)))
        if np.any(self.pose_i == self.pose_j):
            raise ValueError("RelativePoseFactors: a factor couples two different poses (pose_i == pose_j at %d)"
                             % int(np.nonzero(self.pose_i == self.pose_j)[0][0]))

    def evaluate(self, backend, poses):
        if self.n == 0:
            return np.zeros((0, 3)), np.zeros((0, 3, 3)), np.zeros((0, 3, 3))
        if hasattr(backend, "relative_pose"):
            return backend.relative_pose(self.z, self.info, self.pose_i, self.pose_j, poses)
        from . import hostside  # (a backend without the method: the numpy form)
        return hostside.relpose_rows(self.z, self.info, self.pose_i, self.pose_j, poses)[:3]

    def normal_eq_dev(self, backend, d_poses, d_weights=None, loss=None):
        """The factors' (F, 28) rows on the device (HipBackend.relative_pose_normal_eq_dev)."""
        return backend.relative_pose_normal_eq_dev(self, d_poses, d_weights=d_weights, loss=loss)


def relative_pose_factors(pairs_src, pairs_tgt, rel, information, weights=(10.0, 10.0), loss=None, rel_cs=None):
    """One relative-pose factor per loop closure: rel[k] = (tx, ty, theta) is where scan src sits in scan tgt's frame, rel_cs[k]
    -- if given -- its heading as (cos, sin) (a refined record's c, s; otherwise libm's of rel[k, 2]); information (F, 6), an
    all-zero row of which is filled with diag(w_t^2, w_t^2, w_r^2) of `weights`."""
    rel = np.asarray(rel, dtype=np.float64).reshape(-1, 3)
    info = np.array(information, dtype=np.float64).reshape(-1, 6)
    if len(info) != len(rel):
        raise ValueError("relative_pose_factors: %d records, %d informations" % (len(rel), len(info)))
    wt, wr = float(weights[0]), float(weights[1])
    info[~info.any(axis=1)] = (wt * wt, 0.0, 0.0, wt * wt, 0.0, wr * wr)
    if rel_cs is None:
        cs = np.array([(math.cos(t), math.sin(t)) for t in rel[:, 2]], dtype=np.float64).reshape(-1, 2)
    else:
        cs = np.asarray(rel_cs, dtype=np.float64).reshape(-1, 2)
    z = np.concatenate([rel[:, :2], cs], axis=1)
    return RelativePoseFactors(np.asarray(pairs_tgt), np.asarray(pairs_src), z, info, loss=loss)


def odometry_factors_from_poses(odom, **kw):
    """Consecutive-pose factors in the functor's convention: world-frame translation delta and heading
    delta of the odometry track (what GetSolvedOdomFactors produces from poses, solver.cc:406-427)."""
    d = np.diff(odom, axis=0)
    n = len(odom)
    return OdometryFactors(np.arange(n - 1), np.arange(1, n), d[:, :2], d[:, 2], **kw)


def loop_closure_factors(poses, pairs_src, pairs_tgt, rel, loss=None, **kw):
    """One odometry-style constraint per accepted loop closure: the matcher says where scan src sits
    in scan tgt's frame; expressed in the functor's world-frame convention around the current estimate
    of the TARGET pose: T_src - T_tgt = R(th_tgt) t_rel, th_src - th_tgt = th_rel."""
    t_odom, r_odom = [], []
    for s, t, r in zip(pairs_src, pairs_tgt, rel):
        pred = compose(poses[t], r)
        t_odom.append(pred[:2] - poses[t][:2])
        r_odom.append(r[2])
    return OdometryFactors(np.asarray(pairs_tgt), np.asarray(pairs_src), np.asarray(t_odom).reshape(-1, 2),
                           np.asarray(r_odom), loss=loss, **kw)


class HitlConstraint:
    """HitlLCConstraint (data_structures.h:41-51) + its residual blocks (AddHITLResiduals, solver.cc:515-532): the
    points GetRelevantPosesForHITL selected on line a and on line b, EVERY block a PointToLineResidual against
    line_a, all sharing one extra parameter block `chosen_line_pose` (initialised to zero)."""

    def __init__(self, line_a, line_b, a_poses, b_poses):
        self.line_a = np.ascontiguousarray(line_a, dtype=np.float32).reshape(4)
        self.line_b = np.ascontiguousarray(line_b, dtype=np.float32).reshape(4)
        self.blocks = [(int(i), np.ascontiguousarray(p, dtype=np.float32).reshape(-1, 2)) for i, p in list(a_poses) + list(b_poses)]
        self.n_a, self.n_b = len(a_poses), len(b_poses)
        self.chosen_line_pose = np.zeros(3)

    def arrays(self, line_index):
        """The input arrays of nhip_resid_point_to_line for this constraint's blocks.  The blocks never change after
        construction (like the functors' copied vectors, slam_residuals.h:214-215): built once, not per evaluation -- at
        10,000 scans they hold 1.3 M points, and a solve evaluates them dozens of times."""
        if getattr(self, "_arrays", None) is None or self._arrays[0] != line_index:
            nb = len(self.blocks)
            seg = np.tile(self.line_a, (nb, 1)).astype(np.float32)
            pts = np.concatenate([p for _, p in self.blocks]).astype(np.float32) if nb else np.zeros((0, 2), np.float32)
            pb = np.repeat(np.arange(nb, dtype=np.int32), [len(p) for _, p in self.blocks]) if nb else np.zeros(0, np.int32)
            bp = np.array([i for i, _ in self.blocks], dtype=np.int32)
            bl = np.full(nb, line_index, dtype=np.int32)
            self._arrays = (line_index, (seg, pts, pb, bp, bl))
        return self._arrays[1]


def _coo_blocks(idx, H6):
    """The (n, 6) unknowns of n blocks and their (n, 6, 6) matrices -> COO rows, columns and values, block after block."""
    return np.repeat(idx, 6, axis=1).ravel(), np.tile(idx, (1, 6)).ravel(), H6.ravel()


def _blocks_from_normal_equations(neq, idx):
    """(n, 28) rows -- upper triangle of a 6 x 6 J^T J, J^T r, r^T r -- and the (n, 6) unknowns of every block -> the COO
    rows, columns and values of the full symmetric blocks."""
    iu = np.triu_indices(6)
    H6 = np.zeros((len(neq), 6, 6))
    H6[:, iu[0], iu[1]] = neq[:, :21]
    H6 = H6 + np.transpose(H6, (0, 2, 1)) - np.einsum("bij,ij->bij", H6, np.eye(6))
    return _coo_blocks(idx, H6)


class _HostLinearStep:
    """PoseGraph.solve's linear step on the host: H and g from _assemble, scipy's spsolve over the unknowns behind pose 0."""

    def __init__(self, graph):
        self.graph, self.free = graph, np.arange(3, graph.n_unknowns)

    def evaluate(self, poses, lines, research):
        self.H, self.g, cost = self.graph._assemble(poses, lines, research)
        return cost

    def step(self, lam):
        import scipy.sparse as sp
        from scipy.sparse.linalg import spsolve
        Hf = self.H[self.free][:, self.free]
        step = np.zeros(self.graph.n_unknowns)
        with clocked("host_solver"):
            step[self.free] = spsolve(Hf + lam * sp.diags(Hf.diagonal() + 1e-9), -self.g[self.free])
        return step, None


class _DeviceLinearStep:
    """PoseGraph.solve's linear step on the device: the system assembled on the GPU, block-Jacobi PCG.  A solve that reached
    max_iters (flag 1) gives a step like any other -- the cost test accepts or rejects it; a breakdown (flag 2) is a rejected
    step, and the system on the device is still the one at the poses it was evaluated at."""

    def __init__(self, graph, cg_tol, cg_max_iters):
        self.graph, self.system, self.cg_tol, self.cg_max_iters = graph, graph._device_system(), cg_tol, cg_max_iters

    def evaluate(self, poses, lines, research):
        return self.graph._evaluate_device(self.system, poses, lines, research)

    def step(self, lam):
        with clocked("path"), clocked("path_linear"):
            step, res = self.system.solve(lam, 1e-9, self.cg_tol, self.cg_max_iters)
        self.graph._count_linear([res])
        return step, res


class PoseGraph:
    def __init__(self, xy, normals, offsets, odom, window=10, kind=_lib.NHIP_LIDAR_POINT, outlier_threshold=0.25,
                 odom_weights=(1.0, 1.0), device="cuda:0", initial=None, backend=None, features=None, odom_loss=None):
        """odom_loss: None, or the loss.Loss of the odometry chain's factors (as add_loop_closures' for the closures).
        features: None -- every point of scan i against scan j, evaluated as `kind`; or the pair of packed clouds
        ((xy_p, nrm_p, off_p), (xy_e, nrm_e, off_e)) of HipBackend.features(): the reference's FEATURE mode, planar points as
        LIDARNormalResidual blocks and edge points as LIDARPointResidual blocks (xy, normals, offsets and kind are then unused)."""
        self.n = len(odom)
        self.kind = kind
        self.backend = backend if backend is not None else HipBackend(device)
        with clocked("marshal"):
            bs, bt = window_pairs(self.n, window)
        with clocked("path"), clocked("path_setup"):  # (uploads of the clouds and block lists, device allocations: part of "path")
            if features is None:
                self.icp = self.backend.icp(xy, normals, offsets, bs, bt, outlier_threshold)
            else:
                self.icp = _FeatureIcp(self.backend, features, bs, bt, outlier_threshold)
        self.odo = odometry_factors_from_poses(odom, tw=odom_weights[0], rw=odom_weights[1], loss=odom_loss)
        self.lc = None
        self.hitl = []
        self.linear_stats = {k: 0 for k in LINEAR_STATS}  # of this graph's solve(linear_solver="device") calls
        self.covariance_stats = {"systems": 0, "iterations": [], "flags": [], "batches": []}  # of the last cross_covariances("device")
        self._device = None  # (what the system was built from, DeviceSystem): the structure is fixed once the graph is
        # odometry factors always come from `odom`; the estimate may start elsewhere (previous window pass)
        self.poses = np.array(odom if initial is None else initial, dtype=np.float64)

    def add_loop_closures(self, pairs_src, pairs_tgt, rel, weights=(10.0, 10.0), loss=None, information=None, rel_cs=None):
        """One odometry-style factor per record (loop_closure_factors), weighted `weights`.  loss: None -- every record
        enters at full weight -- or a loss.Loss: each solve reweights every record by sqrt(rho'(s)) of its own weighted
        squared residual s at the poses it evaluates, and the cost becomes Ceres' robust cost (DESIGN.md section 3,
        "Robust loss"); closure_weights() reports the weights.
        information: None -- the world-frame factor above -- or an (F, 6) array, L00 L01 L02 L11 L12 L22 over (x, y, theta) per
        record: the records become relative-pose factors ("Relative-pose factors"), which measure the source
        in the target's frame at every evaluation and weigh it by that information; an all-zero row takes
        diag(w_t^2, w_t^2, w_r^2) of `weights`.  rel_cs: with an information, the records' headings as (cos, sin) where the
        caller has them (refined records); otherwise cos and sin of rel[:, 2].  The loss' scale is then in standard deviations."""
        if information is None:
            self.lc = loop_closure_factors(self.poses, pairs_src, pairs_tgt, rel, loss=loss, tw=weights[0], rw=weights[1])
        else:
            self.lc = relative_pose_factors(pairs_src, pairs_tgt, rel, information, weights=weights, loss=loss, rel_cs=rel_cs)

    def closure_weights(self, poses=None):
        """(F, 4) float64 {s, rho, rho', sqrt(rho')} of the loop-closure factors at `poses` (default: the current estimate).
        On a backend with odometry_normal_eq_dev they are the kernel's weights output; on any other, loss.Loss' on the
        backend's residuals.  Without a loss: s, s, 1, 1."""
        from .loss import Loss
        if self.lc is None or self.lc.n == 0:
            return np.zeros((0, 4))
        poses = np.ascontiguousarray(self.poses if poses is None else poses, dtype=np.float64).reshape(-1, 3)
        loss = self.lc.loss if self.lc.loss is not None else Loss("none")
        be = self.backend
        if hasattr(be, "odometry_normal_eq_dev"):
            with clocked("path"):
                d_w = be.torch.empty((self.lc.n, 4), dtype=be.torch.float64, device=be.dev)
                self.lc.normal_eq_dev(be, be.torch.from_numpy(poses).to(be.dev), d_weights=d_w, loss=loss)
                out = d_w.cpu().numpy()
                check(be.lib.nhip_dev_status(C.c_void_p(be.torch.cuda.current_stream(be.dev).cuda_stream), None))
            return out
        with clocked("path"):
            r, _, _ = self.lc.evaluate(be, poses)
        return loss.weights(r)

    def add_hitl(self, constraint):
        """A HitlConstraint (points on the host, evaluated point by point through backend.point_to_line) or a
        hitl.DeviceHitlConstraint (points on the device, reduced there to 28 doubles per block: needs a backend with
        point_to_line_normal_eq)."""
        if hasattr(constraint, "d_points") and not hasattr(self.backend, "point_to_line_normal_eq"):
            raise TypeError("add_hitl: backend %r cannot evaluate a device constraint; pass a HitlConstraint" % self.backend.name)
        self.hitl.append(constraint)

    @property
    def n_unknowns(self):
        return 3 * self.n + 3 * len(self.hitl)

    def _assemble(self, poses, lines, research):
        """The sparse normal equations at `poses`.  Clocks: the backend calls are "path", building their input arrays
        "marshal", everything else here "assemble" (numpy: the solver's own bookkeeping)."""
        t_in, path0, marsh0 = time.perf_counter(), CLOCK["path"], CLOCK["marshal"]
        try:
            return self._assemble_inner(poses, lines, research)
        finally:
            CLOCK["assemble"] += (time.perf_counter() - t_in) - (CLOCK["path"] - path0) - (CLOCK["marshal"] - marsh0)

    def _assemble_inner(self, poses, lines, research):
        import scipy.sparse as sp
        N, NU = self.n, self.n_unknowns
        with clocked("path"):
            self.icp.set_poses(poses)
            if research:
                self.icp.search()  # correspondences are rebuilt per solve, like each window pass of the reference
            neq = self.icp.normal_equations(self.kind)
        coo = []  # (rows, columns, values) per group of blocks, in the order coo_matrix(...).tocsc() sums duplicates
        g = np.zeros(NU)
        cost = 0.5 * float(neq[:, 27].sum()) if len(neq) else 0.0
        bs, bt = self.icp.block_src, self.icp.block_tgt
        idx = np.concatenate([3 * bs[:, None] + np.arange(3), 3 * bt[:, None] + np.arange(3)], axis=1)  # (B, 6)
        coo.append(_blocks_from_normal_equations(neq, idx))
        np.add.at(g, idx.ravel(), neq[:, 21:27].ravel())
        for fac in (self.odo, self.lc):
            if fac is None or fac.n == 0:
                continue
            with clocked("path"):
                r, ji, jj = fac.evaluate(self.backend, poses)
            J = np.concatenate([ji, jj], axis=2)  # (F, 3, 6)
            rho = None
            if fac.loss is not None:  # (the reweighted factor: r~ = w r, J~ = w J, its cost rho / 2)
                r, J, rho = fac.loss.rows(r, J)
            Hf = np.einsum("fki,fkj->fij", J, J)
            gf = np.einsum("fki,fk->fi", J, r)
            idf = np.concatenate([3 * fac.pose_i[:, None] + np.arange(3), 3 * fac.pose_j[:, None] + np.arange(3)], axis=1)
            coo.append(_coo_blocks(idf, Hf))
            np.add.at(g, idf.ravel(), gf.ravel())
            cost += 0.5 * float((r * r).sum() if rho is None else rho.sum())
        for c, con in enumerate(self.hitl):
            if hasattr(con, "d_points"):
                # a DeviceHitlConstraint: 28 doubles per block from the device, over [the block's pose | chosen_line_pose c]
                if con.n_points == 0:
                    continue
                with clocked("path"):
                    neq = self.backend.point_to_line_normal_eq(con, poses, lines, c)
                idh = np.concatenate([3 * con.block_pose.astype(np.int64)[:, None] + np.arange(3),
                                      np.full((con.n_blocks, 1), 3 * N + 3 * c) + np.arange(3)], axis=1)
                coo.append(_blocks_from_normal_equations(neq, idh))
                np.add.at(g, idh.ravel(), neq[:, 21:27].ravel())
                cost += 0.5 * float(neq[:, 27].sum())
                continue
            with clocked("marshal"):
                seg, pts, pb, bp, bl = con.arrays(c)
            if len(pts) == 0:
                continue
            with clocked("path"):
                r, j0, j1 = self.backend.point_to_line(seg, pts, pb, bp, bl, poses, lines)
            J = np.concatenate([j0, j1], axis=1)  # (n, 6): d/d pose of the point's node, d/d chosen_line_pose
            ids = np.concatenate([3 * bp[pb][:, None] + np.arange(3), np.full((len(pts), 1), 3 * N + 3 * c) + np.arange(3)], axis=1)
            coo.append(_coo_blocks(ids, np.einsum("ni,nj->nij", J, J)))
            np.add.at(g, ids.ravel(), (J * r[:, None]).ravel())
            cost += 0.5 * float((r * r).sum())
        rows, cols, vals = (np.concatenate(part) for part in zip(*coo))
        H = sp.coo_matrix((vals, (rows, cols)), shape=(NU, NU)).tocsc()
        return H, g, cost

    def _lines(self):
        return np.array([c.chosen_line_pose for c in self.hitl], dtype=np.float64).reshape(-1, 3)

    def cross_covariances(self, pairs, linear_solver="host", dtype=np.float32, cg_tol=1e-10):
        """Covariance blocks the way LCMatcher asks Ceres for them (GetCovarianceMatrix,
        lc_matcher.cc:28-46): the (source pose, target pose) cross block of (J^T J)^-1 of the current
        problem with the pose just before the earlier of the two held constant instead of pose 0;
        returns the top-left 2 x 2 (translation) of each 3 x 3 block, float32 like the reference
        (dtype=np.float64: the blocks before that cast).
        With a robust loss on the odometry or loop-closure factors, J is the reweighted J~ = sqrt(rho') J at the current
        estimate, as ceres::Covariance sees it: both linear solvers go through _assemble / _evaluate_device.
        linear_solver "host": J^T J comes from the backend's per-block normal equations; the sparse solves are host
        work, one factorisation per gauge.  "device": the system is evaluated and assembled on the GPU as for
        solve(linear_solver="device") (the same backend and constraints are needed: TypeError otherwise) and the wanted
        columns of all the gauged inverses come from ONE batched block-Jacobi PCG to ||r|| <= cg_tol ||b||
        (linsolve.DeviceSystem.inverse_columns); four doubles per pair come down.  .linear_stats counts its systems,
        .covariance_stats describes the last such call."""
        dtype = np.dtype(dtype)
        if dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError("cross_covariances: dtype %r (np.float32 or np.float64)" % (dtype,))
        if linear_solver == "device":
            return self._cross_covariances_device(pairs, cg_tol).astype(dtype)
        if linear_solver != "host":
            raise ValueError("cross_covariances: linear_solver %r (\"host\" or \"device\")" % (linear_solver,))
        import scipy.sparse as sp
        from scipy.sparse.linalg import splu
        H, _, _ = self._assemble(self.poses, self._lines(), research=False)
        H = H.tocsc()[:3 * self.n][:, :3 * self.n]
        out = np.zeros((len(pairs), 2, 2), dtype=np.float64)
        by_gauge = {}
        for k, (s_, t_) in enumerate(pairs):
            by_gauge.setdefault(max(min(int(s_), int(t_)) - 1, 0), []).append(k)
        for gauge, ks in by_gauge.items():
            free = np.concatenate([np.arange(0, 3 * gauge), np.arange(3 * gauge + 3, 3 * self.n)])
            pos = -np.ones(3 * self.n, dtype=np.int64)
            pos[free] = np.arange(len(free))
            lu = splu(H[free][:, free].tocsc() + 1e-12 * sp.identity(len(free), format="csc"))
            for k in ks:
                s_, t_ = int(pairs[k][0]), int(pairs[k][1])
                if s_ == gauge or t_ == gauge:
                    continue  # a constant block has no covariance
                rhs = np.zeros((len(free), 2))
                rhs[pos[3 * t_], 0] = 1.0
                rhs[pos[3 * t_ + 1], 1] = 1.0
                x = lu.solve(rhs)
                out[k] = x[[pos[3 * s_], pos[3 * s_ + 1]], :]
        return out.astype(dtype)

    def _cross_covariances_device(self, pairs, cg_tol):
        """cross_covariances' blocks in float64 from the device: two systems per distinct (gauge, target) -- the columns
        3 t and 3 t + 1 of the inverse gauged there -- solved in one batch; pose 0 is free for this call, the HITL line
        blocks are held constant (the host path's cut to the first 3 N unknowns); the mask is put back afterwards."""
        system = self._device_system()
        N, torch = self.n, self.backend.torch
        index, gauge, rhs, take = {}, [], [], []  # (gauge, target) -> its first system; per pair with a block: (k, s, system)
        for k, (s_, t_) in enumerate(pairs):
            s_, t_ = int(s_), int(t_)
            if not (0 <= s_ < N and 0 <= t_ < N):
                raise ValueError("cross_covariances: pair (%d, %d) outside the %d poses" % (s_, t_, N))
            g = max(min(s_, t_) - 1, 0)
            if s_ == g or t_ == g:
                continue  # a constant block has no covariance
            if (g, t_) not in index:
                index[(g, t_)] = len(gauge)
                gauge += [g, g]
                rhs += [3 * t_, 3 * t_ + 1]
            take.append((k, s_, index[(g, t_)]))
        out = np.zeros((len(pairs), 2, 2), dtype=np.float64)
        self.covariance_stats = {"systems": len(gauge), "iterations": [], "flags": [], "batches": []}
        if not take:
            return out
        held = system.fixed
        system.set_fixed(range(N, N + len(self.hitl)))
        try:
            self._evaluate_device(system, self.poses, self._lines(), research=False)
            with clocked("path"), clocked("path_linear"):
                x, results = system.inverse_columns(gauge, rhs, tol=cg_tol)
                rows = torch.tensor([[3 * s_, 3 * s_, 3 * s_ + 1, 3 * s_ + 1] for _, s_, _ in take], device=x.device)
                cols = torch.tensor([[c, c + 1, c, c + 1] for _, _, c in take], device=x.device)
                blocks = x[rows, cols].cpu().numpy()
        finally:
            system.set_fixed(held)
        out[[k for k, _, _ in take]] = blocks.reshape(-1, 2, 2)
        self.covariance_stats["iterations"] = [r.iterations for r in results]
        self.covariance_stats["flags"] = [r.flag for r in results]
        self.covariance_stats["batches"] = list(system.column_batches)  # (systems, iterations of the slowest, seconds) per call
        self._count_linear(results)
        return out

    def _count_linear(self, results):  # the PcgResults of device solves into .linear_stats and LINEAR_STATS
        for stats in (self.linear_stats, LINEAR_STATS):
            stats["solves"] += len(results)
            stats["iterations"] += sum(r.iterations for r in results)
            stats["not_converged"] += sum(r.flag == 1 for r in results)
            stats["breakdowns"] += sum(r.flag == 2 for r in results)

    def _device_system(self):
        """The block-sparse system of this graph on the device, built on the first solve(linear_solver="device") and again
        only if loop closures or HITL constraints were added since.  Unknown blocks: the N poses, then one per HITL
        constraint.  Rows, in the order _evaluate_device joins them: ICP blocks [source | target], odometry factors
        [pose_i | pose_j], loop closures likewise, then each device HITL constraint's blocks [pose | chosen_line_pose c]."""
        if not hasattr(self.backend, "device_system") or not hasattr(self.icp, "normal_equations_dev"):
            raise TypeError("solve: backend %r has no device linear solver; use linear_solver=\"host\"" % self.backend.name)
        for con in self.hitl:
            if not hasattr(con, "d_points"):
                raise TypeError("solve: linear_solver=\"device\" takes device HITL constraints (hitl.select), not a HitlConstraint")
        built_from = (id(self.lc), tuple(id(c) for c in self.hitl))
        if self._device is not None and self._device[0] == built_from:
            return self._device[1]
        from . import linsolve
        with clocked("path"), clocked("path_linear"):
            u, v = [self.icp.block_src], [self.icp.block_tgt]
            for fac in (self.odo, self.lc):
                if fac is not None:
                    u.append(fac.pose_i)
                    v.append(fac.pose_j)
            for c, con in enumerate(self.hitl):
                u.append(con.block_pose)
                v.append(np.full(con.n_blocks, self.n + c))
            structure = linsolve.BlockStructure(self.n + len(self.hitl), np.concatenate(u), np.concatenate(v))
            system = self.backend.device_system(structure, fixed=[0])  # pose 0 constant
        self._device = (built_from, system)
        return system

    def _evaluate_device(self, system, poses, lines, research):
        """The system at `poses`, assembled on the device from rows that never leave it: the poses go up, the cost comes down."""
        torch, be = self.backend.torch, self.backend
        with clocked("path"):
            self.icp.set_poses(poses)
            if research:
                self.icp.search()
            d_poses = torch.from_numpy(np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)).to(be.dev)
            d_lines = torch.from_numpy(np.ascontiguousarray(lines, dtype=np.float64).reshape(-1, 3)).to(be.dev)
            parts = [self.icp.normal_equations_dev(self.kind)]
            parts += [fac.normal_eq_dev(be, d_poses) for fac in (self.odo, self.lc) if fac is not None]
            parts += [be.point_to_line_normal_eq_dev(con, d_poses, d_lines, c) for c, con in enumerate(self.hitl)]
            rows = torch.cat(parts)
            with clocked("path_linear"):
                return system.assemble(rows)

    def solve(self, iterations=8, damping=1e-3, verbose=False, linear_solver="host", cg_tol=1e-10, cg_max_iters=None):
        """Gauss-Newton with Levenberg damping; pose 0 constant (SetParameterBlockConstant, solver.cc:384-386).
        linear_solver "host": the system assembled in numpy from downloaded rows, scipy's spsolve.  "device": assembled on
        the GPU and solved there by block-Jacobi PCG to ||r|| <= cg_tol ||b|| in at most cg_max_iters iterations (None:
        max(200, 3 x the unknown blocks)); needs a backend with device_system and device HITL constraints (TypeError
        otherwise); .linear_stats counts the solves."""
        if linear_solver not in ("host", "device"):
            raise ValueError("solve: linear_solver %r (\"host\" or \"device\")" % (linear_solver,))
        linear = _DeviceLinearStep(self, cg_tol, cg_max_iters) if linear_solver == "device" else _HostLinearStep(self)
        poses, lines = self.poses.copy(), self._lines()
        cost = linear.evaluate(poses, lines, research=True)
        history, lam, N = [cost], damping, self.n
        for it in range(iterations):
            step, res = linear.step(lam)  # (res: the device's PcgResult, None on the host)
            broke = res is not None and res.flag == 2
            accepted = False
            if not broke:
                trial, trial_lines = poses + step[:3 * N].reshape(-1, 3), lines + step[3 * N:].reshape(-1, 3)
                cost2 = linear.evaluate(trial, trial_lines, research=False)
                accepted = cost2 < cost
            if accepted:
                poses, lines, cost, lam = trial, trial_lines, cost2, max(lam * 0.3, 1e-9)
            else:
                lam *= 10.0
                if not broke:  # (the system is the trial's: back to the one at `poses`)
                    cost = linear.evaluate(poses, lines, research=False)
            history.append(cost)
            if verbose:
                print("iter %d cost %.6g lambda %.2g" % (it, cost, lam) + ("" if res is None else " pcg %r" % (res,)))
        self.poses = poses
        for c, con in enumerate(self.hitl):
            con.chosen_line_pose = lines[c].copy()
        return poses, history


def solve_growing_window(xy, normals, offsets, odom, window_min=1, window_max=10, iterations=4,
                         kind=_lib.NHIP_LIDAR_POINT, outlier_threshold=0.25, odom_weights=(1.0, 1.0),
                         device="cuda:0", verbose=False, backend=None, initial=None, hitl=(), loop_closures=None, features=None,
                         linear_solver="host", lc_loss=None):
    """Solver::OptimizeOverGrowingWindow (solver.cc:339-355): for every window size from
    lidar_constraint_amount_min to _max the problem is rebuilt -- odometry factors, HITL residuals
    (AddHITLResiduals) plus fresh correspondences for all (i, j) blocks of the window, searched at the current
    estimate -- and solved.  features: as PoseGraph's (FEATURE mode); linear_solver: as PoseGraph.solve's; lc_loss: the loss.Loss
    add_loop_closures gets in every pass (None: none); loop_closures: (src, tgt, rel) or (src, tgt, rel, kw), kw the further keywords
    of add_loop_closures (information=, rel_cs=, weights=).  Returns (PoseGraph of the last pass, poses)."""
    poses = np.array(odom if initial is None else initial, dtype=np.float64)
    backend = backend if backend is not None else HipBackend(device)
    if features is None and hasattr(backend, "reserve_icp"):  # (feature clouds: a few points per scan, nothing to reserve)
        with clocked("path"), clocked("path_setup"):
            backend.reserve_icp(offsets, window_max)
    pg = None
    for w in range(window_min, window_max + 1):
        pg = PoseGraph(xy, normals, offsets, odom, window=w, kind=kind, outlier_threshold=outlier_threshold,
                       odom_weights=odom_weights, device=device, initial=poses, backend=backend, features=features)
        for con in hitl:
            pg.add_hitl(con)
        if loop_closures is not None:
            pg.add_loop_closures(*loop_closures[:3], loss=lc_loss, **(loop_closures[3] if len(loop_closures) > 3 else {}))
        poses, hist = pg.solve(iterations=iterations, verbose=verbose, linear_solver=linear_solver)
        if verbose:
            print("window %d: cost %.6g -> %.6g" % (w, hist[0], hist[-1]))
    return pg, poses


def trajectory_error(poses, truth):
    """RMS translation error after aligning the first pose (both tracks start from the same anchor)."""
    def rel(p):
        c, s = math.cos(-p[0, 2]), math.sin(-p[0, 2])
        d = p[:, :2] - p[0, :2]
        return np.stack([c * d[:, 0] - s * d[:, 1], s * d[:, 0] + c * d[:, 1]], 1)
    return float(np.sqrt(np.mean(np.sum((rel(poses) - rel(truth)) ** 2, axis=1))))
