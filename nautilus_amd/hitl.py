"""A human-in-the-loop constraint that stays on the GPU: the point selection and the packed point-to-line blocks.

  Solver::GetRelevantPosesForHITL            src/optimization/solver.cc:479-513
    -> nhip_hitl_select_dev   (class of every point, counts and membership of every scan, block ids and offsets, totals)
    -> nhip_hitl_pack_dev     (the selected points as contiguous blocks: all a-nodes in node order, then all b-nodes)
  Solver::AddHITLResiduals                   solver.cc:515-532
    -> nhip_resid_point_to_line_normal_eq_dev on the packed blocks (HipBackend.point_to_line_normal_eq): 28 doubles per block
The spec is DESIGN.md section 8, "HITL on the device".  hostside.hitl_relevant_poses is the numpy statement of the same
selection (with an np.float64 line width: the reference's comparison).  Torch tensors are only the allocator.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import HitlSpec, check


def default_spec():
    """hitl_line_width 0.05, hitl_pose_point_threshold 10, both lines zero (nhip_hitl_spec_default; works without a device)."""
    s = HitlSpec()
    check(_lib.load().nhip_hitl_spec_default(C.byref(s)))
    return s


def hitl_spec(line_a, line_b, line_width=0.05, point_threshold=10):
    s = default_spec()
    s.line_a[:] = [float(v) for v in np.asarray(line_a, dtype=np.float32).reshape(4)]
    s.line_b[:] = [float(v) for v in np.asarray(line_b, dtype=np.float32).reshape(4)]
    s.line_width, s.point_threshold = float(line_width), int(point_threshold)
    return s


def pose_floats(poses):
    """(n, 4) float32 (cos, sin, x, y): the entries of PoseArrayToAffine(pose).cast<float>(), formed as
    hostside.hitl_relevant_poses forms them (cosine and sine in double, then rounded)."""
    P = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    return np.ascontiguousarray(np.stack([np.float32(np.cos(P[:, 2])), np.float32(np.sin(P[:, 2])), np.float32(P[:, 0]),
                                          np.float32(P[:, 1])], axis=1), dtype=np.float32)


class DeviceHitlConstraint:
    """HitlLCConstraint (data_structures.h:41-51) with its points on the device: d_points (n_points, 2) float32 in block order,
    d_block_offsets (n_blocks + 1), d_block_pose (n_blocks), d_segments (n_blocks, 4): line a for EVERY block (AddHITLResiduals,
    solver.cc:515-532).  Host copies block_pose and block_offsets; n_a, n_b, n_points; chosen_line_pose as HitlConstraint's."""

    def __init__(self, line_a, line_b, d_points, d_block_offsets, d_block_pose, block_pose, block_offsets, n_a, n_b, n_points):
        import torch
        self.line_a = np.ascontiguousarray(line_a, dtype=np.float32).reshape(4)
        self.line_b = np.ascontiguousarray(line_b, dtype=np.float32).reshape(4)
        self.d_points, self.d_block_offsets, self.d_block_pose = d_points, d_block_offsets, d_block_pose
        self.block_pose, self.block_offsets = block_pose, block_offsets
        self.n_a, self.n_b, self.n_points = int(n_a), int(n_b), int(n_points)
        self.n_blocks = self.n_a + self.n_b
        self.d_segments = torch.from_numpy(np.tile(self.line_a, (max(self.n_blocks, 1), 1))).to(d_points.device)
        self._d_line = None  # (line index, d_block_line)
        self.chosen_line_pose = np.zeros(3)

    def d_block_line(self, line_index):
        import torch
        if self._d_line is None or self._d_line[0] != line_index:
            self._d_line = (line_index, torch.full((max(self.n_blocks, 1),), int(line_index), dtype=torch.int32,
                                                   device=self.d_points.device))
        return self._d_line[1]

    def to_host(self):
        """(a_poses, b_poses) as hostside.hitl_relevant_poses returns them: lists of (node index, points (k, 2) float32)."""
        pts = self.d_points[:self.n_points].cpu().numpy().reshape(-1, 2)
        blocks = [(int(self.block_pose[b]), pts[self.block_offsets[b]:self.block_offsets[b + 1]].copy()) for b in range(self.n_blocks)]
        return blocks[:self.n_a], blocks[self.n_a:]


def select(backend, xy, offsets, poses, line_a, line_b, line_width=0.05, point_threshold=10):
    """GetRelevantPosesForHITL on the GPU for the scans (xy, offsets) at `poses` -> DeviceHitlConstraint.  The clouds are the
    backend arena's device copy when it holds one of this `xy` (the ICP batches' upload); otherwise they are uploaded once.
    One small download between the two calls: the totals that size the packed arrays."""
    import torch
    lib, dev = _lib.load(), backend.dev
    spec = hitl_spec(line_a, line_b, line_width, point_threshold)
    held = getattr(getattr(backend, "arena", None), "clouds", None)
    if held is not None and held[4][0] is xy and held[4][2] is offsets:
        d_xy, d_off = held[1], held[3]
        n_scans, n_pts = len(offsets) - 1, int(np.asarray(offsets)[-1])
    else:
        off = np.ascontiguousarray(offsets, dtype=np.int32)
        pts = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
        if not pts.flags.writeable:
            pts = pts.copy()  # (torch.from_numpy wants a writable array)
        n_scans, n_pts = len(off) - 1, int(off[-1])
        if len(pts) != n_pts:
            raise ValueError("hitl.select: offsets[-1] = %d, but %d points" % (n_pts, len(pts)))
        d_xy = torch.from_numpy(pts).to(dev) if n_pts else torch.zeros(2, dtype=torch.float32, device=dev)
        d_off = torch.from_numpy(off).to(dev)
    aff = pose_floats(poses)
    if len(aff) != n_scans:
        raise ValueError("hitl.select: %d poses for %d scans" % (len(aff), n_scans))
    e = lambda n, dt: torch.empty(max(int(n), 1), dtype=dt, device=dev)
    d_aff = torch.from_numpy(aff).to(dev) if n_scans else e(4, torch.float32)
    d_cls, d_cnt, d_blk, d_so, d_tot = e(n_pts, torch.uint8), e(2 * n_scans, torch.int32), e(n_scans, torch.int32), \
        e(n_scans, torch.int32), e(3, torch.int32)
    sp = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    check(lib.nhip_hitl_select_dev(d_xy.data_ptr(), d_off.data_ptr(), n_scans, d_aff.data_ptr(), C.byref(spec), d_cls.data_ptr(),
                                   d_cnt.data_ptr(), d_blk.data_ptr(), d_so.data_ptr(), d_tot.data_ptr(), sp))
    n_a, n_b, n_points = (int(v) for v in d_tot.cpu().numpy()[:3])
    nb = n_a + n_b
    d_pts, d_boff, d_bpose = e(2 * n_points, torch.float32), e(nb + 1, torch.int32), e(nb, torch.int32)
    check(lib.nhip_hitl_pack_dev(d_xy.data_ptr(), d_off.data_ptr(), n_scans, d_cls.data_ptr(), d_cnt.data_ptr(), d_blk.data_ptr(),
                                 d_so.data_ptr(), d_tot.data_ptr(), nb, n_points, d_pts.data_ptr(), d_boff.data_ptr(), d_bpose.data_ptr(), sp))
    check(lib.nhip_dev_status(sp, None))
    return DeviceHitlConstraint(line_a, line_b, d_pts[:2 * n_points].view(n_points, 2), d_boff[:nb + 1], d_bpose[:nb],
                                d_bpose[:nb].cpu().numpy(), d_boff[:nb + 1].cpu().numpy(), n_a, n_b, n_points)
