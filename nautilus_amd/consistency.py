"""Loop-closure consistency on the GPU: the records of loop closure judged against each other.  Two records are consistent if the
cycle they form with the odometry between their ends closes up to the drift that odometry can have gathered (pairwise
consistency maximisation: Mangelson et al., ICRA 2018); all M^2 / 2 cycle checks make a bit matrix, and a large set of mutually
consistent records is grown greedily on it.  One wrong record -- two corridors that look alike, score well and contradict no
free space -- bends a whole trajectory when it enters PoseGraph.add_loop_closures at full weight (a robust loss, loss.py, is
that call's option and the last line of defence behind this filter).

Build-defined (nhip_consistency_adjacency_dev / nhip_consistency_set_dev / nhip_consistency, kernel unit K17), in the place of the
reference's human curation.  The spec -- fp64 + - x and comparisons in a fixed order, integers after them, so a numpy restatement
pins it bit for bit -- is DESIGN.md section 3, "Loop-closure consistency".  Torch tensors are only the allocator, as in place.py.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import NHIP_CONSISTENCY_STATE_BYTES, ConsistencySpec, check, ptr

RECORD_FIELDS = ("cw", "sw", "xw", "yw", "px", "py", "la", "lb")
STATS_FIELDS = ("M", "edges", "max_degree", "steps", "step_cap_hit", "reserved0", "reserved1", "reserved2")
MAX_RECORDS = 65536


def prepare(poses, src, tgt, rel):
    """The prepared records, (M, 8) float64 = RECORD_FIELDS, of M loop closures (src, tgt, rel) under the trajectory `poses`
    ((n_scans, 3): the estimate the pairs were proposed under; it stands in for odometry).  rel is (tx, ty, theta) of scan src
    in scan tgt's frame (SynthBag.true_relative, PoseGraph.add_loop_closures).  float64 numpy, every product and sum rounded on
    its own in the order of DESIGN.md section 3; the one function behind the device path, the host path and the reference."""
    P = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    src, tgt = np.asarray(src, dtype=np.int64).reshape(-1), np.asarray(tgt, dtype=np.int64).reshape(-1)
    Z = np.asarray(rel, dtype=np.float64).reshape(-1, 3)
    if not len(src) == len(tgt) == len(Z):
        raise ValueError("consistency.prepare: %d src, %d tgt, %d rel" % (len(src), len(tgt), len(Z)))
    if len(src) and (min(src.min(), tgt.min()) < 0 or max(src.max(), tgt.max()) >= len(P)):
        raise ValueError("consistency.prepare: a scan id outside the %d poses" % len(P))
    step = np.hypot(np.diff(P[:, 0]), np.diff(P[:, 1]))
    arc = np.concatenate([[0.0], np.cumsum(step)]) if len(P) else np.zeros(0)
    xs, ys, cs, ss = P[src, 0], P[src, 1], np.cos(P[src, 2]), np.sin(P[src, 2])
    xt, yt, ct, st = P[tgt, 0], P[tgt, 1], np.cos(P[tgt, 2]), np.sin(P[tgt, 2])
    cz, sz = np.cos(Z[:, 2]), np.sin(Z[:, 2])
    # A = X_tgt o Z
    ca, sa = (ct * cz) - (st * sz), (st * cz) + (ct * sz)
    xa, ya = ((ct * Z[:, 0]) - (st * Z[:, 1])) + xt, ((st * Z[:, 0]) + (ct * Z[:, 1])) + yt
    # X_src^-1
    ix, iy = -((cs * xs) + (ss * ys)), (ss * xs) - (cs * ys)
    # W = A o X_src^-1
    cw, sw = (ca * cs) + (sa * ss), (sa * cs) - (ca * ss)
    xw, yw = ((ca * ix) - (sa * iy)) + xa, ((sa * ix) + (ca * iy)) + ya
    return np.ascontiguousarray(np.stack([cw, sw, xw, yw, xt, yt, arc[src], arc[tgt]], axis=1))


def default_spec():
    """nhip_consistency_spec_default (works without a device)."""
    s = ConsistencySpec()
    check(_lib.load().nhip_consistency_spec_default(C.byref(s)))
    return s


def spec(**overrides):
    """The defaults with the named fields replaced."""
    s = default_spec()
    for k, v in overrides.items():
        if k not in dict(ConsistencySpec._fields_):
            raise TypeError("consistency.spec: no field %r" % k)
        setattr(s, k, v)
    return s


def workspace_bytes(M):
    """nhip_consistency_workspace_bytes (works without a device): the one buffer of the set's state, the matrix and the degrees."""
    n = _lib.load().nhip_consistency_workspace_bytes(int(M))
    if n < 0:
        check(_lib.NHIP_ERR_ARG)
    return n


def words(M):
    return (int(M) + 63) // 64


def _records(records):
    rec = np.ascontiguousarray(records, dtype=np.float64)
    if rec.ndim != 2 or rec.shape[1] != 8:
        raise ValueError("consistency: records of shape %s, (M, 8) wanted (consistency.prepare makes them)" % (rec.shape,))
    return rec


def adjacency_on_device(d_records, M, spec=None, workspace=None):
    """nhip_consistency_adjacency_dev on a device tensor of prepared records (float64 (M, 8)): (adjacency int64 (M, W) -- the
    uint64 words, bit for bit --, degrees int32 (M,), stats int64 (8,), workspace), on torch's current stream.  The matrix and
    the degrees are views into the workspace, the one buffer of workspace_bytes(M) that set_on_device takes (None: allocated
    here)."""
    import torch
    lib, dev, M = _lib.load(), d_records.device, int(M)
    spec = default_spec() if spec is None else spec
    ws = workspace_bytes(M)
    if workspace is None:
        workspace = torch.empty(ws // 8, dtype=torch.int64, device=dev)
    if workspace.dtype != torch.int64 or workspace.numel() * 8 < ws:
        raise ValueError("consistency.adjacency_on_device: the workspace is an int64 tensor of >= %d bytes" % ws)
    W, at = words(M), NHIP_CONSISTENCY_STATE_BYTES // 8
    d_adj = workspace[at:at + M * W].view(M, W)
    d_deg = workspace[at + M * W:at + M * W + (M + 1) // 2].view(torch.int32)[:M]
    d_stats = torch.empty(8, dtype=torch.int64, device=dev)
    sp = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    check(lib.nhip_consistency_adjacency_dev(d_records.data_ptr(), M, C.byref(spec), d_adj.data_ptr(), d_deg.data_ptr(),
                                             d_stats.data_ptr(), sp))
    return d_adj, d_deg, d_stats, workspace


def set_on_device(d_adj, d_deg, M, workspace, spec=None, check_every=8, workspace_bytes_given=None):
    """nhip_consistency_set_dev on the matrix and degrees of adjacency_on_device and its workspace: (members int32 (M,) in pick
    order, -1 behind them; n_members int32 (1,); stats int64 (8,)), on torch's current stream; the call waits for it.
    check_every: steps enqueued between two looks at the done word (it changes no result).  workspace_bytes_given: what the call
    is told the workspace holds (None: its size).  nhip_dev_status is the caller's to check."""
    import torch
    lib, dev, M = _lib.load(), workspace.device, int(M)
    spec = default_spec() if spec is None else spec
    d_members = torch.empty(max(M, 1), dtype=torch.int32, device=dev)
    d_n = torch.empty(1, dtype=torch.int32, device=dev)
    d_stats = torch.empty(8, dtype=torch.int64, device=dev)
    given = workspace.numel() * workspace.element_size() if workspace_bytes_given is None else int(workspace_bytes_given)
    sp = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    check(lib.nhip_consistency_set_dev(d_adj.data_ptr(), d_deg.data_ptr(), M, C.byref(spec), int(check_every), d_members.data_ptr(),
                                       d_n.data_ptr(), d_stats.data_ptr(), workspace.data_ptr(), given, sp))
    return d_members[:M], d_n, d_stats


def consistent_set(records, spec=None):
    """The host-memory form (nhip_consistency) on prepared records (M, 8): (members int32 (M,) in pick order, -1 behind them;
    n_members; stats int64 (8,): STATS_FIELDS)."""
    spec = default_spec() if spec is None else spec
    rec = _records(records)
    members = np.full(len(rec), -1, dtype=np.int32)
    n, stats = np.zeros(1, dtype=np.int32), np.zeros(8, dtype=np.int64)
    check(_lib.load().nhip_consistency(ptr(rec), len(rec), C.byref(spec), ptr(members), ptr(n), ptr(stats)))
    return members, int(n[0]), stats


def keep(members, n_members, M, min_set=3):
    """The boolean mask (M,) of the records in the set; all False if the set has fewer than min_set members: whether a small
    set is trusted is the caller's decision."""
    mask = np.zeros(int(M), dtype=bool)
    if int(n_members) >= int(min_set):
        mask[np.asarray(members, dtype=np.int64)[:int(n_members)]] = True
    return mask
