"""Loop-closure consistency on the GPU (K17, nhip_consistency.hip) against the numpy restatement (tests/consistency_reference.py),
through the entry points on device buffers and through the host-memory form: the matrix's words, the degrees, the members, their
count and the stats byte for byte, on every scene of the CPU test -- word, workgroup and tile seams, ties, cliques, tolerance edges
one ulp either side, poses 10 km out, NaN and inf records, the step cap -- with nhip_dev_status clean; the batching of the steps
is invisible; a short workspace and stale degrees cost an error code."""
import ctypes as C

import numpy as np
import pytest

from tests import consistency_reference as R
from nautilus_amd import _lib, consistency

pytestmark = pytest.mark.gpu

SCENES = sorted(R.scenes())


def status_clean():
    info = (C.c_int32 * 4)()
    rc = _lib.load().nhip_dev_status(None, info)
    return rc == _lib.NHIP_OK, list(info)


def on_device(torch, rec, sp, check_every=8):
    d_rec = torch.from_numpy(np.ascontiguousarray(rec)).to("cuda:0") if len(rec) else torch.zeros((1, 8), dtype=torch.float64, device="cuda:0")
    d_adj, d_deg, d_astats, ws = consistency.adjacency_on_device(d_rec, len(rec), sp)
    d_mem, d_n, d_stats = consistency.set_on_device(d_adj, d_deg, len(rec), ws, sp, check_every=check_every)
    torch.cuda.synchronize()
    return (d_adj.cpu().numpy().view(np.uint64), d_deg.cpu().numpy(), d_astats.cpu().numpy(), d_mem.cpu().numpy(), int(d_n.cpu()[0]),
            d_stats.cpu().numpy())


@pytest.mark.parametrize("name", SCENES)
def test_device_equals_the_restatement(gpu, name):
    import torch
    rec, sp, want = R.scene_results()[name]
    assert status_clean()[0]
    adj, deg, astats, members, n, stats = on_device(torch, rec, sp)
    assert adj.shape == want["adj"].shape and adj.tobytes() == want["adj"].tobytes()
    assert deg.dtype == np.int32 and deg.tobytes() == want["deg"].tobytes()
    assert astats.tobytes() == want["adj_stats"].tobytes()
    assert members.dtype == np.int32 and members.tobytes() == want["members"].tobytes()
    assert n == want["n_members"] and stats.tobytes() == want["stats"].tobytes()
    ok, info = status_clean()
    assert ok, info
    # the host-memory form
    members, n, stats = consistency.consistent_set(rec, sp)
    assert members.tobytes() == want["members"].tobytes() and n == want["n_members"] and stats.tobytes() == want["stats"].tobytes()
    ok, info = status_clean()
    assert ok, info


@pytest.mark.parametrize("name", ["loop_257", "identical_130", "capped_130"])
def test_the_batching_is_invisible(gpu, name):
    import torch
    rec, sp, want = R.scene_results()[name]
    assert want["n_members"] > 64  # (more steps than the longest batch)
    for every in (1, 8, 64, 0):
        _, _, _, members, n, stats = on_device(torch, rec, sp, check_every=every)
        assert members.tobytes() == want["members"].tobytes() and n == want["n_members"] and stats.tobytes() == want["stats"].tobytes(), every
    assert status_clean()[0]


def test_short_workspace_and_stale_degrees_cost_an_error_code(gpu):
    import torch
    rec, sp, want = R.scene_results()["loop_129"]
    M = len(rec)
    d_rec = torch.from_numpy(rec).to("cuda:0")
    d_adj, d_deg, _, ws = consistency.adjacency_on_device(d_rec, M, sp)
    with pytest.raises(_lib.NhipError) as e:
        consistency.set_on_device(d_adj, d_deg, M, ws, sp, workspace_bytes_given=consistency.workspace_bytes(M) - 1)
    assert e.value.code == _lib.NHIP_ERR_ARG and "workspace" in str(e.value)
    with pytest.raises(_lib.NhipError):
        consistency.set_on_device(d_adj, d_deg, M, ws, sp, check_every=-1)
    # a degree outside [0, M) counts as 0: reported, never followed anywhere
    v0 = int(want["members"][0])
    d_deg[v0] = M + 7
    d_deg[3] = -1
    members, n, stats = consistency.set_on_device(d_adj, d_deg, M, ws, sp)
    torch.cuda.synchronize()
    ok, info = status_clean()
    assert not ok and info[0] == 131072 and info[1] == 131072 and info[2] in (M + 7, -1) and info[3] in (v0, 3)
    assert status_clean()[0]  # (the record was consumed)
    n = int(n.cpu()[0])
    members = members.cpu().numpy()
    assert 0 < n <= M and members[0] != v0 and len(set(members[:n].tolist())) == n and (members[n:] == -1).all()
    A = R.adjacency_bool(rec, sp)
    assert all(A[a, b] for a in members[:n] for b in members[:n] if a != b)  # (still a clique of the matrix)
