"""Loop-closure consistency without a device ("Loop-closure consistency"): the numpy host path
(hostside.consistent_set: product code) equals the restatement written from the DESIGN text (tests/consistency_reference.py) byte
for byte on every scene of the GPU test; consistency.prepare against 3 x 3 matrices; the spec's defaults, the workspace rule and
the rejection of bad specs; and the conditions the defaults were chosen under, on the fixture of the study."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import consistency_reference as R
from nautilus_amd import _lib, consistency, hostside

SCENES = sorted(R.scenes())


@pytest.mark.parametrize("name", SCENES)
def test_host_path_equals_the_restatement(name):
    rec, sp, want = R.scene_results()[name]
    members, n, stats, adj, deg = hostside.consistent_set(rec, sp, adjacency=True)
    assert adj.dtype == np.uint64 and adj.shape == want["adj"].shape and adj.tobytes() == want["adj"].tobytes()
    assert deg.dtype == np.int32 and deg.tobytes() == want["deg"].tobytes()
    assert members.dtype == np.int32 and members.tobytes() == want["members"].tobytes()
    assert n == want["n_members"] and stats.tobytes() == want["stats"].tobytes()
    assert hostside.consistent_set(rec, sp)[0].tobytes() == members.tobytes()


def test_the_scenes_are_what_their_names_say():
    res = R.scene_results()
    assert res["loop_0"][2]["n_members"] == 0 and res["loop_0"][2]["adj"].shape == (0, 0)
    assert res["edge_free_70"][2]["members"][:2].tolist() == [0, -1] and res["edge_free_70"][2]["stats"][1] == 0
    for M in (65, 130):  # every tie goes to the smaller index
        assert res["identical_%d" % M][2]["members"].tolist() == list(range(M))
    two = res["two_cliques_66"][2]
    assert two["n_members"] == 33 and two["members"][0] == 0 and (two["deg"] == 32).all()
    pend = res["pendant_11"][2]  # the hub has the largest degree and is in no clique as large as the one of 4
    assert pend["deg"].argmax() == 4 and pend["members"][0] == 4 and pend["n_members"] < 4
    cap = res["capped_130"][2]
    assert cap["stats"][3] == 70 and cap["stats"][4] == 1 and cap["members"][:70].tolist() == list(range(70)) and (cap["members"][70:] == -1).all()
    capl, free = res["capped_loop_257"][2], res["loop_257"][2]
    assert capl["stats"][4] == 1 and capl["members"][:9].tolist() == free["members"][:9].tolist() and free["n_members"] > 64
    bad = res["nan_inf_70"][2]  # a NaN or an inf anywhere in a record: consistent with nothing
    assert (bad["deg"][[5, 64, 17, 40]] == 0).all() and bad["n_members"] > 10
    for which in ("t0", "r0", "t_max", "r_max"):
        assert [res["edge_%s_%s" % (which, k)][2]["stats"][1] for k in ("below", "on", "above")] == [0, 1, 1]
    assert [res["exact_t0_%s" % k][2]["stats"][1] for k in ("below", "on", "above")] == [0, 1, 1]
    # the words' columns beyond M are zero
    for name, (rec, _, want) in res.items():
        M = len(rec)
        if M % 64:
            assert not (want["adj"][:, -1] >> np.uint64(M % 64)).any(), name
    # fp64 is there for poses 10 km out: the far scene keeps the near scene's set
    assert res["far_10km_129"][2]["members"].tolist() == res["loop_129"][2]["members"].tolist()


def mat(p):
    c, s = math.cos(p[2]), math.sin(p[2])
    return np.array([[c, -s, p[0]], [s, c, p[1]], [0, 0, 1.0]])


def test_prepare_against_matrices():
    poses, src, tgt, rel, _ = R.fixture()
    rec = consistency.prepare(poses, src, tgt, rel)
    assert rec.shape == (600, 8) and rec.dtype == np.float64 and rec.flags.c_contiguous
    arc = np.concatenate([[0.0], np.cumsum(np.hypot(np.diff(poses[:, 0]), np.diff(poses[:, 1])))])
    for m in range(0, 600, 7):
        Wm = mat(poses[tgt[m]]) @ mat(rel[m]) @ np.linalg.inv(mat(poses[src[m]]))
        assert np.abs(rec[m, :4] - [Wm[0, 0], Wm[1, 0], Wm[0, 2], Wm[1, 2]]).max() < 1e-12
        assert rec[m, 4] == poses[tgt[m], 0] and rec[m, 5] == poses[tgt[m], 1]
        assert rec[m, 6] == arc[src[m]] and rec[m, 7] == arc[tgt[m]]
    # records made from the poses themselves: W is the identity
    own = R.compose(R.inverse(poses[tgt]), poses[src])
    rec = consistency.prepare(poses, src, tgt, own)
    assert np.abs(rec[:, :4] - [1.0, 0.0, 0.0, 0.0]).max() < 1e-12
    with pytest.raises(ValueError):
        consistency.prepare(poses, [len(poses)], [0], [[0, 0, 0]])
    with pytest.raises(ValueError):
        consistency.prepare(poses, [1, 2], [0], [[0, 0, 0]])
    assert consistency.prepare(poses, [], [], np.zeros((0, 3))).shape == (0, 8)


def test_defaults_workspace_and_bad_specs_need_no_device():
    lib = _lib.load()
    sp = consistency.default_spec()
    assert C.sizeof(_lib.ConsistencySpec) == 56
    assert (sp.t0, sp.t_rate, sp.t_max, sp.r0, sp.r_rate, sp.r_max, sp.max_steps, sp.flags) == (0.8, 0.1, 16.0, 0.1, 0.005, 0.5, 65536, 0)
    assert consistency.spec(t0=0.25, max_steps=3).t0 == 0.25 and consistency.spec(max_steps=3).max_steps == 3
    with pytest.raises(TypeError):
        consistency.spec(nothing=1)
    assert len(consistency.STATS_FIELDS) == 8 and len(consistency.RECORD_FIELDS) == 8
    # one buffer: the set's state and live set, the matrix, the degrees; 256-byte granules
    for M in (0, 1, 64, 65, 1000, 65536):
        W = (M + 63) // 64
        need = _lib.NHIP_CONSISTENCY_STATE_BYTES + 8 * M * W + 4 * M
        assert consistency.workspace_bytes(M) == (need + 255) // 256 * 256
    assert _lib.NHIP_CONSISTENCY_STATE_BYTES == 256 + 8 * 1024
    for M in (-1, 65537):
        assert lib.nhip_consistency_workspace_bytes(M) == -1 and len(lib.nhip_last_error()) > 0
        with pytest.raises(_lib.NhipError):
            consistency.workspace_bytes(M)
    bad = [dict(t0=-0.1), dict(t_rate=-1.0), dict(r0=math.nan), dict(r_rate=-0.5), dict(t_max=math.nan), dict(r_max=-1.0),
           dict(t0=1.0, t_max=0.5), dict(r0=0.4, r_max=0.3), dict(max_steps=0), dict(max_steps=-3), dict(t_max=math.inf), dict(flags=1)]
    stats = np.zeros(8, dtype=np.int64)
    n = np.zeros(1, dtype=np.int32)
    for kw in bad:
        s = consistency.spec(**kw)
        for rc in (lib.nhip_consistency(None, 0, C.byref(s), None, _lib.ptr(n), _lib.ptr(stats)),
                   lib.nhip_consistency_adjacency_dev(None, 0, C.byref(s), None, None, None, None),
                   lib.nhip_consistency_set_dev(None, None, 0, C.byref(s), 8, None, None, None, None, 1 << 20, None)):
            assert rc == _lib.NHIP_ERR_ARG, kw
            assert len(lib.nhip_last_error()) > 0
        with pytest.raises(ValueError):
            hostside.consistent_set(np.zeros((2, 8)), s)
    # a workspace one byte short is an argument error before anything is launched
    good = consistency.default_spec()
    rc = lib.nhip_consistency_set_dev(None, None, 100, C.byref(good), 8, None, None, None, None, consistency.workspace_bytes(100) - 1, None)
    assert rc == _lib.NHIP_ERR_ARG and b"workspace" in lib.nhip_last_error()
    assert lib.nhip_consistency_set_dev(None, None, 100, C.byref(good), -1, None, None, None, None, 1 << 30, None) == _lib.NHIP_ERR_ARG
    with pytest.raises(ValueError):
        hostside.consistent_set(np.zeros((3, 7)))
    assert consistency.keep(np.array([4, 1, 2, -1, -1]), 3, 5, 3).tolist() == [False, True, True, False, True]
    assert not consistency.keep(np.array([4, 1, 2, -1, -1]), 3, 5, 4).any()
    assert consistency.keep(np.zeros(0, dtype=np.int32), 0, 0, 0).shape == (0,)


def test_the_defaults_meet_their_conditions_on_the_fixture():
    """The conditions the defaults were chosen under (the study's table is in DESIGN.md section 3), on the restatement alone:
    of the fixture's 600 records the set holds at least 80 % of the 450 untouched ones, none of the 50 displaced by one common
    transform, and at most 1 % of its members are displaced records."""
    (kw, members, untouched, displaced, coherent), = R.study([{}])
    print("default spec on the fixture: %d members, %d of 450 untouched, %d of 100 displaced, %d of 50 coherent" % (
        members, untouched, displaced, coherent))
    assert untouched >= 0.8 * 450
    assert coherent == 0
    assert displaced + coherent <= 0.01 * members
