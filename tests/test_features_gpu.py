"""Scan features on the GPU (nhip_feat.hip) against the numpy statement of the spec (tests/feature_reference.py, tied to the
CPU oracle by tests/test_features_cpu.py): bit equality of scores and selections, the packed clouds, the three ways in, the
correspondence search on feature clouds, and the FEATURE-mode solve on both backends."""
import ctypes as C

import numpy as np
import pytest

from nautilus_amd import _lib, csm, features, posegraph, synth
from oracle import oracle as O
from tests import feature_reference as R

LENGTHS = [0, 1, 10, 11, 12, 20, 63, 64, 65, 255, 256, 257, 1081, 1088, 1089, 2047, 2048, 2049, 5000]  # (2048: what LDS holds)
SPECS = {"default": R.Spec(),
         "p3": R.Spec(threshold=0.0, neighbors_per_side=3, min_neighbors=2, max_planar=1, max_edge=64)}


@pytest.fixture(scope="module")
def scans(small_bag):
    """One launch's scans: cuts of SynthBag scans at the lengths where the kernel changes path (several scans concatenated
    for the long ones), the designed inputs of tests/test_features_cpu.py, 16 whole scans."""
    cat = np.concatenate(small_bag.scans[:8])
    assert len(small_bag.scans[0]) > 257 and len(cat) > 5000
    out = [cat[:n] for n in LENGTHS]
    out += [R.line(200, 0.05), R.line(200, 0.05, 45.0), R.line(200, 0.05, 30.0), R.line(60, 0.2), R.line(60, 0.9),
            np.ones((40, 2), np.float32), R.wall_with_jump()]
    out += small_bag.scans[16:32]
    xy, off = csm.pack_scans(out)
    rng = np.random.default_rng(5)
    nrm = rng.normal(size=xy.shape).astype(np.float32)
    return xy, off, nrm


@pytest.fixture(scope="module")
def want(scans):
    xy, off, _ = scans
    return {k: R.extract(xy, off, s) for k, s in SPECS.items()}


def _spec(name):
    return features.feature_spec(**SPECS[name].fields())


def _extract_dev(xy, off, spec):
    """nhip_features_extract_dev, called directly: (planar_idx, planar_count, edge_idx, edge_count, scores) + device tensors."""
    import torch
    lib, dev = _lib.load(), torch.device("cuda:0")
    n = len(off) - 1
    d_xy, d_off = torch.from_numpy(xy).to(dev), torch.from_numpy(off).to(dev)
    d_pi = torch.full((n, spec.max_planar), -7, dtype=torch.int32, device=dev)
    d_ei = torch.full((n, spec.max_edge), -7, dtype=torch.int32, device=dev)
    d_pc, d_ec = torch.full((n,), -7, dtype=torch.int32, device=dev), torch.full((n,), -7, dtype=torch.int32, device=dev)
    d_sc = torch.zeros(len(xy), dtype=torch.float64, device=dev)
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.nhip_features_extract_dev(d_xy.data_ptr(), d_off.data_ptr(), n, C.byref(spec), d_pi.data_ptr(), d_pc.data_ptr(),
                                             d_ei.data_ptr(), d_ec.data_ptr(), d_sc.data_ptr(), sp))
    _lib.check(lib.nhip_dev_status(sp, None))
    return (d_pi.cpu().numpy(), d_pc.cpu().numpy(), d_ei.cpu().numpy(), d_ec.cpu().numpy(), d_sc.cpu().numpy()), (d_xy, d_off, d_pi, d_pc, d_ei, d_ec)


@pytest.fixture(scope="module")
def got_default(gpu, scans):
    xy, off, _ = scans
    return _extract_dev(xy, off, _spec("default"))


def _assert_equal(got, want, off):
    pi, pc, ei, ec, sc = got
    wpi, wpc, wei, wec, wsc = want
    for s in range(len(pc)):  # (per scan, so that a failure names the scan)
        a, b = sc[off[s]:off[s + 1]], wsc[off[s]:off[s + 1]]
        assert np.array_equal(np.isnan(a), np.isnan(b)), "scan %d (%d points): NaN positions" % (s, len(a))
        ok = ~np.isnan(b)
        assert a[ok].tobytes() == b[ok].tobytes(), "scan %d (%d points): scores" % (s, len(a))
        assert pc[s] == wpc[s] and list(pi[s]) == list(wpi[s]), "scan %d: planar %s, want %s" % (s, pi[s], wpi[s])
        assert ec[s] == wec[s] and list(ei[s]) == list(wei[s]), "scan %d: edge %s, want %s" % (s, ei[s], wei[s])


@pytest.mark.gpu
def test_extract_bit_equal_default_spec(gpu, scans, want, got_default):
    xy, off, _ = scans
    w = want["default"]
    # the cases are what they are meant to be: ties and the exact gate, negative scores, nothing scored, NaN, both paths
    nl = len(LENGTHS)
    assert list(w[0][nl][:w[1][nl]]) == [10, 50, 90, 130, 170] and (w[4][off[nl + 2]:off[nl + 3]] < 0).sum() > 20
    assert np.isnan(w[4][off[nl + 4]:off[nl + 6]]).all() and w[1][nl + 4] == 0 and w[1][nl - 1] == 20 and w[3][nl - 1] == 10
    assert w[1][:3].sum() == 0 and w[3][:3].sum() == 0 and w[1].max() == 20 and w[3].max() == 10
    _assert_equal(got_default[0], w, off)


@pytest.mark.gpu
def test_extract_bit_equal_short_neighbourhoods_caps_1_and_64(gpu, scans, want):
    xy, off, _ = scans
    w = want["p3"]
    assert w[1].max() == 1 and w[3].max() > 20  # a cap of 1, and more rounds than the default caps ever run
    got, _ = _extract_dev(xy, off, _spec("p3"))
    _assert_equal(got, w, off)


@pytest.mark.gpu
def test_pack_equals_gather(gpu, scans, got_default):
    xy, off, nrm = scans
    (pi, pc, ei, ec, _), (d_xy, d_off, d_pi, d_pc, d_ei, d_ec) = got_default
    import torch
    d_nrm = torch.from_numpy(nrm).to(d_xy.device)
    n = len(off) - 1
    for idx, cnt, d_idx, d_cnt, cap in ((pi, pc, d_pi, d_pc, 20), (ei, ec, d_ei, d_ec, 10)):
        wx, wn, wo = R.clouds(xy, nrm, off, idx, cnt)
        gx, gn, go = features.pack(d_xy, d_nrm, d_off, n, d_idx, d_cnt, cap)
        assert np.array_equal(go, wo) and gx.tobytes() == wx.tobytes() and gn.tobytes() == wn.tobytes() and len(gx) > 100
        gx, gn, go = features.pack(d_xy, None, d_off, n, d_idx, d_cnt, cap)  # without normals
        assert gn is None and np.array_equal(go, wo) and gx.tobytes() == wx.tobytes()


@pytest.mark.gpu
def test_pack_checks_indices_and_counts_from_device_memory(gpu, scans, got_default):
    """An index equal to its scan's length and a count of cap + 1: reported (NHIP_ERR_ARG naming them), never an address;
    the index is left out, the scan with the bad count contributes nothing, every other scan's points are in place, and
    the next call is clean."""
    import torch
    xy, off, nrm = scans
    (pi, pc, _, _, _), (d_xy, d_off, d_pi, d_pc, _, _) = got_default
    lib, n, cap = _lib.load(), len(off) - 1, 20
    a, b = n - 3, n - 9  # two whole scans
    assert pc[a] >= 3 and pc[b] >= 3
    bad_idx, bad_cnt = pi.copy(), pc.copy()
    bad_idx[a, 1] = off[a + 1] - off[a]
    bad_cnt[b] = cap + 1
    d_bi, d_bc = torch.from_numpy(bad_idx).to(d_xy.device), torch.from_numpy(bad_cnt).to(d_xy.device)
    d_nrm = torch.from_numpy(nrm).to(d_xy.device)
    d_xo = torch.zeros(2 * n * cap, dtype=torch.float32, device=d_xy.device)
    d_no, d_oo = torch.zeros_like(d_xo), torch.zeros(n + 1, dtype=torch.int32, device=d_xy.device)
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    info = (C.c_int32 * 4)()
    assert lib.nhip_dev_status(sp, info) == _lib.NHIP_OK
    _lib.check(lib.nhip_features_pack_dev(d_xy.data_ptr(), d_nrm.data_ptr(), d_off.data_ptr(), n, d_bi.data_ptr(), d_bc.data_ptr(), cap,
                                          d_xo.data_ptr(), d_no.data_ptr(), d_oo.data_ptr(), sp))
    assert lib.nhip_dev_status(sp, info) == _lib.NHIP_ERR_ARG
    msg = lib.nhip_last_error().decode()
    assert info[0] == 64 | 128 and info[1] in (64, 128) and "nhip_features_pack_dev" in msg
    assert (list(info)[1:] == [64, int(bad_idx[a, 1]), a * cap + 1] and "feature index" in msg) or \
        (list(info)[1:] == [128, cap + 1, b] and "feature count" in msg)
    good_idx, good_cnt = pi.copy(), pc.copy()
    good_idx[a, 1:-1], good_cnt[a] = pi[a, 2:], pc[a] - 1
    good_cnt[b] = 0
    wx, wn, wo = R.clouds(xy, nrm, off, good_idx, good_cnt)
    go = d_oo.cpu().numpy()
    m = int(go[-1])
    assert np.array_equal(go, wo) and d_xo[:2 * m].cpu().numpy().tobytes() == wx.tobytes()
    assert d_no[:2 * m].cpu().numpy().tobytes() == wn.tobytes()
    assert lib.nhip_dev_status(sp, info) == _lib.NHIP_OK and list(info) == [0, 0, 0, 0]  # reported once
    _lib.check(lib.nhip_features_pack_dev(d_xy.data_ptr(), d_nrm.data_ptr(), d_off.data_ptr(), n, d_pi.data_ptr(), d_pc.data_ptr(), cap,
                                          d_xo.data_ptr(), d_no.data_ptr(), d_oo.data_ptr(), sp))
    assert lib.nhip_dev_status(sp, info) == _lib.NHIP_OK
    assert np.array_equal(d_oo.cpu().numpy()[1:], np.cumsum(pc))
    with pytest.raises(_lib.NhipError):  # the Python layer raises
        features.pack(d_xy, d_nrm, d_off, n, d_bi, d_bc, cap)
    assert lib.nhip_features_pack_dev(d_xy.data_ptr(), None, d_off.data_ptr(), n, d_bi.data_ptr(), d_bc.data_ptr(), 65,
                                      d_xo.data_ptr(), None, d_oo.data_ptr(), sp) == _lib.NHIP_ERR_ARG


@pytest.mark.gpu
def test_handle_api_and_python_layer_equal_the_dev_call(gpu, scans, got_default):
    xy, off, nrm = scans
    pi, pc, ei, ec, sc = got_default[0]
    f = features.extract(xy, off, want_scores=True)
    st = csm.ScanTable(xy, off)
    h = features.extract_on_handle(st, want_scores=True)
    st.close()
    for a, b, c in zip((pi, pc, ei, ec, sc), (f.planar_idx, f.planar_count, f.edge_idx, f.edge_count, f.scores), h):
        assert a.tobytes() == b.tobytes() == c.tobytes() and a.shape == b.shape == c.shape
    assert features.extract(xy, off).scores is None
    (xp, np_, op), (xe, ne, oe) = f.clouds(xy, nrm, off)
    wx, wn, wo = R.clouds(xy, nrm, off, ei, ec)
    assert np.array_equal(oe, wo) and xe.tobytes() == wx.tobytes() and ne.tobytes() == wn.tobytes()
    assert np.array_equal(np.diff(op), pc) and len(xp) == pc.sum() == len(np_)
    # no scans, and scans without points
    e = features.extract(np.zeros((0, 2), np.float32), np.zeros(1, np.int32), want_scores=True)
    assert e.planar_idx.shape == (0, 20) and e.edge_count.shape == (0,) and len(e.scores) == 0
    e = features.extract(np.zeros((0, 2), np.float32), np.zeros(4, np.int32))
    assert (e.planar_idx == -1).all() and (e.edge_idx == -1).all() and not e.planar_count.any() and not e.edge_count.any()
    (xp, np_, op), _ = e.clouds(np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32), np.zeros(4, np.int32))
    assert len(xp) == 0 and len(np_) == 0 and list(op) == [0, 0, 0, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("threshold", [0.008, 0.3])
def test_search_on_feature_clouds_bit_exact(gpu, small_bag, threshold):
    """IcpBatch on the GPU's planar / edge clouds of the 48-scan bag at odometry poses, window 3, against the oracle's search
    on the same clouds, compared as tests/test_corr_gpu.py compares full clouds.  At threshold 0.3 a third of the scans
    have no edge point: empty sources and empty targets."""
    from nautilus_amd.correspondence import IcpBatch, window_pairs
    xy, off = csm.pack_scans(small_bag.scans)
    nrm = np.concatenate(small_bag.normals).astype(np.float32)
    both = posegraph.HipBackend().features(xy, nrm, off, features.feature_spec(threshold=threshold))
    bs, bt = window_pairs(small_bag.n_scans, 3)
    if threshold == 0.3:
        ne = np.diff(both[1][2])
        assert (ne == 0).sum() >= 10 and (ne > 0).sum() >= 10
    total = 0
    for fxy, fnrm, foff in both:
        batch = IcpBatch(fxy, fnrm, foff, bs, bt)
        batch.set_poses(small_bag.odom)
        n = batch.search()
        rows, boff = batch.correspondences()
        wantc, counts, cap = O.corr_search_batch(fxy, fnrm, foff, bs, bt, O.pose_affines(small_bag.odom), 0.25)
        assert np.array_equal(np.diff(boff), counts) and n == counts.sum()
        for b in range(len(bs)):
            assert np.array_equal(rows[boff[b]:boff[b + 1]], wantc[cap[b]:cap[b] + counts[b]]), b
        neq = batch.normal_equations(_lib.NHIP_LIDAR_POINT).cpu().numpy()
        assert not neq[counts == 0].any() and np.isfinite(neq).all()  # empty blocks are zero rows
        total += n
    assert total > (100 if threshold == 0.3 else 300)


@pytest.mark.gpu
def test_feature_solve_agrees_across_backends_without_research(gpu, monkeypatch):
    """SynthBag(24), windows 4..5, FEATURE mode through HipBackend and through OracleBackend on the same GPU-extracted
    clouds: equal correspondence counts, poses within 1e-6 (the bound test_same_loop_on_the_cpu_backend_agrees holds the
    two backends to); and the feature solve searches exactly twice as often as the all-points solve with the same
    arguments -- once per batch and pass, no search again after losing an arena."""
    from nautilus_amd.correspondence import IcpBatch
    from oracle.cpu_backend import OracleBackend
    bag = synth.SynthBag(24)
    xy, off = csm.pack_scans(bag.scans)
    nrm = np.concatenate(bag.normals).astype(np.float32)
    calls = []
    real = IcpBatch.search
    monkeypatch.setattr(IcpBatch, "search", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    be = posegraph.HipBackend()
    kw = dict(window_min=4, window_max=5, iterations=3)
    posegraph.solve_growing_window(xy, nrm, off, bag.odom, backend=be, **kw)
    n_all = len(calls)
    feats = be.features(xy, nrm, off)
    assert np.diff(feats[0][2]).max() <= 20 and np.diff(feats[1][2]).max() <= 10
    del calls[:]
    pg_h, poses_h = posegraph.solve_growing_window(xy, nrm, off, bag.odom, backend=be, features=feats, **kw)
    n_feat = len(calls)
    print("searches: all points %d, FEATURE mode %d" % (n_all, n_feat))
    assert n_all == 2 and n_feat == 2 * n_all
    pg_o, poses_o = posegraph.solve_growing_window(xy, nrm, off, bag.odom, backend=OracleBackend(), features=feats, **kw)
    assert pg_h.icp.planar.n_corr == pg_o.icp.planar.n_corr > 0 and pg_h.icp.edge.n_corr == pg_o.icp.edge.n_corr > 0
    print("max |pose difference| %.3g" % np.abs(poses_h - poses_o).max())
    assert np.abs(poses_h - poses_o).max() < 1e-6


@pytest.mark.gpu
def test_example_loop_in_feature_mode_equals_the_cpu_loop(gpu):
    """examples/slam_loop.py run(residual="feature") on the product (features, search and normal equations on the GPU) and on
    the oracle's backend fed by the numpy reference's features: the same loop, the same trajectory."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import slam_loop
    from tests.test_features_cpu import _ReferenceFeatures
    kw = dict(n_scans=60, window=3, iterations=2, residual="feature", min_scatter_score=0.3, cell_bits=8)
    a, b = slam_loop.run(**kw), slam_loop.run(backend=_ReferenceFeatures(), **kw)
    print(a, b)
    assert a["backend"] == "hip" and a["residual"] == "feature" and a["t_features_s"] > 0
    for k in ("planar_points", "edge_points", "icp_correspondences", "hitl_points"):
        assert a[k] == b[k] > 0, k
    for k in ("err_icp_m", "err_hitl_m"):
        assert abs(a[k] - b[k]) < 1e-6, k


@pytest.mark.gpu
def test_empty_feature_clouds_pass_through_on_the_gpu(gpu, small_bag):
    """No edge point in any scan (an empty cloud: no bytes to upload), planar points in two scans only: empty blocks through
    search, compaction and normal equations, and the poses the oracle's backend gives."""
    from oracle.cpu_backend import OracleBackend
    n = 6
    xy, off = csm.pack_scans(small_bag.scans[:n])
    nrm = np.concatenate(small_bag.normals[:n]).astype(np.float32)
    be = posegraph.HipBackend()
    (xy_p, nrm_p, off_p), _ = be.features(xy, nrm, off)
    keep = off_p[2]
    some = (xy_p[:keep].copy(), nrm_p[:keep].copy(), np.minimum(off_p, keep).astype(np.int32))
    empty = (np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32), np.zeros(n + 1, np.int32))
    for feats in ((some, empty), (empty, empty)):
        a = posegraph.PoseGraph(None, None, None, small_bag.odom[:n], window=2, backend=be, features=feats)
        b = posegraph.PoseGraph(None, None, None, small_bag.odom[:n], window=2, backend=OracleBackend(), features=feats)
        pa, pb = a.solve(iterations=2)[0], b.solve(iterations=2)[0]
        assert a.icp.n_corr == b.icp.n_corr and a.icp.edge.n_corr == 0 and np.abs(pa - pb).max() < 1e-6
    assert a.icp.n_corr == 0
