"""Scan features without a GPU: the numpy reference of the spec (tests/feature_reference.py) tied to the CPU oracle's scatter
score, the preconditions of the designed inputs the GPU twin (tests/test_features_gpu.py) relies on, the pure-host part of the
C ABI, and PoseGraph's FEATURE mode driven through the oracle's CPU backend."""
import ctypes as C

import numpy as np
import pytest

from nautilus_amd import _lib, csm, features, posegraph, synth
from oracle import oracle as O
from oracle.cpu_backend import OracleBackend
from tests import feature_reference as R


@pytest.fixture(scope="module")
def bag40():
    bag = synth.SynthBag(40)
    xy, off = csm.pack_scans(bag.scans)
    return bag, xy, off, np.concatenate(bag.normals).astype(np.float32)


@pytest.fixture(scope="module")
def ref_clouds(bag40):
    _, xy, off, nrm = bag40
    return R.feature_clouds(xy, nrm, off, R.Spec())


def test_reference_scores_are_the_oracles_scatter_score_of_the_neighbourhoods(bag40):
    """Byte for byte: the reference's vectorised float sums against orc_scatter_matrix_score on the explicitly built,
    ordered neighbourhoods -- one SynthBag scan and the line at 30 degrees (negative scores)."""
    bag = bag40[0]
    spec = R.Spec()
    for pts in (bag.scans[7], R.line(200, 0.05, 30.0)):
        sc = R.scores(pts, spec)
        hoods = [R.neighbourhood(pts, i, spec) for i in range(len(pts))]
        scored = [i for i, h in enumerate(hoods) if h is not None]
        assert len(scored) > 150 and np.array_equal(np.isnan(sc), np.array([h is None for h in hoods]))
        xy, off = csm.pack_scans([pts[hoods[i]] for i in scored])
        want = O.scatter_matrix_scores(xy, off)
        assert want.tobytes() == sc[scored].tobytes()


def test_designed_inputs_hold_their_preconditions():
    S = R.Spec()
    p, e, sc = R.extract_scan(R.line(200, 0.05), S)  # every score a tie at exactly 0, the distance gate hit at exactly 2.0
    assert np.isnan(sc[:10]).all() and (sc[10:] == 0).all() and p == [10, 50, 90, 130, 170] and e == []
    assert float(R._norm(R.line(200, 0.05)[10], R.line(200, 0.05)[50])) == 2.0
    _, e, _ = R.extract_scan(R.line(200, 0.05), R.Spec(threshold=0.0))
    assert e == [199, 159, 119, 78, 38]
    _, _, sc = R.extract_scan(R.line(200, 0.05, 30.0), S)
    assert (sc < 0).sum() > 20 and np.nanmin(sc) > -1e-6  # slightly negative: keys made of bit patterns would order them wrongly
    _, _, sc = R.extract_scan(R.line(200, 0.05, 45.0), S)
    assert (~np.isnan(sc)).sum() == 190 and np.nanmax(np.abs(sc)) < 1e-6  # (x == y: all four scatter entries are one number)
    _, _, sc = R.extract_scan(R.line(11, 0.05), S)
    assert list(np.nonzero(~np.isnan(sc))[0]) == [10]
    for n in (0, 1, 10):
        p, e, sc = R.extract_scan(R.line(n, 0.05), S)
        assert p == [] and e == [] and np.isnan(sc).all()
    _, _, sc = R.extract_scan(R.line(60, 0.2), S)  # the left filter: 0.2 m spacing keeps 4 of the 10 left neighbours
    assert (~np.isnan(sc)).sum() == 43
    _, _, sc = R.extract_scan(R.line(60, 0.9), S)  # no left neighbour within 0.8 m: 9 right ones are too few
    assert np.isnan(sc).all()
    p, e, sc = R.extract_scan(np.ones((40, 2), np.float32), S)  # 0 / 0
    assert np.isnan(sc).all() and p == [] and e == []
    # right neighbours are not distance-tested: the points before the jump score high (an edge), and one of them is picked
    w = R.wall_with_jump()
    p, e, sc = R.extract_scan(w, S)
    assert np.nanmax(sc[50:60]) > 0.008 and any(50 <= i < 60 for i in e) and len(p) >= 2
    assert all(R.neighbourhood(w, i, S) is not None and 60 in R.neighbourhood(w, i, S) for i in range(51, 60))


def test_spec_default_and_struct():
    s = features.default_spec()
    assert C.sizeof(_lib.FeatureSpec) == 40
    assert (s.threshold, s.distance_threshold, s.max_neighbor_distance) == (0.008, 2.0, 0.8)
    assert (s.neighbors_per_side, s.min_neighbors, s.max_planar, s.max_edge) == (10, 10, 20, 10)
    assert {k: getattr(s, k) for k, _ in _lib.FeatureSpec._fields_} == R.Spec().fields()
    assert _lib.load().nhip_feature_spec_default(None) == _lib.NHIP_ERR_ARG


BAD = [dict(neighbors_per_side=0), dict(neighbors_per_side=65), dict(min_neighbors=0), dict(min_neighbors=20),
       dict(neighbors_per_side=3, min_neighbors=6), dict(max_planar=0), dict(max_planar=65), dict(max_edge=0), dict(max_edge=65),
       dict(threshold=float("nan")), dict(threshold=float("inf")), dict(distance_threshold=-1.0),
       dict(distance_threshold=float("inf")), dict(max_neighbor_distance=-0.5), dict(max_neighbor_distance=float("nan"))]


@pytest.mark.parametrize("bad", BAD, ids=lambda d: ",".join("%s=%s" % kv for kv in d.items()))
def test_bad_specs_are_argument_errors(bad):
    """... with or without a device, before anything is launched (every pointer here is NULL)."""
    lib = _lib.load()
    s = features.feature_spec(**bad)
    assert lib.nhip_features_extract_dev(None, None, 0, C.byref(s), None, None, None, None, None, None) == _lib.NHIP_ERR_ARG
    assert len(lib.nhip_last_error()) > 0
    assert lib.nhip_features_extract(None, C.byref(s), None, None, None, None, None) == _lib.NHIP_ERR_ARG
    assert lib.nhip_features_extract_dev(None, None, 0, None, None, None, None, None, None, None) == _lib.NHIP_ERR_ARG


def test_accepted_spec_limits():
    """The ends of the accepted ranges are accepted: with no device the call gets as far as asking for one."""
    lib = _lib.load()
    want = _lib.NHIP_OK if _lib.device_count() > 0 else _lib.NHIP_ERR_NODEV
    for ok in (dict(neighbors_per_side=64, min_neighbors=127, max_planar=64, max_edge=64), dict(neighbors_per_side=1, min_neighbors=1),
               dict(max_planar=1, max_edge=1, threshold=0.0, distance_threshold=0.0, max_neighbor_distance=0.0)):
        s = features.feature_spec(**ok)
        assert lib.nhip_features_extract_dev(None, None, 0, C.byref(s), None, None, None, None, None, None) == want


@pytest.mark.skipif(_lib.load() is not None and _lib.device_count() > 0, reason="GPU present")
def test_entry_points_fail_loudly_without_gpu():
    lib = _lib.load()
    s = features.default_spec()
    assert lib.nhip_features_extract_dev(None, None, 0, C.byref(s), None, None, None, None, None, None) == _lib.NHIP_ERR_NODEV
    assert b"no HIP device" in lib.nhip_last_error()
    assert lib.nhip_features_pack_dev(None, None, None, 0, None, None, 20, None, None, None, None) == _lib.NHIP_ERR_NODEV
    assert lib.nhip_features_extract(None, C.byref(s), None, None, None, None, None) == _lib.NHIP_ERR_NODEV


def _block_counts(icp):
    return np.diff(icp.boff)


def test_feature_mode_solve_on_the_oracle_backend(bag40, ref_clouds):
    """PoseGraph(features=...) through OracleBackend on the reference's clouds: blocks no larger than the caps, and a
    trajectory better than the odometry's."""
    bag, xy, off, nrm = bag40
    (xy_p, nrm_p, off_p), (xy_e, nrm_e, off_e) = ref_clouds
    assert np.diff(off_p).max() <= 20 and np.diff(off_e).max() <= 10 and np.diff(off_p).mean() > 10 and np.diff(off_e).mean() > 3
    pg = posegraph.PoseGraph(None, None, None, bag.odom, window=10, backend=OracleBackend(), features=ref_clouds)
    poses, hist = pg.solve(iterations=8)
    cp, ce = _block_counts(pg.icp.planar), _block_counts(pg.icp.edge)
    assert len(cp) == len(ce) == len(pg.icp.block_src) == sum(min(i, 10) for i in range(40))
    assert cp.max() <= 20 and ce.max() <= 10 and cp.sum() > 0 and ce.sum() > 0 and pg.icp.n_corr == cp.sum() + ce.sum()
    e_odom, e_feat = posegraph.trajectory_error(bag.odom, bag.truth), posegraph.trajectory_error(poses, bag.truth)
    print("trajectory error: odometry %.4f m, FEATURE mode %.4f m; correspondences per block: planar %.2f, edge %.2f"
          % (e_odom, e_feat, cp.mean(), ce.mean()))
    assert hist[-1] < hist[0] and e_feat < e_odom


def test_features_none_changes_nothing(bag40):
    """features=None is the graph as it was: the same batch from backend.icp on the full clouds, the same poses -- for
    PoseGraph and for solve_growing_window -- and FEATURE mode is a different problem."""
    bag, xy, off, nrm = bag40
    sub = slice(0, 12)
    xy12, off12 = csm.pack_scans(bag.scans[sub])
    nrm12 = np.concatenate(bag.normals[sub]).astype(np.float32)
    odom = bag.odom[sub]
    be = OracleBackend()
    a = posegraph.PoseGraph(xy12, nrm12, off12, odom, window=2, backend=be)
    b = posegraph.PoseGraph(xy12, nrm12, off12, odom, window=2, backend=be, features=None)
    assert type(a.icp) is type(b.icp) and not isinstance(b.icp, posegraph._FeatureIcp)
    pa, pb = a.solve(iterations=2)[0], b.solve(iterations=2)[0]
    # what the graph computes without the argument, restated: the Gauss-Newton step of the full-cloud batch
    icp = be.icp(xy12, nrm12, off12, *posegraph.window_pairs(12, 2), 0.25)
    icp.set_poses(odom)
    assert icp.search() == a.icp.n_corr > 5000
    assert pa.tobytes() == pb.tobytes()
    _, ga = posegraph.solve_growing_window(xy12, nrm12, off12, odom, 1, 2, iterations=1, backend=be)
    _, gb = posegraph.solve_growing_window(xy12, nrm12, off12, odom, 1, 2, iterations=1, backend=be, features=None)
    assert ga.tobytes() == gb.tobytes()
    f = R.feature_clouds(xy12, nrm12, off12, R.Spec())
    _, gf = posegraph.solve_growing_window(None, None, None, odom, 1, 2, iterations=1, backend=be, features=f)
    assert gf.shape == ga.shape and np.isfinite(gf).all() and not np.array_equal(gf, ga)


def test_empty_feature_clouds_pass_through(bag40):
    """Scans without edge points -- here: none at all -- and scans without any feature give empty blocks, not errors."""
    bag, xy, off, nrm = bag40
    n = 6
    xy6, off6 = csm.pack_scans(bag.scans[:n])
    nrm6 = np.concatenate(bag.normals[:n]).astype(np.float32)
    (xy_p, nrm_p, off_p), _ = R.feature_clouds(xy6, nrm6, off6, R.Spec())
    keep = off_p[2]  # the planar points of scans 0 and 1 only
    off_some = np.minimum(off_p, keep).astype(np.int32)
    empty = (np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32), np.zeros(n + 1, np.int32))
    pg = posegraph.PoseGraph(None, None, None, bag.odom[:n], window=2, backend=OracleBackend(),
                             features=((xy_p[:keep], nrm_p[:keep], off_some), empty))
    poses, hist = pg.solve(iterations=2)
    assert pg.icp.edge.n_corr == 0 and _block_counts(pg.icp.planar)[1:].sum() == 0 and np.isfinite(poses).all()
    pg = posegraph.PoseGraph(None, None, None, bag.odom[:n], window=2, backend=OracleBackend(), features=(empty, empty))
    poses, hist = pg.solve(iterations=1)
    assert pg.icp.n_corr == 0 and np.allclose(poses, bag.odom[:n], atol=1e-9)  # odometry factors alone: already at their optimum


class _ReferenceFeatures(OracleBackend):
    """The oracle's backend with the numpy reference as its extractor (the product's is HipBackend.features)."""

    def features(self, xy, normals, offsets, spec=None):
        return R.feature_clouds(xy, normals, offsets, R.Spec())


def test_example_loop_runs_in_feature_mode():
    """examples/slam_loop.py run(residual="feature"): the features are extracted once, both growing-window solves use them."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import slam_loop
    out = slam_loop.run(n_scans=60, window=3, iterations=2, residual="feature", backend=_ReferenceFeatures(), min_scatter_score=0.3,
                        cell_bits=8)
    print(out)
    assert out["residual"] == "feature" and out["planar_points"] > 60 * 10 and out["edge_points"] > 60 * 3
    assert 0 < out["icp_correspondences"] <= (60 * 3 - 6) * 30 and out["err_icp_m"] < out["err_odometry_m"]
    assert np.isfinite(out["err_hitl_m"])
    with pytest.raises(ValueError):
        slam_loop.run(n_scans=4, residual="planar", backend=_ReferenceFeatures())
