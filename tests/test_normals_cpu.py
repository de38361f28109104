"""Scan normals without a GPU: the spec's defaults and its accepted ranges through the C ABI, and what the numpy restatement
(tests/normals_reference.py) says about the method -- its quality against the analytic normals of a synthetic world, what
the fold is worth, and that no input of tests/test_normals_gpu.py has a vote on a bin boundary."""
import ctypes as C

import numpy as np
import pytest

from nautilus_amd import _lib, csm, normals, synth
from tests import normals_reference as R


def test_default_spec_is_the_lua_values():
    s = normals.default_spec()
    assert (s.neighborhood_size, s.neighborhood_step_size, s.mean_distance) == (0.15, 0.1, 0.1)  # default_config.lua:147-156
    assert (s.bin_number, s.max_growth_steps, s.seed, s.flags) == (32, 32, 1, 0)
    assert C.sizeof(_lib.NormalsSpec) == 40
    for k, v in R.DEFAULTS.items():
        assert getattr(s, k) == v
    # (size_t)(1 / (2.0 * 0.1 * 0.1)) is 49, not 50: 2.0 * 0.1 * 0.1 rounds up
    assert R.sample_limit(s.mean_distance) == 49 and 1 / (2.0 * 0.1 * 0.1) < 50.0
    assert normals.spec(seed=9, bin_number=16).seed == 9
    with pytest.raises(TypeError):
        normals.spec(bins=3)


BAD = [dict(neighborhood_size=0.0), dict(neighborhood_size=-0.15), dict(neighborhood_size=float("nan")),
       dict(neighborhood_size=float("inf")), dict(neighborhood_step_size=0.0), dict(neighborhood_step_size=float("inf")),
       dict(neighborhood_step_size=float("nan")), dict(mean_distance=0.0), dict(mean_distance=-0.1), dict(mean_distance=float("nan")),
       dict(mean_distance=float("inf")),
       dict(mean_distance=1e-200),  # (the limit's term overflows)
       dict(mean_distance=0.0622),  # term 129.2: above NHIP_NORMALS_MAX_SAMPLES
       dict(mean_distance=0.8),     # term 0.78: below 1
       dict(bin_number=1), dict(bin_number=0), dict(bin_number=-32), dict(bin_number=65),
       dict(max_growth_steps=-1), dict(max_growth_steps=1025)]


@pytest.mark.parametrize("bad", BAD, ids=lambda d: "%s=%r" % next(iter(d.items())))
def test_out_of_range_spec_is_an_argument_error_without_a_device(bad):
    lib = _lib.load()
    s = normals.spec(**bad)
    for rc in (lib.nhip_normals_estimate_dev(None, None, 0, C.byref(s), None, None, None),
               lib.nhip_normals_estimate(None, C.byref(s), None, None)):
        assert rc == _lib.NHIP_ERR_ARG
        msg = lib.nhip_last_error().decode()
        assert next(iter(bad)) in msg or "sample limit" in msg, msg


def test_edges_of_the_accepted_ranges_and_other_arguments():
    lib = _lib.load()
    nodev = _lib.device_count() == 0
    for ok in (dict(bin_number=2), dict(bin_number=64), dict(max_growth_steps=0), dict(max_growth_steps=1024),
               dict(mean_distance=0.0625),  # term exactly 128
               dict(mean_distance=0.70)):   # term 1.02
        s = normals.spec(**ok)
        rc = lib.nhip_normals_estimate_dev(None, None, 0, C.byref(s), None, None, None)
        assert rc == (_lib.NHIP_ERR_NODEV if nodev else _lib.NHIP_OK), (ok, lib.nhip_last_error())
    s = normals.default_spec()
    assert lib.nhip_normals_estimate_dev(None, None, -1, C.byref(s), None, None, None) == _lib.NHIP_ERR_ARG
    assert b"n_scans" in lib.nhip_last_error()
    assert lib.nhip_normals_estimate_dev(None, None, 0, None, None, None, None) == _lib.NHIP_ERR_ARG
    assert lib.nhip_normals_spec_default(None) == _lib.NHIP_ERR_ARG


@pytest.fixture(scope="module")
def dense_scans():
    bag = synth.SynthBag(40, dense=True)
    ids = [0, 13, 27]
    xy, off = csm.pack_scans([bag.scans[i] for i in ids])
    return xy, off, np.concatenate([bag.normals[i] for i in ids])


@pytest.fixture(scope="module")
def folded(dense_scans):
    xy, off, _ = dense_scans
    return R.estimate(xy, off)


def test_quality_against_the_analytic_normals(dense_scans, folded):
    """Three dense 1081-beam scans of the synthetic room: the share of points whose estimated normal lies within 10 degrees
    of the wall's, modulo sign.  Measured with this restatement: 0.9713 (median error 1.7 degrees, 90th percentile 6.6);
    the bound is that minus 0.03 -- one noisy wall segment more or less moves the share by about 0.01."""
    xy, off, truth = dense_scans
    nrm, info, _ = folded
    share = R.share_within(nrm, truth)
    print("share within 10 degrees: %.4f" % share)
    assert share >= 0.9713 - 0.03
    assert np.all(info[:, 0] >= 2) and np.all(info[:, 2] >= 0) and np.all(info[:, 2] <= 16)  # every bin is a folded one
    assert np.allclose(np.linalg.norm(nrm.astype(np.float64), axis=1), 1.0, atol=1e-6) and np.all(nrm[:, 1] >= -1e-7)


def test_the_fold_is_what_keeps_oblique_walls(dense_scans, folded):
    """The departure DESIGN.md section 3 lists first: without the fold, the sign of a pair's normal follows the random order
    of the pair, and half the votes of an oblique wall land in the bin of its mirror image (measured: 0.8427 against 0.9713)."""
    xy, off, truth = dense_scans
    unfolded = R.estimate(xy, off, fold=False)[0]
    with_fold, without = R.share_within(folded[0], truth), R.share_within(unfolded, truth)
    print("share within 10 degrees: %.4f with the fold, %.4f without" % (with_fold, without))
    assert without < with_fold


@pytest.mark.parametrize("name", sorted(R.PARITY_SPECS))
def test_no_input_of_the_gpu_tests_is_ambiguous(name):
    """What lets tests/test_normals_gpu.py compare every point: no vote of the crafted batch has angle / step within 1e-9 of
    a bin boundary, under either spec it is compared at.  The crafted points are what they are meant to be."""
    xy, off, marks = R.crafted_batch()
    nrm, info, amb = R.crafted_expected(name)
    assert list(np.diff(off)[:len(R.CRAFTED_LENGTHS)]) == list(R.CRAFTED_LENGTHS) and len(xy) < 6000
    assert not amb.any()
    limit = R.sample_limit(dict(R.DEFAULTS, **R.PARITY_SPECS[name])["mean_distance"])
    i = marks["coincident"]
    assert np.all(info[i:i + 12] == (12, 0, -1, limit << 16)) and not nrm[i:i + 12].any()  # samples, no votes
    assert [tuple(info[marks[k]][:2]) for k in ("grow1", "grow2", "grow32", "never")] == [(3, 1), (14, 2), (40, 32), (1, 32)]
    assert tuple(info[marks["never"]]) == (1, 32, -1, 0) and not nrm[marks["never"]].any()
    for k in ("nan", "inf"):
        assert tuple(info[marks[k]]) == (0, 32, -1, 0) and not nrm[marks[k]].any()
    a, u = marks["at_radius"], marks["ulp_inside"]
    assert [tuple(r[:2]) for r in info[a:a + 2]] == [(2, 1), (2, 1)]  # at float(0.15): not a neighbour until the radius grows
    assert [tuple(r[:2]) for r in info[u:u + 2]] == [(2, 0), (2, 0)]  # one ulp closer: a neighbour at once
    assert (info[:, 3] >> 16).max() == limit and info[:, 2].max() <= dict(R.DEFAULTS, **R.PARITY_SPECS[name])["bin_number"] // 2
