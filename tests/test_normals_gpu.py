"""Scan normals on the GPU (nhip_normals.hip) against the numpy statement of the spec (tests/normals_reference.py): the info
words equal, the normals within one float ulp at 1.0, on one launch of crafted scans at the lengths where the kernels change
path; determinism; the three ways in; and the normal-residual solve on estimated normals."""
import numpy as np
import pytest

from nautilus_amd import _lib, csm, normals, posegraph, synth
from tests import normals_reference as R
from tests.normals_device import estimate_dev as _estimate_dev


@pytest.fixture(scope="module")
def batch():
    return R.crafted_batch()


@pytest.fixture(scope="module")
def got_default(gpu, batch):
    xy, off, _ = batch
    nrm, info, st = _estimate_dev(xy, off, normals.default_spec())
    assert st[0] == _lib.NHIP_OK
    return nrm, info


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(R.PARITY_SPECS))
def test_crafted_scans_equal_the_restatement(gpu, batch, name):
    """Lengths 0 .. 2500 around the tile (256), the LDS form's limit (1088) and past it, coincident points, isolated points
    that need 1, 2, 32 growths or never reach two neighbours, NaN and inf points, a pair at exactly float(0.15) and one an ulp
    closer (tests/test_normals_cpu.py asserts that the batch holds them): the info words are equal on every point that is
    not ambiguous -- none is -- and the normals within 2^-23, the rounding of a double cos / sin that differs from numpy's
    in its last bits."""
    xy, off, marks = batch
    want_nrm, want_info, amb = R.crafted_expected(name)
    nrm, info, st = _estimate_dev(xy, off, normals.spec(**R.PARITY_SPECS[name]))
    assert st[0] == _lib.NHIP_OK
    keep = ~amb
    assert amb.sum() <= len(xy) // 10000
    for s in range(len(off) - 1):  # (per scan, so that a failure names the scan)
        sl = slice(off[s], off[s + 1])
        k = keep[sl]
        bad = np.nonzero((info[sl][k] != want_info[sl][k]).any(axis=1))[0]
        assert len(bad) == 0, "scan %d (%d points): info of point %d is %s, want %s" % (
            s, off[s + 1] - off[s], bad[0], info[sl][k][bad[0]], want_info[sl][k][bad[0]])
        err = np.abs(nrm[sl][k].astype(np.float64) - want_nrm[sl][k].astype(np.float64))
        print("scan %d (%d points): largest normal difference %.3g" % (s, off[s + 1] - off[s], err.max() if err.size else 0.0))
        assert err.size == 0 or err.max() <= 2.0 ** -23, "scan %d: normals" % s
    assert np.array_equal(info[keep], want_info[keep])


@pytest.mark.gpu
def test_deterministic_seeded_and_independent_of_the_batch(gpu, batch, got_default):
    xy, off, _ = batch
    nrm, info = got_default
    again = _estimate_dev(xy, off, normals.default_spec())
    assert again[0].tobytes() == nrm.tobytes() and again[1].tobytes() == info.tobytes()
    other = _estimate_dev(xy, off, normals.spec(seed=2))
    assert other[0].tobytes() != nrm.tobytes() and np.array_equal(other[1][:, :2], info[:, :2])  # (the neighbours do not depend on it)
    # a scan estimated alone equals the same scan inside the batch: one of each form, and a short one
    for s in (R.CRAFTED_LENGTHS.index(257), R.CRAFTED_LENGTHS.index(1088), R.CRAFTED_LENGTHS.index(1089), R.CRAFTED_LENGTHS.index(3)):
        sl = slice(off[s], off[s + 1])
        alone = _estimate_dev(xy[sl], np.array([0, off[s + 1] - off[s]], np.int32), normals.default_spec())
        assert alone[0].tobytes() == nrm[sl].tobytes() and alone[1].tobytes() == info[sl].tobytes(), "scan %d" % s


@pytest.mark.gpu
def test_the_three_forms_agree(gpu, batch, got_default):
    xy, off, _ = batch
    nrm, info = got_default
    # the handle form
    st = csm.ScanTable(xy, off)
    h_nrm, h_info = normals.estimate_on_handle(st, info=True)
    assert h_nrm.tobytes() == nrm.tobytes() and h_info.tobytes() == info.tobytes()
    assert normals.estimate_on_handle(st).tobytes() == nrm.tobytes()
    # the Python entry point, and through the backend
    p_nrm, p_info = normals.estimate(xy, off, info=True)
    assert p_nrm.tobytes() == nrm.tobytes() and p_info.tobytes() == info.tobytes()
    assert p_nrm.dtype == np.float32 and p_nrm.shape == (len(xy), 2)
    assert posegraph.HipBackend("cuda:0").normals(xy, off).tobytes() == nrm.tobytes()
    # d_info = NULL
    assert _estimate_dev(xy, off, normals.default_spec(), want_info=False)[0].tobytes() == nrm.tobytes()
    # no scans at all, and scans without points
    assert normals.estimate(np.zeros((0, 2), np.float32), np.zeros(1, np.int32)).shape == (0, 2)
    assert normals.estimate(np.zeros((0, 2), np.float32), np.zeros(4, np.int32)).shape == (0, 2)


@pytest.mark.gpu
def test_a_non_monotone_offset_is_reported_and_its_scan_left_alone(gpu, batch, got_default):
    """The offsets are device memory: the kernels check them.  Entry 2 of {0, 63, -5, 192} is no offset: scan 1 (63 .. -5)
    and scan 2 (-5 .. 192) are refused -- nothing is written for them, the zeros the caller put there stay -- scan 0 is
    estimated as ever, and nhip_dev_status names the first offender."""
    xy, off, _ = batch
    nrm, info = got_default
    s = R.CRAFTED_LENGTHS.index(63)
    pts = xy[off[s]:off[s] + 192]  # (the 63-point scan and what follows it)
    bad_off = np.array([0, 63, -5, 192], np.int32)
    b_nrm, b_info, (rc, st) = _estimate_dev(pts, bad_off, normals.default_spec())
    assert rc == _lib.NHIP_ERR_ARG and b"scan offset" in _lib.load().nhip_last_error()
    assert st[0] == 256 and st[1] == 256 and st[2] == -5 and st[3] in (2, 3)
    assert b_nrm[:63].tobytes() == nrm[off[s]:off[s + 1]].tobytes() and b_info[:63].tobytes() == info[off[s]:off[s + 1]].tobytes()
    assert not b_nrm[63:].any() and np.all(b_info[63:] == -7)
    assert _lib.load().nhip_dev_status(None, None) == _lib.NHIP_OK  # (the record was consumed)
    with pytest.raises(_lib.NhipError):
        normals.estimate(pts, bad_off)
    good = _estimate_dev(pts[:63], np.array([0, 63], np.int32), normals.default_spec())  # (and the library works on)
    assert good[2][0] == _lib.NHIP_OK and good[0].tobytes() == b_nrm[:63].tobytes()


@pytest.mark.gpu
def test_normal_residual_solve_on_estimated_normals(gpu):
    """A 40-scan bag solved by PoseGraph(kind=NHIP_LIDAR_NORMAL) on normals estimated from its clouds ends closer to the
    truth than the odometry it started from (measured: DESIGN.md section 8)."""
    bag = synth.SynthBag(40, dense=True)
    xy, off = csm.pack_scans(bag.scans)
    est = normals.estimate(xy, off)
    analytic = np.concatenate(bag.normals).astype(np.float32)
    share = R.share_within(est, analytic)
    errs = {}
    for name, nrm in (("estimated", est), ("analytic", analytic)):
        pg = posegraph.PoseGraph(xy, nrm, off, bag.odom, window=3, kind=_lib.NHIP_LIDAR_NORMAL)
        errs[name] = posegraph.trajectory_error(pg.solve(iterations=4)[0], bag.truth)
    e_odom = posegraph.trajectory_error(bag.odom, bag.truth)
    print("trajectory error: odometry %.4f m, estimated normals %.4f m, analytic normals %.4f m; %.4f of the estimated "
          "normals within 10 degrees of the analytic ones" % (e_odom, errs["estimated"], errs["analytic"], share))
    assert errs["estimated"] < e_odom
