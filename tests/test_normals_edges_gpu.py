"""The scan normals at their sample-list, bin-count and mask edges (kernels nhip_normals.hip, K9; DESIGN.md section 3, "Scan
normals"): specs at the last rows of the LDS and the private taken lists and one past the LDS list, bin counts 2 .. 5, 63 and 64,
scans every point of which has every other as a neighbour, a point at exactly the grown radius, pairs of subnormal and of
underflowing squared length, and a launch of 65,600 scans -- each against the numpy restatement (tests/normals_reference.py): the
four info words equal, the normals within 2^-23 (the rounding of a double cos / sin that differs from numpy's in its last bits,
as in tests/test_normals_gpu.py).  Inputs: tests/normals_edges.py (tests/test_normals_edges_cpu.py holds their preconditions:
none of their points is ambiguous, so none is left out)."""
import numpy as np
import pytest

from nautilus_amd import _lib, normals
from tests import normals_edges as E
from tests.normals_device import estimate_dev

pytestmark = pytest.mark.gpu


def _run(spec_name, xy, off, **kw):
    nrm, info, st = estimate_dev(xy, off, normals.spec(**E.SPECS[spec_name]), **kw)
    assert st == (_lib.NHIP_OK, [0, 0, 0, 0]), st
    return nrm, info


@pytest.mark.parametrize("spec,inp", E.CASES, ids=["%s-%s" % c for c in E.CASES])
def test_edge_inputs_equal_the_restatement(gpu, spec, inp):
    """Every (spec, input) pair of normals_edges.CASES: info words equal on every point that is not ambiguous -- none is --
    and normals within 2^-23; twice, with the same bytes.  A failure names the scan."""
    xy, off = E.INPUTS[inp]()
    want_nrm, want_info, amb = E.expected(spec, inp)
    nrm, info = _run(spec, xy, off, fill=-7.25)
    keep = ~amb
    assert amb.sum() <= len(xy) // 10000
    worst = 0.0
    for s in np.nonzero(np.diff(off))[0]:  # (per scan, so that a failure names the scan)
        sl = slice(off[s], off[s + 1])
        k = keep[sl]
        bad = np.nonzero((info[sl][k] != want_info[sl][k]).any(axis=1))[0]
        assert len(bad) == 0, "scan %d (%d points): info of point %d is %s, want %s" % (
            s, off[s + 1] - off[s], bad[0], info[sl][k][bad[0]], want_info[sl][k][bad[0]])
        err = np.abs(nrm[sl][k].astype(np.float64) - want_nrm[sl][k].astype(np.float64))
        worst = max(worst, err.max() if err.size else 0.0)
        assert err.size == 0 or err.max() <= 2.0 ** -23, "scan %d (%d points): normals differ by %.3g" % (s, off[s + 1] - off[s], err.max())
    print("%s on %s: %d points, largest normal difference %.3g" % (spec, inp, len(xy), worst))
    assert np.array_equal(info[keep], want_info[keep])
    again = _run(spec, xy, off, fill=-7.25)
    assert again[0].tobytes() == nrm.tobytes() and again[1].tobytes() == info.tobytes()


@pytest.mark.parametrize("spec", ["lds_full", "general_full"])
def test_a_blob_alone_equals_the_blob_in_the_batch(gpu, spec):
    """In both forms: a scan's normals are a function of its points and the seed, wherever it sits in a launch -- with every
    mask word full and the taken list at its last row too."""
    xy, off = E.dense_blobs()
    nrm, info = _run(spec, xy, off)
    for s, n in enumerate(E.BLOB_LENGTHS):
        sl = slice(off[s], off[s + 1])
        a_nrm, a_info = _run(spec, xy[sl], np.array([0, n], np.int32))
        assert a_nrm.tobytes() == nrm[sl].tobytes() and a_info.tobytes() == info[sl].tobytes(), "scan %d (%d points)" % (s, n)


def test_without_info_the_normals_are_the_same(gpu):
    """d_info = NULL under the spec that fills the private list."""
    for inp in ("dense_blobs", "tiny_pairs"):
        xy, off = E.INPUTS[inp]()
        nrm, _ = _run("general_full", xy, off)
        bare, none = _run("general_full", xy, off, want_info=False)
        assert none is None and bare.tobytes() == nrm.tobytes(), inp


def test_65600_scans_launch_and_leave_the_tail_alone(gpu):
    """The grid is (n_scans, 5): the scan index on x, where 65,536 and more launch.  Scans 65,535, 65,536 and the last have
    points; their normals are written, and nothing behind the last point is (estimate_dev keeps filler there and checks it)."""
    xy, off = E.many_scans()
    want_nrm, want_info, _ = E.expected("default", "many_scans")
    nrm, info = _run("default", xy, off, fill=-7.25)
    for s in E.MANY_NON_EMPTY:
        sl = slice(off[s], off[s + 1])
        assert sl.stop > sl.start and np.array_equal(info[sl], want_info[sl]), "scan %d" % s
        assert not np.any(nrm[sl] == np.float32(-7.25)), "scan %d: not written" % s
    assert off[-1] == len(xy) and np.all(nrm != np.float32(-7.25)) and np.all(info[:, 0] >= 1)
