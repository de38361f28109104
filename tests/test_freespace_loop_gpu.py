"""The free-space check inside HipBackend.match and the example loop ("Free-space check"): the counts of the
matcher's own records equal the numpy reference's, the call without the parameter is what it was, and --lc-verify on the
product keeps what the host path keeps on the CPU backend."""
import numpy as np
import pytest

from nautilus_amd import csm, freespace, posegraph
from tests import freespace_reference as R

pytestmark = pytest.mark.gpu


def test_match_with_freespace_counts_its_own_records(gpu, small_bag):
    bag = small_bag
    xy, off = csm.pack_scans(bag.scans)
    src, tgt, th0 = bag.sample_pairs(per_target=2, targets=np.array([5, 15, 30]), min_sep=1)
    backend = posegraph.HipBackend()
    plain = backend.match(xy, off, src, tgt, th0, 16)
    assert len(plain) == 3
    m, spec, search, counts = backend.match(xy, off, src, tgt, th0, 16, freespace=freespace.default_spec())
    assert m.tobytes() == plain[0].tobytes() and (search.n_theta, search.nx, search.ny) == (61, 81, 81)
    assert counts.shape == (len(src), 8) and counts.dtype == np.int32
    want = R.counts(xy, off, src, tgt, th0, m, spec, search)
    assert np.array_equal(counts, want)
    assert (counts[:, 0] == np.diff(off)[src]).all() and (counts[:, 3] > 0).all()
    wide = backend.match(xy, off, src, tgt, th0, 16, freespace=freespace.spec(hit_radius=0, end_margin=0))[3]
    assert np.array_equal(wide, R.counts(xy, off, src, tgt, th0, m, spec, search, R.make_spec(0, 0)))
    assert (wide[:, 3] <= counts[:, 3]).all() and (wide[:, 6] >= counts[:, 6]).all()
    empty = backend.match(xy, off, src[:0], tgt[:0], th0[:0], 16, freespace=freespace.default_spec())
    assert len(empty) == 4 and empty[3].shape == (0, 8)
    with pytest.raises(ValueError, match="submap"):
        backend.match(xy, off, src, tgt, th0, 16, submap_radius=2, poses=bag.odom, freespace=freespace.default_spec())


def test_the_loop_verifies_on_the_device_what_the_host_path_verifies(gpu):
    """examples/slam_loop.py --lc-verify free-space on the product (the check inside HipBackend.match) and on the oracle's CPU
    backend (hostside.freespace_counts): the same records kept and rejected."""
    import examples.slam_loop as loop
    from oracle.cpu_backend import OracleBackend
    kw = dict(n_scans=32, window=3, spacing=0.06, hitl=False, gate="geometric", iterations=2)
    plain = loop.run(**kw)
    assert plain["backend"] == "hip" and plain["lc_accepted"] > 20
    for permille in (None, 5):
        dev = loop.run(lc_verify="free-space", lc_max_violation=permille, **kw)
        assert dev["lc_verified"] + dev["lc_verify_rejected"] == plain["lc_accepted"]
        assert dev["lc_accepted"] == dev["lc_verified"] and (dev["lc_verify_rejected"] > 0) == (permille == 5)
    # (at the default the shares are far from the gate: the two backends' poses, equal to solver precision, decide alike)
    host = loop.run(backend=OracleBackend(), lc_verify="free-space", **kw)
    assert (dev["lc_max_violation"], host["lc_max_violation"]) == (5, 200)
    dev = loop.run(lc_verify="free-space", **kw)
    assert (dev["lc_verified"], dev["lc_verify_rejected"]) == (host["lc_verified"], host["lc_verify_rejected"])
