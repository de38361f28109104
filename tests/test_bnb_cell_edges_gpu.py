"""Points on cell edges through the branch-and-bound matcher.  A point whose quotient x / res lies on or one float step
beside an integer is where the bounds phase's single-precision window origins hand over to the double-precision path
(nhip_bnb_origin.h, window_origin): the records must be the oracle's in the fused form, the split form (bounds + seeds, then
candidates) and the form that keeps every rotation in the pair's workgroup -- for scans of fewer than 64 points, of one
workgroup's held origins (<= 1088 points) and longer ones, 8- and 16-bit cells."""
import math
import os

import numpy as np
import pytest

from nautilus_amd import csm
from oracle import oracle as O

pytestmark = pytest.mark.gpu

DEG = math.radians(1.0)
RES = 0.05


def _on_edges(pts):
    """Every coordinate moved to the nearest multiple of RES (as float32), then, point by point, left there or moved one
    float step down or up."""
    snapped = (np.round(pts.astype(np.float64) / RES) * RES).astype(np.float32)
    out = snapped.copy()
    i = np.arange(len(pts))
    for d, to in ((1, -np.inf), (2, np.inf)):
        sel = i % 3 == d
        out[sel] = np.nextafter(snapped[sel], np.float32(to))
    return np.ascontiguousarray(out)


@pytest.mark.parametrize("cell_bits", [8, 16])
def test_points_on_cell_edges_every_form(gpu, small_bag, cell_bits):
    base = small_bag.scans[8]
    pool = np.concatenate([small_bag.scans[i] for i in (6, 7, 9)])
    scans = [_on_edges(pool[:n]) for n in (17, 63, 1081, 1088, 1300)] + [base]
    tgt = len(scans) - 1
    src = np.arange(tgt, dtype=np.int32)
    slot = np.zeros(tgt, dtype=np.int32)
    th0 = np.array([0.0, 0.0, 0.0, 0.01, -0.02], dtype=np.float64)  # (theta0 = 0: the middle rotation is the identity)
    spec = csm.grid_spec(30.0, RES, 2.0, 1e-10, 12, cell_bits)
    ospec = O.grid_spec(30.0, RES, 2.0, 1e-10, cell_bits)
    search = csm.search_spec(7, 25, 25, DEG)
    xy, off = csm.pack_scans(scans)
    st = csm.ScanTable(xy, off)
    grids = csm.LikelihoodGrids(st, [tgt], spec)
    try:
        got, sums = csm.match_pairs(st, grids, src, slot, th0, search)
        for env in ({"NHIP_BNB_KERNELS": "1"}, {"NHIP_BNB_KERNELS": "1", "NHIP_BNB_SPLIT": "1"},
                    {"NHIP_BNB_SPLIT": "1", "NHIP_BNB_SPLIT_BATCH": "2", "NHIP_BNB_SPLIT_MIN": "1"}):
            os.environ.update(env)
            try:
                got_v, sums_v = csm.match_pairs(st, grids, src, slot, th0, search)
            finally:
                for k in env:
                    os.environ.pop(k, None)
            assert got_v.tobytes() == got.tobytes() and np.array_equal(sums_v, sums), env
        ogr = O.grid_build_batch(xy, off, [tgt], ospec)
        want = O.csm_match_batch(xy, off, ogr, ospec, src, slot, th0, O.search_spec(7, 25, 25, DEG))
        for f in ("itheta", "ix", "iy"):
            assert np.array_equal(got[f], want[f]), (f, got[f], want[f])
        assert np.array_equal(sums, want["sum"])
        assert sums.min() > 0  # (the points do score against the target)
    finally:
        grids.close()
        st.close()
