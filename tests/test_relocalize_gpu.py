"""Global localisation on the GPU: HipBackend.global_localize against hostside.global_localize run with the same backend's
matcher, record for record, on a small table spec; and one run at the full spec on the mapped lap, through the map files, held
to the truth within what the host route leaves with the CPU oracle's matcher plus one cell and one step."""
import math

import numpy as np
import pytest

from nautilus_amd import _lib, csm, hostside, rangesig
from tests import relocalize_cases as cases

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def mapped(gpu, tmp_path_factory):
    """the lap's map from HipBackend.occupancy_grid, written as STEM.pgm / STEM.yaml and read back: only the files are known"""
    from nautilus_amd import occupancy, posegraph
    bag = cases.lap()
    xy, off, poses, (x0, y0, w, h) = cases.map_inputs(bag)
    be = posegraph.HipBackend(DEV)
    occ = occupancy.spec(cell_x0=x0, cell_y0=y0, width=w, height=h)
    grid = be.occupancy_grid(poses, spec=occ, xy=xy, offsets=off)[0]
    stem = str(tmp_path_factory.mktemp("relocalize") / "map")
    hostside.write_occupancy_map(stem, grid, occ)
    grid2, info = hostside.read_occupancy_map(stem)
    res, cx0, cy0, width, height = hostside.occupancy_map_window(grid2, info)
    assert np.array_equal(grid2, grid) and (res, cx0, cy0, width, height) == (0.05, x0, y0, w, h)
    window = rangesig.spec(None, res=res, cell_x0=cx0, cell_y0=cy0, width=width, height=height, flags=_lib.NHIP_RANGESIG_UNKNOWN_STOPS)
    return bag, be, grid2, window


def test_global_localize_small_spec_equals_host_route(mapped):
    bag, be, grid, window = mapped
    q = cases.QUERIES[:6]
    qxy, qoff = csm.pack_scans([bag.scans[i] for i in q])
    gs, srch = csm.grid_spec(6.0, 0.05, 2.0, 1e-10, 8), csm.search_spec(21, 17, 17, math.radians(1.0))
    spec = rangesig.spec(window, top_k=3, flags=_lib.NHIP_RANGESIG_UNKNOWN_STOPS)
    got = be.global_localize(qxy, qoff, grid, window, spec=spec, grid_spec=gs, search=srch)
    want = hostside.global_localize(be, qxy, qoff, grid, window, spec=spec, grid_spec=gs, search=srch)
    assert np.array_equal(got["candidates"], want["candidates"]) and np.array_equal(got["anchors"], want["anchors"])
    assert got["stats"].tolist() == want["stats"].tolist() and got["proposals"].tobytes() == want["proposals"].tobytes()
    assert got["records"].tobytes() == want["records"].tobytes() and np.array_equal(got["rank"], want["rank"])
    assert got["poses"].tobytes() == want["poses"].tobytes()
    assert got["records"].shape == (6, 3) and (got["rank"] >= 0).all() and (got["candidates"][:, :, 0] >= 0).all()


def test_global_localize_full_spec(mapped):
    """the 23 queries of tests/relocalize_cases.py -- odd scans, none in the map, NO priors, none left out -- at the defaults:
    the position and heading errors against the truth stay within those of hostside.global_localize with the CPU oracle's
    matcher on the same queries (0.060 m, 0.280 degrees: tests/test_relocalize_cpu.py) plus one cell and one step of the
    lattice: the device route differs from it only by the matcher's exact-score re-ranking"""
    bag, be, grid, window = mapped
    q = cases.QUERIES
    assert len(q) <= 24 and all(i % 2 == 1 for i in q)
    qxy, qoff = csm.pack_scans([bag.scans[i] for i in q])
    r = be.global_localize(qxy, qoff, grid, window)
    assert cases.near_truth(r["proposals"], bag.truth[q]).any(axis=1).all()
    pos, ang = cases.errors(r["poses"], bag.truth[q])
    print("ranks %s; position error max %.4f m, heading error max %.4f deg; %d anchors" % (r["rank"].tolist(), pos.max(), ang.max(), len(r["anchors"])))
    assert (r["rank"] >= 0).all() and r["stats"][6] == 0
    assert pos.max() <= cases.ORACLE_POSITION_ERROR_M + 0.05 and ang.max() <= cases.ORACLE_HEADING_ERROR_DEG + 1.0
