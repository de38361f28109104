"""The end-to-end loop writes the occupancy grid of its solved trajectory: `examples/slam_loop.py --grid-output STEM`
ray-traces the final poses' scans on the GPU (HipBackend.occupancy_grid), writes STEM.pgm and STEM.yaml and reports
occupancy_s and the three cell counts."""
import os
import sys

import numpy as np
import pytest

from nautilus_amd import csm, hostside, occupancy, posegraph, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _slam_loop():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import slam_loop
    return slam_loop


@pytest.mark.gpu
def test_loop_writes_the_grid_of_its_final_poses(gpu, tmp_path):
    stem = str(tmp_path / "map")
    out = _slam_loop().run(n_scans=40, window=3, iterations=2, min_scatter_score=0.3, cell_bits=8, grid_output=stem)
    assert os.path.exists(stem + ".pgm") and os.path.exists(stem + ".yaml")
    grid, info = hostside.read_occupancy_map(stem)
    assert out["occupancy_s"] > 0
    counts = [int((grid == v).sum()) for v in (100, 0, -1)]
    assert [out["grid_occupied"], out["grid_free"], out["grid_unknown"]] == counts and counts[0] > 500 and counts[1] > 50000
    # the same call here, on the poses the run reports (the bag is the loop's: slam_loop.run)
    poses = np.array(out["grid_poses"], dtype=np.float64)
    assert poses.shape == (40, 3)
    spec = occupancy.window_spec(poses)
    assert [spec.cell_x0, spec.cell_y0, spec.width, spec.height] == out["grid_window"] and grid.shape == (spec.height, spec.width)
    bag = synth.SynthBag(40, dense=True)
    xy, off = csm.pack_scans(bag.scans)
    got, hits, misses, stats = posegraph.HipBackend().occupancy_grid(poses, spec=spec, xy=xy, offsets=off)
    assert np.array_equal(got, grid) and stats[5:].tolist() == counts
    assert info["resolution"] == spec.res and info["origin"] == [spec.cell_x0 * spec.res, spec.cell_y0 * spec.res, 0.0]
    assert info["occupied_thresh"] == 0.65 and info["free_thresh"] == 0.196 and info["negate"] == 0
    # every occupied cell lies in the room (24 m x 16 m, centred; drift and noise of a few centimetres)
    cy, cx = np.nonzero(grid == 100)
    assert np.abs((cx + spec.cell_x0 + 0.5) * spec.res).max() < 12.5 and np.abs((cy + spec.cell_y0 + 0.5) * spec.res).max() < 8.5
