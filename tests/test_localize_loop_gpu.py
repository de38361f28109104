"""examples/localize.py end to end: the run with --backend hip -- the map ray-traced, the windows gathered, the tables built and
the scans matched on the GPU -- agrees with the run on the CPU oracle (numpy map, numpy windows, the oracle's matcher) on the
queries, the rejected count and the poses, both through the map files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _example(stem, backend):
    run = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "localize.py"), "--backend", backend, "--scans", "24", "--map-scans",
                          "16", "--map", stem], capture_output=True, text=True, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    return json.loads(run.stdout.strip().splitlines()[-1])


def test_example_on_the_gpu_agrees_with_the_oracle_run(gpu, tmp_path):
    hip, cpu = _example(str(tmp_path / "hip"), "hip"), _example(str(tmp_path / "cpu"), "oracle")
    assert hip["backend"] == "hip" and cpu["backend"] == "oracle"
    for stem in ("hip", "cpu"):
        assert os.path.exists(str(tmp_path / stem) + ".pgm") and os.path.exists(str(tmp_path / stem) + ".yaml")
    assert open(str(tmp_path / "hip.pgm"), "rb").read() == open(str(tmp_path / "cpu.pgm"), "rb").read()  # the same map
    for k in ("queries", "rejected", "map_cells", "map_cells_occupied", "points_per_window_min", "points_per_window_max"):
        assert hip[k] == cpu[k], (k, hip[k], cpu[k])
    assert hip["queries"] == 8 and hip["rejected"] == 0
    # the poses are lattice poses: equal records give equal doubles
    assert np.array_equal(np.array(hip["poses"], dtype=np.float64), np.array(cpu["poses"], dtype=np.float64))
    assert hip["position_error_max_m"] <= 0.15 and hip["heading_error_max_deg"] <= 1.0
