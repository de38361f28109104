"""Transient returns in the loop: transient.static_scans -- one occupancy trace, then the filter, in-stream -- against the
reference composition on a 40-scan bag with one walker; the cleaned clouds go into the table build, the occupancy grid and the
map vectorisation unchanged; `examples/slam_loop.py --movers N --drop-transients` runs to the end and prints the stats, and
without the two flags the example's result is the one the parent commit printed (tests/golden/slam_loop_40_scans.json: every
key of its result line that is not a time, recorded from the parent's script on the same arguments)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from nautilus_amd import csm, occupancy, posegraph, synth, transient, vectorize
from tests import transient_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def walked():
    """SynthBag(40) at its truth poses with one walker (the quality test's, tests/test_transient_cpu.py), the occupancy window
    of every pose +- 30 m, the reference composition once"""
    bag = synth.SynthBag(40)
    i = np.arange(40)
    centres = np.stack([bag.truth[0, 0] + 0.15 * i, bag.truth[0, 1] + 2.0 + 0.02 * i], axis=1)
    scans, masks = synth.add_movers(bag.scans, bag.truth, [(centres, 0.3)])
    xy, off = csm.pack_scans(scans)
    occ = occupancy.window_spec(bag.truth, 30.0)
    return xy, off, bag.truth, occ, np.concatenate(masks), R.static_scans(xy, off, bag.truth, occ)


def test_static_scans_equals_the_reference_composition(gpu, walked):
    xy, off, poses, occ, mover, want = walked
    got = transient.static_scans(xy, off, poses, occ)
    R.same(got[:5], want[:5], "static_scans")
    assert got.occupancy_stats.tobytes() == want[5].tobytes() and got.hits.tobytes() == want[6].tobytes()
    assert got.misses.tobytes() == want[7].tobytes()
    R.packing_properties(xy, off, got[:5])
    flagged = got.labels == R.TRANSIENT
    # (the walker's last positions have not been seen through by two later scans yet: not every one of its returns can be flagged)
    assert mover.sum() > 300 and flagged[mover].mean() > 0.5 and flagged[~mover].mean() < 0.01
    # the backend's call: the same, on the clouds it is given
    back = posegraph.HipBackend().drop_transients(poses, occ_spec=occ, xy=xy, offsets=off)
    R.same(back[:5], want[:5], "HipBackend.drop_transients")
    # overrides reach the transient spec
    naive = transient.static_scans(xy, off, poses, occ, support_radius=0)
    R.same(naive[:5], R.static_scans(xy, off, poses, occ, support_radius=0)[:5], "support_radius 0")


def test_cleaned_clouds_go_into_the_other_entry_points(gpu, walked):
    """the table build, the occupancy grid and the vector map take the cleaned clouds as they are, and give what they give on
    the reference's cleaned clouds"""
    xy, off, poses, occ, mover, want = walked
    got = transient.static_scans(xy, off, poses, occ)
    ids = np.array([3, 31], dtype=np.int32)
    spec = csm.grid_spec(max_shift=10)
    tables = []
    for cxy, coff in ((got.xy, got.offsets), (want[0], want[1])):
        st = csm.ScanTable(cxy, coff)
        grids = csm.LikelihoodGrids(st, ids, spec)
        tables.append([grids.interior(k).copy() for k in range(len(ids))])
        grids.close()
        st.close()
    for a, b in zip(*tables):
        assert a.tobytes() == b.tobytes() and a.max() > 0
    a = occupancy.occupancy_grid(got.xy, got.offsets, poses, occ)
    b = occupancy.occupancy_grid(want[0], want[1], poses, occ)
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()
    assert a[3][2] == want[4][0] + want[4][2]  # beams traced: the kept returns
    vspec = vectorize.window_spec(poses, 30.0)
    lines_a, rec_a, stats_a = vectorize.vectorize(got.xy, got.offsets, poses, vspec)
    lines_b, rec_b, stats_b = vectorize.vectorize(want[0], want[1], poses, vspec)
    assert lines_a.tobytes() == lines_b.tobytes() and rec_a.tobytes() == rec_b.tobytes() and stats_a.tobytes() == stats_b.tobytes()
    assert len(lines_a) > 0


def _example(*args):
    run = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "slam_loop.py"), "--scans", "40"] + list(args),
                         capture_output=True, text=True, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    return run.stdout.strip().splitlines()


def test_example_drops_transients_and_prints_the_stats(gpu):
    lines = _example("--movers", "1", "--drop-transients")
    out = json.loads(lines[-1])
    stats = out["transient_stats"]
    assert any(l.startswith("transients: kept %d of %d returns" % (stats["points_static"] + stats["points_unobserved"],
                                                                 sum(stats[k] for k in list(stats)[:4]))) for l in lines[:-1])
    assert out["movers"] == 1 and out["mover_returns"] > 300 and stats["scans_processed"] == 40 and stats["scans_bad_offsets"] == 0
    assert stats["points_transient"] > 0 and stats["points_invalid"] == 0
    assert out["transient_mover_share"] > 0.5 and out["transient_other_share"] < 0.01
    assert out["err_hitl_m"] < 0.05


def test_example_without_the_flags_prints_the_parents_result(gpu):
    lines = _example()
    assert len(lines) == 1
    out = json.loads(lines[0])
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "slam_loop_40_scans.json")))
    rest = {k: v for k, v in out.items() if not (k.endswith("_s") or k == "pcg_by_phase")}
    assert sorted(rest) == sorted(want)
    for k in want:
        assert rest[k] == want[k], (k, rest[k], want[k])
