"""The point loops that keep their loads in flight across turns (nhip_bnb_bounds.h coarse_rotation, nhip_bnb_origin.h
cache_origins) at the scan lengths where a turn, a body of a turn or the clamped load can go wrong (tests/point_prefetch.py,
checked in tests/test_point_prefetch_cpu.py): the branch-and-bound records and sums of every form -- fused, fused with every
pair handed over to csm_bnb_rot_kernel, split in one round, split in rounds of two pairs, each also in the instrumented build --
against the records and sums of the kernels that perform every add, byte for byte.  400-cell table, 3 rotations, 17 x 17, both
cell widths.  One child process per cell width, started with NHIP_TUNABLES=1, runs all of it and leaves the arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import point_prefetch as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=[8, 16], ids=["8bit", "16bit"])
def child(request, gpu, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("point_prefetch") / ("cells%d.npz" % request.param))
    p = subprocess.run([sys.executable, "-m", "tests.point_prefetch", str(request.param), out], cwd=ROOT,
                       env=dict(os.environ, NHIP_TUNABLES="1"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode()[-4000:]
    z = np.load(out)
    return z, json.loads(str(z["meta"]))


def test_every_form_equals_the_every_add_kernels(child):
    z, meta = child
    want_rec, want_sum = z["rec_every_add"], z["sum_every_add"]
    assert len(want_sum) == len(M.LENGTHS) and len(want_rec) == 16 * len(M.LENGTHS)
    assert want_sum.min() >= 0 and (want_sum > 0).sum() >= len(M.LENGTHS) - 3, want_sum  # (the walls are seen: real sums)
    for name in M.EVERY_ADD:
        assert z["rec_" + name].tobytes() == want_rec.tobytes() and np.array_equal(z["sum_" + name], want_sum), name
    for name in M.FORMS:
        for v in (name, name + "_instr"):
            bad = [M.LENGTHS[i] for i in np.nonzero(z["sum_" + v] != want_sum)[0]]
            assert not bad, (v, "sums differ at lengths", bad)
            rec = z["rec_" + v].reshape(-1, 16)
            bad = [M.LENGTHS[i] for i in np.nonzero((rec != want_rec.reshape(-1, 16)).any(axis=1))[0]]
            assert not bad, (v, "records differ at lengths", bad)


def test_every_form_ran_what_it_names(child):
    _, meta = child
    for name, (_, form) in M.FORMS.items():
        for v in (name, name + "_instr"):
            launch = meta[v]["launch"]
            print(v, launch, meta[v]["stats"])
            assert launch["form_id"] == form and launch["n_pairs"] == len(M.LENGTHS), (v, launch)
            assert launch["instrumented"] == v.endswith("_instr"), (v, launch)
            assert launch["hand_over_kernel"] == (name == "hand_over"), (v, launch)
    # the loops were walked: the candidates' kernels built window origins (rotation passes by strip path), the hand-over
    # kernel took pairs over, the bounds phase cost clocks
    for v in ("split_instr", "split_rounds_instr", "hand_over_instr"):
        s = meta[v]["stats"]
        assert s["passes_l2_runs"] + s["passes_per_cell_field"] + s["passes_per_cell_capacity"] >= 1, (v, s)
        assert s["clk_origins"] > 0 and s["clk_bounds"] > 0, (v, s)
    assert meta["hand_over_instr"]["stats"]["pairs_handed_over"] >= 1, meta["hand_over_instr"]["stats"]
