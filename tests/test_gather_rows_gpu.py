"""The gather of the bounds (nhip_bnb_bounds.h coarse_rotation; tests/gather_rows.py states the inputs, checked in
tests/test_gather_rows_cpu.py): run lengths 0, 1, 63, 64, 65, 128 and 129 and a lane whose weight forces the early reduction,
with the pooled table in LDS and at the smallest table that stays in global memory, in every form and its instrumented
build.  Records and sums byte for byte those of the kernels that perform every add; on the saturated
table, where a bound that came out too low would drop a block, the instrumented counts are tests/lattice_edge.py's prediction
and every scan's record is pose 0 with n times the top level.  One child process per cell width, started with
NHIP_TUNABLES=1."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from nautilus_amd import csm
from tests import gather_rows as M
from tests import lattice_edge as L
from tests import rotation_round_trips as RT
from tests import saturated_cases as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=[8, 16], ids=["8bit", "16bit"])
def child(request, gpu, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("gather_rows") / ("cells%d.npz" % request.param))
    p = subprocess.run([sys.executable, "-m", "tests.gather_rows", str(request.param), out], cwd=ROOT,
                       env=dict(os.environ, NHIP_TUNABLES="1"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode()[-4000:]
    z = np.load(out)
    return request.param, z, json.loads(str(z["meta"]))


def _variants():
    return [v for name in M.FORMS for v in (name, name + "_instr")]


def test_every_form_equals_the_every_add_kernels(child):
    _, z, meta = child
    for group in ("lds", "global"):
        n = meta[group]["n_pairs"]
        want_rec, want_sum = z["rec_%s_every_add" % group], z["sum_%s_every_add" % group]
        assert n == len(M.RUNS) + 1 == len(want_sum) and len(want_rec) == 16 * n
        assert (want_sum[1:] > 0).all(), (group, want_sum)  # (every scan but the empty one scores)
        for name in M.EVERY_ADD:
            assert z["rec_%s_%s" % (group, name)].tobytes() == want_rec.tobytes() and np.array_equal(z["sum_%s_%s" % (group, name)], want_sum), (group, name)
        for v in _variants():
            assert np.array_equal(z["sum_%s_%s" % (group, v)], want_sum), (group, v, z["sum_%s_%s" % (group, v)], want_sum)
            assert z["rec_%s_%s" % (group, v)].tobytes() == want_rec.tobytes(), (group, v)


def test_the_table_is_where_the_group_says(child):
    _, _, meta = child
    assert meta["lds"]["side"] == L.SIDE and RT.pool_in_lds(meta["lds"]["pool_words"], M.LDS_THETA)
    assert meta["global"]["side"] == RT.GLOBAL_SIDE and not RT.pool_in_lds(meta["global"]["pool_words"])
    for group in ("lds", "global"):
        for v in _variants():
            name = next(f for f in sorted(M.FORMS, key=len, reverse=True) if v.startswith(f))
            launch = meta[group][v]
            forms = (2, 3) if name == "split_rounds" else (M.FORMS[name][1],)
            assert launch["form_id"] in forms and launch["instrumented"] == v.endswith("_instr"), (group, v, launch)


def test_saturated_records_and_counts(child):
    bits, z, meta = child
    want = L.saturated_counts(M.NXY, M.NXY, M.LDS_THETA)
    rec = z["rec_lds_split"].view(csm.MATCH_DTYPE)
    sums = z["sum_lds_split"]
    for i, (name, pts) in enumerate(M.lds_scans()):
        if len(pts) == 0:
            continue
        assert (int(rec["itheta"][i]), int(rec["ix"][i]), int(rec["iy"][i])) == (0, 0, 0) and int(sums[i]) == len(pts) * S.levels(bits), (name, rec[i], sums[i])
        for form in M.FORMS:
            c = meta["lds"][form + "_counts"][i]
            print(bits, name, form, c)
            assert c == want, (bits, name, form, c, want)
