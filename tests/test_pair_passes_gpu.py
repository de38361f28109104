"""Two live sub-blocks side by side in one pass of exact sums (nhip_bnb.hip strip_sub_blocks, nhip_bnb_exact.h pair_sums8;
tests/pair_passes.py states the pairing and the inputs, checked in tests/test_pair_passes_cpu.py).  Every listed lattice at 1
and 3 rotations (the bench's 81 x 81 at 1), every placed scan -- tests/lattice_edge.py's and three ties between the halves of
a pair, between rows of a half, between a pair and a single -- at 1 .. 193 coincident points, in every form and its
instrumented build, with the switch on and with NHIP_BNB_PAIR_SUBS=0: records and sums byte for byte those of the kernels
that perform every add, and the closed form n * cell of the oracle's table.  On the saturated table the instrumented build's
counters are the numpy prediction: the pair passes and those across a block boundary, 0 with the switch off and in the fused
form, and the sub-blocks evaluated are tests/lattice_edge.py's whatever the pairing.  One child process per cell width,
started with NHIP_TUNABLES=1, runs all of it and leaves the arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from nautilus_amd import csm
from oracle import oracle as O
from tests import lattice_edge as L
from tests import pair_passes as M
from tests import saturated_cases as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=[8, 16], ids=["8bit", "16bit"])
def child(request, gpu, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pair_passes") / ("cells%d.npz" % request.param))
    p = subprocess.run([sys.executable, "-m", "tests.pair_passes", str(request.param), out], cwd=ROOT,
                       env=dict(os.environ, NHIP_TUNABLES="1"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode()[-4000:]
    z = np.load(out)
    return request.param, z, json.loads(str(z["meta"]))


def _names():
    return ["%dx%dx%d" % (nt, nx, ny) for nx, ny, nt in M.groups()]


def test_every_form_equals_the_every_add_kernels(child):
    _, z, meta = child
    assert sorted(meta) == sorted(_names())
    for g in _names():
        n = meta[g]["n_pairs"]
        want_rec, want_sum = z["rec_%s_every_add" % g], z["sum_%s_every_add" % g]
        assert len(want_sum) == n == 17 * len(M.LENGTHS) and len(want_rec) == 16 * n, g
        assert want_sum.min() > 0, (g, want_sum)  # (every placed scan scores)
        for name in M.EVERY_ADD:
            assert z["rec_%s_%s" % (g, name)].tobytes() == want_rec.tobytes() and np.array_equal(z["sum_%s_%s" % (g, name)], want_sum), (g, name)
        for v in M.variants():
            bad = list(np.nonzero(z["sum_%s_%s" % (g, v)] != want_sum)[0])
            assert not bad, (g, v, "sums differ at pairs", bad)
            rec = z["rec_%s_%s" % (g, v)].reshape(-1, 16)
            bad = list(np.nonzero((rec != want_rec.reshape(-1, 16)).any(axis=1))[0])
            assert not bad, (g, v, "records differ at pairs", bad)


def test_records_are_the_closed_forms(child):
    """... and those records are n times one cell of the oracle's table, first maximum in index order."""
    bits, z, meta = child
    images = {t: O.grid_build(L.target(t), O.grid_spec(L.RANGE, L.RES, L.SIGMA, L.FLOOR_P, bits)) for t in M.TARGETS}
    for nx, ny, n_theta in M.groups():
        g = "%dx%dx%d" % (n_theta, nx, ny)
        rec = z["rec_%s_split" % g].view(csm.MATCH_DTYPE)
        sums = z["sum_%s_split" % g]
        for i, (name, t, cell, n) in enumerate(M.sources(nx, ny, bits)):
            pose, best = S.first_maximum(L.volume(images[t], cell, n, nx, ny, n_theta))
            assert (int(rec["itheta"][i]), int(rec["ix"][i]), int(rec["iy"][i])) == pose and int(sums[i]) == best, (g, name, rec[i], pose, best)
            claim = M.placements(nx, ny, bits)[name.split("/")[0]][2]
            if n_theta == 1:
                assert pose == (0,) + claim, (g, name)


def test_every_form_ran_what_it_names_and_reports_the_switch(child):
    _, _, meta = child
    for g in _names():
        assert meta[g]["side"] == L.SIDE and meta[g]["pool_bytes"] <= 36 * 1024, meta[g]  # (the pooled table stays in LDS)
        for v, env in M.variants().items():
            name = next(f for f in sorted(M.FORMS, key=len, reverse=True) if v.startswith(f))
            launch = meta[g][v]
            forms = (2, 3) if name == "split_rounds" else (M.FORMS[name][1],)
            assert launch["form_id"] in forms and launch["n_pairs"] == meta[g]["n_pairs"], (g, v, launch)
            assert launch["instrumented"] == ("NHIP_BNB_INSTRUMENT" in env), (g, v, launch)
            assert launch["hand_over_kernel"] == (name == "hand_over"), (g, v, launch)
            assert launch["pair_subs"] == ("NHIP_BNB_PAIR_SUBS" not in env) and launch["l2_runs"], (g, v, launch)


def test_saturated_counts_are_the_prediction(child):
    bits, _, meta = child
    seen_pairs = 0
    for nx, ny, n_theta in M.groups():
        g = "%dx%dx%d" % (n_theta, nx, ny)
        edge = L.saturated_counts(nx, ny, n_theta)
        for name in M.FORMS:
            for off in (False, True):
                pairs = M.saturated_pairs(nx, ny, n_theta, name, switch=not off)
                want = dict(edge, pair_passes=pairs["pair_passes"], pair_passes_across_blocks=pairs["pair_passes_across_blocks"])
                got = meta[g][name + "_instr" + ("_off" if off else "") + "_counts"]
                assert len(got) == len(M.LENGTHS)
                for c in got:
                    print(bits, g, name, "off" if off else "on", c)
                    assert c == want, (bits, g, name, off, c, want)
                seen_pairs += pairs["pair_passes"] > 0
    assert seen_pairs
