"""The seeds without their strip bounds (nhip_bnb.hip rotation_pass; tests/seed_passes.py states the rule and the inputs,
checked in tests/test_seed_passes_cpu.py).  Lattices 7 x 7 .. 13 x 13, 9 x 13, 13 x 9 at 1, 3 and 9 rotations and the bench's
81 x 81 at 1; every placed scan -- tests/lattice_edge.py's, a seed block with one sub-block that scores, a scan that scores
nothing -- at 1 .. 193 coincident points; the fused form, the split form and the hand-over kernel, each with its instrumented
build, with the seeds' bounds left out (the default) and with NHIP_BNB_SEED_BOUNDS=1, without a gate and under a gate whose
floor is above 0: records and sums byte for byte those of the kernels that perform every add and of the build that takes
the bounds, and the first maximum of the oracle's volume.  On the saturated table the instrumented build's counters are
tests/lattice_edge.py's prediction either way.  One child process per cell width, started with NHIP_TUNABLES=1."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from nautilus_amd import csm
from oracle import oracle as O
from tests import lattice_edge as L
from tests import saturated_cases as S
from tests import seed_passes as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=[8, 16], ids=["8bit", "16bit"])
def child(request, gpu, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("seed_passes") / ("cells%d.npz" % request.param))
    p = subprocess.run([sys.executable, "-m", "tests.seed_passes", str(request.param), out], cwd=ROOT,
                       env=dict(os.environ, NHIP_TUNABLES="1"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode()[-4000:]
    z = np.load(out)
    return request.param, z, json.loads(str(z["meta"]))


def _names():
    return ["%dx%dx%d" % (nt, nx, ny) for nx, ny, nt in M.groups()]


def _rows(z, g, v):
    return z["rec_%s_%s" % (g, v)].reshape(-1, 16), z["sum_%s_%s" % (g, v)]


def test_every_form_equals_the_every_add_kernels_and_the_build_with_bounds(child):
    _, z, meta = child
    assert sorted(k for k in meta if k != "floors") == sorted(_names())
    for g in _names():
        n = meta[g]["n_pairs"]
        want_rec, want_sum = _rows(z, g, "every_add")
        assert len(want_sum) == n == 16 * len(M.LENGTHS) and len(want_rec) == n, g
        for name in M.EVERY_ADD:
            rec, sums = _rows(z, g, name)
            assert rec.tobytes() == want_rec.tobytes() and np.array_equal(sums, want_sum), (g, name)
        for v in M.variants():
            rec, sums = _rows(z, g, v)
            bad = list(np.nonzero(sums != want_sum)[0])
            assert not bad, (g, v, "sums differ at pairs", bad)
            bad = list(np.nonzero((rec != want_rec).any(axis=1))[0])
            assert not bad, (g, v, "records differ at pairs", bad)
        for v in M.variants():  # switch off against switch on, byte for byte, gated too
            if v.endswith("_bounds"):
                continue
            for tail in ("", "_gated"):
                a, b = _rows(z, g, v + tail), _rows(z, g, v + "_bounds" + tail)
                assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), (g, v, tail)


def test_records_are_the_first_maxima_of_the_oracles_volume(child):
    bits, z, meta = child
    images = {t: O.grid_build(L.target(t), O.grid_spec(L.RANGE, L.RES, L.SIGMA, L.FLOOR_P, bits)) for t in M.TARGETS}
    for nx, ny, n_theta in M.groups():
        g = "%dx%dx%d" % (n_theta, nx, ny)
        for form in M.SEED_FORMS:
            rec = z["rec_%s_%s" % (g, form)].view(csm.MATCH_DTYPE)
            sums = z["sum_%s_%s" % (g, form)]
            for i, (name, t, cell, n) in enumerate(M.sources(nx, ny, bits)):
                pose, best = S.first_maximum(L.volume(images[t], cell, n, nx, ny, n_theta))
                assert (int(rec["itheta"][i]), int(rec["ix"][i]), int(rec["iy"][i])) == pose and int(sums[i]) == best, (g, form, name, rec[i], pose, best)
                if name.startswith("nothing/"):
                    assert pose == (0, 0, 0) and best == 0
                else:
                    assert best > 0, (g, name)
                claim = M.placements(nx, ny, bits)[name.split("/")[0]][2]
                if n_theta == 1 and claim is not None:
                    assert pose == (0,) + claim, (g, name)


def test_a_gate_keeps_the_records_that_reach_its_floor(child):
    bits, z, meta = child
    floors = {int(n): f for n, f in meta["floors"].items()}
    assert all(f >= 2 for f in floors.values()), floors  # (the best starts at sum floor - 1 > 0: every seed keeps its bounds)
    for nx, ny, n_theta in M.groups():
        g = "%dx%dx%d" % (n_theta, nx, ny)
        for v in M.variants():
            rec, sums = _rows(z, g, v)
            grec, gsums = _rows(z, g, v + "_gated")
            # the contract of the gate (tests/test_csm_gate_gpu.py): a record whose score is below min_score is rejected
            kept = rec.copy().view(csm.MATCH_DTYPE).reshape(-1)["score"].astype(np.float64) >= M.MIN_SCORE
            assert kept.any() and not kept.all(), g  # (`nothing` is rejected)
            assert np.array_equal(csm.rejected(grec.copy().view(csm.MATCH_DTYPE).reshape(-1)), ~kept), (g, v)
            assert grec[kept].tobytes() == rec[kept].tobytes() and np.array_equal(gsums[kept], sums[kept]), (g, v)
            assert (gsums[~kept] == -1).all(), (g, v)


def test_every_form_ran_what_it_names_and_reports_the_switch(child):
    _, _, meta = child
    for g in _names():
        assert meta[g]["side"] == L.SIDE and meta[g]["pool_bytes"] <= 36 * 1024, meta[g]  # (the pooled table stays in LDS)
        for v, env in M.variants().items():
            name = next(f for f in sorted(M.SEED_FORMS, key=len, reverse=True) if v.startswith(f))
            launch = meta[g][v]
            assert launch["form_id"] == M.FORMS[name][1] and launch["n_pairs"] == meta[g]["n_pairs"], (g, v, launch)
            assert launch["instrumented"] == ("NHIP_BNB_INSTRUMENT" in env), (g, v, launch)
            assert launch["hand_over_kernel"] == (name == "hand_over"), (g, v, launch)
            assert launch["seed_bounds"] == ("NHIP_BNB_SEED_BOUNDS" in env), (g, v, launch)
            assert launch["l2_runs"] and launch["pair_subs"] and launch["zero_chunks"], (g, v, launch)


def test_seed_passes_leave_their_bounds_out_exactly_when_the_best_sum_is_zero(child):
    """The instrumented build's own account: without a gate some seed begins at a best sum of 0 (the first always does) and
    each of those leaves its bounds out unless the switch is set; under the gate none begins at 0 and none leaves them out.
    A seed per wave with a rotation whose bounds reach above 0: at most min(8, rotations) per pair that scores."""
    bits, _, meta = child
    for nx, ny, n_theta in M.groups():
        g = "%dx%dx%d" % (n_theta, nx, ny)
        scoring = meta[g]["n_pairs"] - len(M.LENGTHS)  # (`nothing` has no seed)
        for v, env in M.variants().items():
            if "_instr" not in v:
                assert meta[g][v + "_stats"] is None
                continue
            s, gs = meta[g][v + "_stats"], meta[g][v + "_gated_stats"]
            print(bits, g, v, s, gs)
            assert scoring <= s["seed_passes_best0"] <= s["seed_passes"] <= scoring * min(8, n_theta), (g, v, s)
            assert s["seed_passes_without_bounds"] == (0 if "NHIP_BNB_SEED_BOUNDS" in env else s["seed_passes_best0"]), (g, v, s)
            assert 0 < gs["seed_passes"] <= scoring * min(8, n_theta), (g, v, gs)
            assert gs["seed_passes_best0"] == 0 and gs["seed_passes_without_bounds"] == 0, (g, v, gs)
            if "NHIP_BNB_SEED_BOUNDS" not in env and n_theta == 1:
                assert s["seed_blocks_zero_sub"] == 0  # (one wave, one seed, no bounds taken: nothing to count)


def test_saturated_counts_are_the_prediction(child):
    bits, _, meta = child
    for nx, ny, n_theta in M.groups():
        g = "%dx%dx%d" % (n_theta, nx, ny)
        want = L.saturated_counts(nx, ny, n_theta)
        for name in M.SEED_FORMS:
            for tail in ("", "_bounds"):
                got = meta[g][name + "_instr" + tail + "_counts"]
                assert len(got) == len(M.LENGTHS)
                for c in got:
                    print(bits, g, name, tail, c)
                    assert {k: c[k] for k in want} == want, (bits, g, name, tail, c, want)
                    assert c["seed_passes"] == min(8, n_theta), (g, name, tail, c)
