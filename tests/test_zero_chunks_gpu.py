"""Exact sums that leave out the chunks of the cell list whose windows hold only empty cells (nhip_bnb.hip chunk_mask;
tests/zero_chunks.py states the rule and the inputs, checked in tests/test_zero_chunks_cpu.py).  Lattices 9 x 9 x 1, 17 x 17 x 3
and 81 x 81 x 1 on a 320-cell grid, and the lattice's edge on tests/lattice_edge.py's own; every input in every form -- one
kernel per pair, with hand-over, split, a pair shared by several workgroups -- and its instrumented build, with the switch on
and with NHIP_BNB_ZERO_CHUNKS=0: records and sums byte for byte those of the kernels that perform every add, and the first
maximum of the oracle's volume.  The instrumented build's chunk counters, one pair at a time, are the statement's: where one
entry alone is not empty every pass visits its one chunk of the list's nch; where every chunk holds such an entry, or the
rotation has no usable run list, or the switch is off, every pass visits them all; against an empty table no pass is made.
One child process per cell width, started with NHIP_TUNABLES=1, runs all of it and leaves the arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from nautilus_amd import csm
from oracle import oracle as O
from tests import saturated_cases as S
from tests import zero_chunks as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = ["%dx%dx%d" % (nt, nx, ny) for nx, ny, nt in M.LATTICES]


@pytest.fixture(scope="module", params=[8, 16], ids=["8bit", "16bit"])
def child(request, gpu, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("zero_chunks") / ("cells%d.npz" % request.param))
    p = subprocess.run([sys.executable, "-m", "tests.zero_chunks", str(request.param), out], cwd=ROOT,
                       env=dict(os.environ, NHIP_TUNABLES="1"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode()[-4000:]
    z = np.load(out)
    return request.param, z, json.loads(str(z["meta"]))


def test_every_form_equals_the_every_add_kernels(child):
    bits, z, meta = child
    assert sorted(meta) == sorted(GROUPS + ["edge"])
    for g in GROUPS + ["edge"]:
        n = meta[g]["n_pairs"]
        want_rec, want_sum = z["rec_%s_every_add" % g], z["sum_%s_every_add" % g]
        assert len(want_sum) == n and len(want_rec) == 16 * n, g
        for name in M.EVERY_ADD:
            assert z["rec_%s_%s" % (g, name)].tobytes() == want_rec.tobytes() and np.array_equal(z["sum_%s_%s" % (g, name)], want_sum), (g, name)
        for v in M.variants():
            bad = list(np.nonzero(z["sum_%s_%s" % (g, v)] != want_sum)[0])
            assert not bad, (g, v, "sums differ at pairs", bad)
            rec = z["rec_%s_%s" % (g, v)].reshape(-1, 16)
            bad = list(np.nonzero((rec != want_rec.reshape(-1, 16)).any(axis=1))[0])
            assert not bad, (g, v, "records differ at pairs", bad)


def test_records_are_the_first_maxima_of_the_oracles_volumes(child):
    bits, z, meta = child
    gs = O.grid_spec(M.RANGE, M.RES, M.SIGMA, M.FLOOR_P, bits)
    images = {t: O.grid_build(M.target(t), gs) for t in M.TARGETS}
    for (nx, ny, n_theta), g in zip(M.LATTICES, GROUPS):
        assert meta[g]["side"] == M.SIDE and meta[g]["pad"] == M.PAD, meta[g]
        rec, sums = z["rec_%s_split" % g].view(csm.MATCH_DTYPE), z["sum_%s_split" % g]
        srcs = M.sources(nx, ny, bits)
        assert len(srcs) == meta[g]["n_pairs"]
        for i, (name, t, cells) in enumerate(srcs):
            vol = np.asarray(O.csm_scores(M.scan(cells), images[t], gs, 0.0, O.search_spec(n_theta, nx, ny, M.THETA_STEP)))
            pose, best = S.first_maximum(vol.astype(np.int64))
            assert (int(rec["itheta"][i]), int(rec["ix"][i]), int(rec["iy"][i])) == pose and int(sums[i]) == best, (g, name, rec[i], pose, best)


def test_every_form_ran_what_it_names_and_reports_the_switch(child):
    _, _, meta = child
    for g in GROUPS + ["edge"]:
        for v, env in M.variants().items():
            name = next(f for f in sorted(M.FORMS, key=len, reverse=True) if v.startswith(f))
            launch = meta[g][v]
            forms = (2, 3) if name == "split_rounds" else (M.FORMS[name][1],)
            assert launch["form_id"] in forms and launch["n_pairs"] == meta[g]["n_pairs"], (g, v, launch)
            assert launch["instrumented"] == ("NHIP_BNB_INSTRUMENT" in env), (g, v, launch)
            assert launch["hand_over_kernel"] == (name == "hand_over"), (g, v, launch)
            assert launch["zero_chunks"] == ("NHIP_BNB_ZERO_CHUNKS" not in env) and launch["l2_runs"] and launch["pair_subs"], (g, v, launch)


def test_chunk_counters_are_the_statements(child):
    bits, _, meta = child
    masked_passes = 0
    for (nx, ny, n_theta), g in zip(M.LATTICES, GROUPS):
        if n_theta != 1:
            continue
        srcs = M.sources(nx, ny, bits)
        for form in ("hand_over", "split"):
            for off in (False, True):
                got = meta[g]["%s_instr%s_counts" % (form, "_off" if off else "")]
                assert sorted(int(i) for i in got) == [i for i, s in enumerate(srcs) if M.counted(s[0])]
                for i, c in got.items():
                    name, _, cells = srcs[int(i)]
                    row, col = M.stored_origins(M.scan(cells), 0, 1, nx, ny)
                    nch = M.list_chunks(row, col)
                    print(bits, g, form, "off" if off else "on", name, "nch", nch, c)
                    full, made = c["chunk_visits_full"], c["chunk_visits"]
                    pfull, pmade = c["pose_chunk_visits_full"], c["pose_chunk_visits"]
                    assert full % nch == 0 and pfull % nch == 0 and (bits == 16 or pfull == 0), (g, form, off, name, c)
                    if name.startswith("nothing/"):
                        assert (full, made, pfull, pmade) == (0, 0, 0, 0), (g, form, off, name, c)
                    elif off or not M.has_run_list(row, col) or name.startswith("alternate/"):
                        assert made == full and pmade == pfull, (g, form, off, name, c)
                    else:  # one entry alone is not empty: each pass visits its chunk, one of nch
                        assert made == full // nch and pmade == pfull // nch, (g, form, off, name, c)
                        masked_passes += full // nch if nch > 1 else 0
    assert masked_passes > 0
