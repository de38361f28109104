"""The branch-and-bound matcher at the lattice's edge: blocks of the last block column / row of a lattice that is no multiple
of 8 hold sub-blocks without a single pose, which the matcher neither counts as alive nor evaluates (nhip_bnb.hip
process_candidate_c / process_candidate; tests/lattice_edge.py states the rule and the inputs, checked in
tests/test_lattice_edge_cpu.py).  Every lattice of the list at 1 and 3 rotations (the bench's 81 x 81 at 1), every placed
scan at every length, in every form -- fused, fused with every rotation handed over to csm_bnb_rot_kernel, split in one round,
split in rounds of two pairs shared among workgroups, each also in the instrumented build -- against the records and sums of
the kernels that perform every add, byte for byte, and against the closed form n * cell of the oracle's table.  On the
saturated table (bound == sum: everything stays alive, every block is taken once, order cannot matter) the instrumented
build's counters are the numpy prediction: no sub-block without a pose evaluated, edge blocks whole only where all four
sub-blocks hold poses (never at the bench's residue).  The list's lattices with an even side, a multiple of 8 among them,
cannot reach the kernels -- a search has odd sides -- and are shown to be refused; the odd sides beside them run.
One child process per cell width, started with NHIP_TUNABLES=1, runs all of it and leaves the arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from nautilus_amd import csm
from oracle import oracle as O
from tests import dropin_seams as D
from tests import lattice_edge as L
from tests import saturated_cases as S
from tests.test_csm_gpu import _dropin_info, _same_call

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=[8, 16], ids=["8bit", "16bit"])
def child(request, gpu, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("lattice_edge") / ("cells%d.npz" % request.param))
    p = subprocess.run([sys.executable, "-m", "tests.lattice_edge", str(request.param), out], cwd=ROOT,
                       env=dict(os.environ, NHIP_TUNABLES="1"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode()[-4000:]
    z = np.load(out)
    return request.param, z, json.loads(str(z["meta"]))


def _names(ran=True):
    """The groups that ran (ran=False: those with an even side, which the library refuses)."""
    return ["%dx%dx%d" % (nt, nx, ny) for nx, ny, nt in L.groups() if L.admitted(nx, ny) == ran]


def _ran():
    return [g for g in L.groups() if L.admitted(g[0], g[1])]


def test_every_form_equals_the_every_add_kernels(child):
    _, z, meta = child
    assert sorted(meta) == sorted(_names() + _names(False)) and len(_names()) == 2 * (4 + len(L.ODD_NEIGHBOURS)) - 1
    for g in _names():
        n = meta[g]["n_pairs"]
        want_rec, want_sum = z["rec_%s_every_add" % g], z["sum_%s_every_add" % g]
        assert len(want_sum) == n == 14 * len(L.LENGTHS) and len(want_rec) == 16 * n, g
        assert want_sum.min() > 0, (g, want_sum)  # (every placed scan scores)
        for name in L.EVERY_ADD:
            assert z["rec_%s_%s" % (g, name)].tobytes() == want_rec.tobytes() and np.array_equal(z["sum_%s_%s" % (g, name)], want_sum), (g, name)
        for name in L.FORMS:
            for v in (name, name + "_instr"):
                bad = list(np.nonzero(z["sum_%s_%s" % (g, v)] != want_sum)[0])
                assert not bad, (g, v, "sums differ at pairs", bad)
                rec = z["rec_%s_%s" % (g, v)].reshape(-1, 16)
                bad = list(np.nonzero((rec != want_rec.reshape(-1, 16)).any(axis=1))[0])
                assert not bad, (g, v, "records differ at pairs", bad)


def test_records_are_the_closed_forms(child):
    """... and the every-add kernels' records are n times one cell of the oracle's table, first maximum in index order."""
    bits, z, meta = child
    images = {t: O.grid_build(L.target(t), O.grid_spec(L.RANGE, L.RES, L.SIGMA, L.FLOOR_P, bits)) for t in L.TARGETS}
    for nx, ny, n_theta in _ran():
        g = "%dx%dx%d" % (n_theta, nx, ny)
        rec = z["rec_%s_fused" % g].view(csm.MATCH_DTYPE)
        sums = z["sum_%s_fused" % g]
        for i, (name, t, cell, n) in enumerate(L.sources(nx, ny, bits)):
            pose, best = S.first_maximum(L.volume(images[t], cell, n, nx, ny, n_theta))
            assert (int(rec["itheta"][i]), int(rec["ix"][i]), int(rec["iy"][i])) == pose and int(sums[i]) == best, (g, name, rec[i], pose, best)
            claim = L.placements(nx, ny, bits)[name.split("/")[0]][2]
            if n_theta == 1:
                assert pose == (0,) + claim, (g, name)


def test_every_form_ran_what_it_names(child):
    _, _, meta = child
    for g in _names():
        assert meta[g]["side"] == L.SIDE and meta[g]["pool_bytes"] <= 36 * 1024, meta[g]  # (the pooled table stays in LDS)
        for name, (_, form) in L.FORMS.items():
            for v in (name, name + "_instr"):
                launch = meta[g][v]
                forms = (2, 3) if name == "split_rounds" else (form,)
                assert launch["form_id"] in forms and launch["n_pairs"] == meta[g]["n_pairs"], (g, v, launch)
                assert launch["instrumented"] == v.endswith("_instr"), (g, v, launch)
                assert launch["hand_over_kernel"] == (name == "hand_over"), (g, v, launch)


def test_saturated_counts_are_the_prediction(child):
    bits, _, meta = child
    seen_edge = seen_whole = 0
    for nx, ny, n_theta in _ran():
        g = "%dx%dx%d" % (n_theta, nx, ny)
        want = L.saturated_counts(nx, ny, n_theta)
        for name in L.FORMS:
            got = meta[g][name + "_counts"]
            assert len(got) == len(L.LENGTHS)
            for c in got:
                print(bits, g, name, c)
                assert c == want, (bits, g, name, c, want)
                assert c["sub_blocks_without_pose"] == 0
                if nx % L.B <= L.B4 and ny % L.B <= L.B4:
                    assert c["edge_blocks_whole"] == 0, (g, name, c)
                assert c["edge_blocks_refined"] > 0, (g, name, c)  # (an odd side is no multiple of 8)
                seen_edge += c["edge_blocks_whole"] == 0
                seen_whole += c["edge_blocks_whole"] > 0
    assert seen_edge and seen_whole
    assert L.saturated_counts(9, 9, 1)["blocks_whole"] == 1 and L.saturated_counts(9, 9, 1)["sub_blocks"] == 5


def test_even_sides_are_refused(child):
    """(4, 4), (5, 4), (8, 8), (12, 9) and (13, 16) are in the list and cannot be run: a search has odd sides, so a lattice that
    is a multiple of 8 -- where the counters of the edge would stay 0 -- never reaches the kernels.  The library says so, in
    the branch-and-bound and in the every-add form; the odd sides on either side ran above."""
    _, _, meta = child
    assert len(_names(False)) == 2 * 5
    for g in _names(False):
        assert meta[g]["refused"] and "must be odd" in meta[g]["refused"], (g, meta[g])
    for nx, ny in L.LATTICES:
        if not L.admitted(nx, ny):
            for n in (nx, ny):
                if n % 2 == 0:
                    assert {(n - 1) , (n + 1)} <= {v for pair in L.ODD_NEIGHBOURS + L.LATTICES for v in pair}, (nx, ny)


def test_drop_in_call_on_a_lattice_with_an_edge_block(gpu):
    """nhip_csm_get_transformation with ROT of tests/dropin_seams.py: 49 x 49 coarse translations, 6 blocks of 8 and one pose
    -- the bench's residue -- with the truth one step beyond the upper and beyond the lower corner, so that the coarse sums
    rise towards the edge.  Against the CPU oracle's two-level search, as tests/test_dropin_seams_gpu.py compares."""
    f = D.flow(D.ROT, 3 * D.DEG)
    assert f.coarse == "bnb" and f.side1 == 49 and f.side1 % L.B == 1
    for bits in (16, 8):
        walk = D.translation_walk(D.ROT, bits, False)
        for ij in ((f.h1 + 1, f.h1 + 1), (-f.h1 - 1, -f.h1 - 1)):
            case = walk[ij]
            got = csm.CorrelativeScanMatcher(*case.ctor, cell_bits=case.bits).GetTransformation(case.a, case.b, case.rot_a, case.rot_b, case.restriction)
            info = _dropin_info()
            assert _same_call(got, D.want(case)), (case.name, got, D.want(case), info)
