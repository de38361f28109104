"""The bounds phase of csm_bnb_kernel where it keeps a round trip off a wave's way -- (cos, sin) of all of a wave's
rotations at once, the point slots that outlive a rotation, the gather one row ahead, the staging loop's four loads in
flight (nhip_bnb.hip, nhip_bnb_bounds.h, nhip_bnb_origin.h) -- at the rotation counts, scan lengths, pooled-table sizes and
window origins where each can go wrong (tests/rotation_round_trips.py, checked in tests/test_rotation_round_trips_cpu.py):
the branch-and-bound records and sums of every form -- fused, fused with every pair handed over to csm_bnb_rot_kernel, split
in one round, split in rounds of two pairs, each also in the instrumented build -- against the records and sums of the kernels
that perform every add, byte for byte.  400-cell table (and the tables of the staging cases), 17 x 17 translations, both cell
widths.  One child process per cell width, started with NHIP_TUNABLES=1, runs all of it and leaves the arrays.

A non-null pair_kbase: one product caller passes it, nhip_csm_get_transformation (nhip_dropin.hip) for a coarse search of
more than 8 rotations dealt over several workgroups.  test_last_part_of_a_dealt_search goes through it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from nautilus_amd import csm
from tests import dropin_seams as S
from tests import rotation_round_trips as M
from tests.test_csm_gpu import _dropin_info, _same_call

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=[8, 16], ids=["8bit", "16bit"])
def child(request, gpu, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rotation_round_trips") / ("cells%d.npz" % request.param))
    p = subprocess.run([sys.executable, "-m", "tests.rotation_round_trips", str(request.param), out], cwd=ROOT,
                       env=dict(os.environ, NHIP_TUNABLES="1"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode()[-4000:]
    z = np.load(out)
    return z, json.loads(str(z["meta"]))


def _groups(meta):
    """The groups that ran (an even number of rotations is refused, see test_even_rotation_counts_are_refused)."""
    return [g for g in meta if "refused" not in meta[g]]


def test_every_form_equals_the_every_add_kernels(child):
    z, meta = child
    assert len(_groups(meta)) == len([n for n in M.N_THETAS if n % 2]) + 2 + len(M.POOL_SIDES) + 1
    for g in _groups(meta):
        n = meta[g]["n_pairs"]
        want_rec, want_sum = z["rec_%s_every_add" % g], z["sum_%s_every_add" % g]
        assert len(want_sum) == n and len(want_rec) == 16 * n, g
        assert want_sum.min() >= 0 and want_sum.max() > 0, (g, want_sum)  # (the walls are seen: real sums)
        for name in M.EVERY_ADD:
            assert z["rec_%s_%s" % (g, name)].tobytes() == want_rec.tobytes() and np.array_equal(z["sum_%s_%s" % (g, name)], want_sum), (g, name)
        for name in M.FORMS:
            for v in (name, name + "_instr"):
                bad = list(np.nonzero(z["sum_%s_%s" % (g, v)] != want_sum)[0])
                assert not bad, (g, v, "sums differ at pairs", bad)
                rec = z["rec_%s_%s" % (g, v)].reshape(-1, 16)
                bad = list(np.nonzero((rec != want_rec.reshape(-1, 16)).any(axis=1))[0])
                assert not bad, (g, v, "records differ at pairs", bad)
    # an empty scan scores nothing in every form, the full scan something
    lengths = z["sum_lengths_every_add"]
    assert lengths[M.LENGTHS.index(0)] == 0 and lengths[M.LENGTHS.index(1081)] > 0


def test_every_form_ran_what_it_names(child):
    _, meta = child
    for g in _groups(meta):
        for name, (_, form) in M.FORMS.items():
            for v in (name, name + "_instr"):
                launch = meta[g][v]
                # (rounds of two pairs: beside each other on the helper stream where the workspace holds two rounds' state,
                #  form 3; one after the other where a round's state is larger -- 61 rotations -- form 2: bnb_plan)
                forms = (2, 3) if name == "split_rounds" else (form,)
                assert launch["form_id"] in forms and launch["n_pairs"] == meta[g]["n_pairs"], (g, v, launch)
                assert name != "split_rounds" or (launch["pairs_per_round"] == 2 and launch["rounds"] == (meta[g]["n_pairs"] + 1) // 2), (g, v, launch)
                assert launch["instrumented"] == v.endswith("_instr"), (g, v, launch)
                assert launch["hand_over_kernel"] == (name == "hand_over"), (g, v, launch)
    # the tables are the ones the case lists were made for
    for side, residue in M.POOL_SIDES.items():
        m = meta["pool%d" % side]
        assert m["side"] == side and m["pool_words"] % M.ROUND == residue and M.pool_in_lds(m["pool_words"]), m
    m = meta["pool%d" % M.GLOBAL_SIDE]
    assert m["side"] == M.GLOBAL_SIDE and not M.pool_in_lds(m["pool_words"]), m
    assert meta["rows"]["side"] == meta["lengths"]["side"] == M.BASE_SIDE


def test_even_rotation_counts_are_refused(child):
    """8 and 16 rotations -- every wave one, every wave two -- are in the list and cannot be run: a search has an odd number of
    rotations.  The library says so; the counts on either side (7, 9, 15, 17) ran above."""
    _, meta = child
    for n in M.N_THETAS:
        g = "rot%d" % n
        if n % 2 == 0:
            assert meta[g]["refused"] and "n_theta must be odd" in meta[g]["refused"], (g, meta[g])
        else:
            assert "refused" not in meta[g] and meta[g]["fused"]["n_pairs"] == meta[g]["n_pairs"], g
    assert [n for n in M.N_THETAS if n % 2 == 0] == [8, 16]


def test_last_part_of_a_dealt_search(gpu):
    """The product caller with a non-null pair_kbase: ROT of tests/dropin_seams.py at 20 degrees, 41 coarse rotations dealt
    over 6 workgroups of 7 -- waves 0 .. 6 of each have one rotation, wave 7 none -- and part 5's kbase = 35 puts its
    rotation 6 on entry 41, the copy of the last rotation BEHIND the table's 41 entries: the end of the delta table.  The
    source is the target turned by -20 degrees, so the winner is the table's last rotation, found in part 5 (its copy ties and
    must lose).  Against the CPU oracle's two-level search, as tests/test_dropin_seams_gpu.py compares."""
    f = S.flow(S.ROT, 20 * S.DEG)
    assert (f.coarse, f.parts, f.per, f.n_theta1) == ("bnb", 6, 7, 41) and (f.parts - 1) * f.per + f.per - 1 == f.n_theta1
    for bits in (16, 8):
        case = S.rotation_walk(bits)[20]
        got = csm.CorrelativeScanMatcher(*case.ctor, cell_bits=case.bits).GetTransformation(case.a, case.b, case.rot_a, case.rot_b, case.restriction)
        info = _dropin_info()
        assert _same_call(got, S.want(case)), (case.name, got, S.want(case))
        assert info["coarse_itheta"] == 40 and info["chained"] is False and csm.last_launch()["n_pairs"] == 6, info
