"""The seam systems of the device linear solver and their reference, on the CPU (tests/linsolve_seams.py; the GPU half,
which holds the kernels to them: tests/test_linsolve_seams_gpu.py): the structures are what the kernels' thresholds need,
the reference converges on every system with a cap that still tells block Jacobi from scalar Jacobi, the iterate tolerance
is the float64 reference's distance from a longdouble restatement times 16, and a reference that is wrong the way a kernel
could be misses that tolerance a hundredfold."""
import numpy as np
import pytest

from tests import linsolve_reference as LR
from tests import linsolve_seams as S
from tests.test_linsolve_cpu import check_structure


@pytest.fixture(scope="module")
def assembled():
    """name -> (values, grad) by the reference, once per system."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = S.reference_assembly(S.system(name))[:2]
        return cache[name]
    return get


def test_structures_reach_the_kernels_seams():
    for s in (S.chain(86), S.chain(257), S.pair(65), S.hubs()):
        check_structure(s.st)
    assert np.all(np.diff(S.pair(65).st.contrib_ptr) == 65) and S.pair(65).st.nnzb == 4
    for nb in S.CHAINS:
        ga, gb = -(-3 * nb // S.LT), -(-nb // S.LT)
        print("chain(%d): ga %d, gb %d, %d partials of p.q -- %s" % (nb, ga, gb, ga + S.LONG_WGS, S.CHAINS[nb]))
    assert [(-(-3 * nb // S.LT), -(-nb // S.LT)) for nb in S.CHAINS] == [(2, 1), (3, 1), (4, 2), (257, 86), (769, 257)]
    assert 3 * 85 < S.LT < 3 * 85 + 2, "block 85's scalar rows 255, 256, 257 lie in two workgroups"
    h = S.hubs()
    lens = h.row_lengths()
    print("hubs: %d blocks, %d stored blocks, %d rows; hub rows %r; %d long rows; plain rows up to %d" % (
        h.nb, h.st.nnzb, h.st.n_rows, {b: int(lens[b]) for b in S.HUB_ROWS}, int((lens > S.LONG_ROW).sum()),
        int(np.delete(lens, list(S.HUB_ROWS)).max())))
    assert h.nb == 613 and {b: int(lens[b]) for b in S.HUB_ROWS} == S.HUB_ROWS
    assert {64, 65, 256, 257, 514} <= set(S.HUB_ROWS.values()) and sum(66 <= n <= 300 and n not in (256, 257) for n in S.HUB_ROWS.values()) >= 4
    long_rows = np.nonzero(lens > S.LONG_ROW)[0]
    assert long_rows.tolist() == list(S.LONG_HUBS) and len(long_rows) >= 12 > S.LONG_WGS, "a long workgroup takes a second turn"
    assert lens[63] == S.LONG_ROW and 63 not in long_rows, "the longest row that stays a lane's"
    assert {63, 64, 255, 256, 511, 512} <= set(S.HUB_ROWS), "a wave edge and two chunk edges of the list builder"
    assert sum(b >= 512 for b in long_rows) >= 4 and long_rows[-1] == h.nb - 1, "long rows in the last, partial chunk"
    assert np.all(h.u != h.v) and len(set(zip(np.minimum(h.u, h.v), np.maximum(h.u, h.v)))) == h.st.n_rows, "distinct ties"
    for name, fixed in S.hubs_fixed_sets().items():
        assert len(set(fixed)) == len(fixed) < h.nb
    several = S.hubs_fixed_sets()["several"]
    cols = h.st.col[h.st.row_ptr[300]:h.st.row_ptr[301]]
    at = int(np.nonzero(cols == several[3])[0][0])
    assert 10 < at < len(cols) - 10 and several[3] not in S.HUB_ROWS, "a fixed column neighbour in the middle of a long row"
    assert S.hubs_fixed_sets()["long_hub"][0] in long_rows and lens[S.hubs_fixed_sets()["long_hub"][0]] > 2 * S.LT
    iso = S.chain(257, isolated=1).st
    assert iso.n_blocks == 258 and iso.row_ptr[258] - iso.row_ptr[257] == 1 and iso.col[-1] == 257
    assert iso.contrib_ptr[-1] == iso.contrib_ptr[-2], "the isolated block has a diagonal block without contributors"


def test_vectorised_assembly_of_a_chain_is_the_pinned_assembly():
    """A chain's contributor lists have at most 2 entries and a 2-term pinned sum does not depend on the order of its terms,
    so np.add.at restates LR.assemble bit for bit: held to it here on chain(257), used on the two large chains."""
    s = S.chain(257)
    assert np.diff(s.st.contrib_ptr).max() == 2
    want, got = LR.assemble(s.st, s.rows), S.assemble_short_lists(s.st, s.rows)
    assert np.array_equal(S.bits(got[0]), S.bits(want[0])) and np.array_equal(S.bits(got[1]), S.bits(want[1]))
    assert S.bits(got[2]) == S.bits(want[2]) and np.abs(want[1]).min() > 0
    t = np.array([[1.0, 2.0 ** -60], [2.0 ** -60, 1.0], [-0.0, -0.0]])
    for a, b in t:
        assert S.bits(LR.pinned_sum([a, b])) == S.bits(LR.pinned_sum([b, a])) == S.bits(0.0 + a + b)
    for nb in S.BIG_CHAINS:
        assert np.diff(S.chain(nb).st.contrib_ptr).max() == 2
    with pytest.raises(AssertionError):
        S.assemble_short_lists(S.pair(63).st, S.pair(63).rows)


@pytest.mark.parametrize("name", S.PCG_SYSTEMS)
def test_reference_converges_and_its_cap_stays_below_scalar_jacobi(assembled, name):
    s = S.system(name)
    values, grad = assembled(name)
    x, k_ref, rel, flag = LR.pcg(s.st, values, grad, s.fixed, S.LAM, S.FLOOR, S.TOL, 5000)
    k_scalar, flag_scalar = LR.pcg(s.st, values, grad, s.fixed, S.LAM, S.FLOOR, S.TOL, 5000, "scalar")[1::2]
    print("PCG %s: k_ref %d, cap %d, scalar Jacobi %d (flag %d), recursive residual %.3g" % (
        name, k_ref, LR.iteration_cap(k_ref), k_scalar, flag_scalar, rel))
    assert flag == 0 and rel <= S.TOL and k_ref > S.K_ITER
    assert LR.iteration_cap(k_ref) < k_scalar, "the cap must tell block Jacobi from scalar Jacobi"


def test_fixed_sets_of_the_hubs_system_converge(assembled):
    s = S.hubs()
    values, grad = assembled("hubs")
    for what, fixed in S.hubs_fixed_sets().items():
        x, k_ref, rel, flag = LR.pcg(s.st, values, grad, fixed, S.LAM, S.FLOOR, S.TOL, 5000)
        print("PCG hubs, fixed %s (%d blocks): k_ref %d, cap %d" % (what, len(fixed), k_ref, LR.iteration_cap(k_ref)))
        assert flag == 0 and k_ref > S.K_ITER, "more than the %d iterates the GPU test compares" % S.K_ITER


def test_iterate_tolerance_is_the_references_own_error_times_16(assembled):
    worst = 0.0
    for name in ("hubs", "chain86", "chain257"):
        s = S.system(name)
        values, grad = assembled(name)
        f64 = LR.pcg_iterates(s.st, values, grad, s.fixed, S.LAM, S.FLOOR, S.K_ITER)
        ld = LR.pcg_iterates(s.st, values, grad, s.fixed, S.LAM, S.FLOOR, S.K_ITER, longdouble=True)
        for k in range(1, S.K_ITER + 1):
            dx, drel = S.iterate_distance(f64[k], ld[k])
            print("%s k %d: |x_f64 - x_ld| / |x| %.3g, relative residual %.6g differs by %.3g" % (name, k, dx, f64[k][1], drel))
            worst = max(worst, dx, drel)
        # the trace is what max_iters = k returns
        for k in (1, S.K_ITER):
            x, kk, rel, flag = LR.pcg(s.st, values, grad, s.fixed, S.LAM, S.FLOOR, 0.0, k)
            assert (kk, flag) == (k, 1) and np.array_equal(S.bits(x), S.bits(f64[k][0])) and rel == f64[k][1]
        assert f64[S.K_ITER][1] < f64[1][1] < 1.0 and np.abs(f64[1][0]).max() > 0
    print("ITERATE: measured %.3g (constant %.3g), ITERATE_TOL %.3g" % (worst, S.ITERATE_MEASURED, S.ITERATE_TOL))
    assert np.finfo(LR.LD).eps < 2.0 ** -60, "longdouble must carry more than float64 here"
    # (the constant is what was measured; another BLAS may order the reference's own dot products differently, so it is held
    #  to a factor here -- the tolerance itself does not move with the measurement)
    assert S.ITERATE_MEASURED / 4 <= worst <= 2 * S.ITERATE_MEASURED and S.ITERATE_TOL == 16 * S.ITERATE_MEASURED


MUTATIONS = [("pq_twice", "hubs", 256), ("rr_short", "chain257", 256), ("q_stale", "hubs", 511), ("unfixed", "hubs", None)]


@pytest.mark.parametrize("mutation, name, where", MUTATIONS)
def test_a_wrong_reference_misses_the_iterate_tolerance_a_hundredfold(assembled, mutation, name, where):
    s = S.system(name)
    values, grad = assembled(name)
    fixed = s.fixed
    if mutation == "unfixed":  # the fixed neighbour in the middle of hub 300's row
        fixed = S.hubs_fixed_sets()["several"]
        where = fixed[3]
    want = LR.pcg_iterates(s.st, values, grad, fixed, S.LAM, S.FLOOR, S.K_ITER)
    same = S.mutated_iterates(s, values, grad, fixed, S.K_ITER)
    for k in range(S.K_ITER + 1):
        assert np.array_equal(S.bits(same[k][0]), S.bits(want[k][0])) and same[k][1] == want[k][1], "the copy is the reference"
    wrong = S.mutated_iterates(s, values, grad, fixed, S.K_ITER, mutation, where)
    worst = S.worst_distance(wrong, want)
    print("MUTATION %s on %s at block %d: distance %.3g = %.3g ITERATE_TOL" % (mutation, name, where, worst, worst / S.ITERATE_TOL))
    assert worst >= 100 * S.ITERATE_TOL
