"""The device linear solver's CPU half ("Block-sparse system"): the structure builder and the numpy
restatement (tests/linsolve_reference.py) against the host path they replace -- PoseGraph._assemble and scipy's spsolve --
on random row lists and on the three systems the iteration counts of DESIGN section 8 item 12 were taken on.  The GPU half,
which holds the kernels to the restatement: tests/test_linsolve_gpu.py."""
import numpy as np
import pytest

from nautilus_amd import linsolve, posegraph
from tests import linsolve_reference as LR

LAM, FLOOR, TOL = 1e-3, 1e-9, 1e-10
# Two sums of the same n terms in different orders each differ from the exact sum by at most (n - 1) u (sum of magnitudes)
# to first order (u = 2^-53), so from each other by at most 2 (n - 1) u (...); K covers the second-order terms and the
# rounding of the comparison itself: the project's (K + n) 2^-53 (sum of magnitudes) form with both sums' n.
K_SUM = 4


@pytest.fixture(scope="module")
def systems():
    """Per table system: (graph, bag, structure, rows, (values, grad, cost) by the reference), at the graph's start poses."""
    out = {}
    for n, w in LR.CPU_SYSTEMS:
        pg, bag = LR.oracle_graph(n, w)
        u, v, rows = LR.graph_rows(pg, pg.poses.copy(), pg._lines())
        st = linsolve.BlockStructure(pg.n + len(pg.hitl), u, v)
        out[(n, w)] = (pg, bag, st, rows, LR.assemble(st, rows))
    return out


def check_structure(st):
    assert st.row_ptr[0] == 0 and st.row_ptr[-1] == st.nnzb == len(st.col) and np.all(np.diff(st.row_ptr) >= 1)
    assert st.contrib_ptr[0] == 0 and st.contrib_ptr[-1] == st.n_contrib == 4 * st.n_rows
    assert sorted(st.contrib.tolist()) == list(range(4 * st.n_rows)), "every quadrant of every row lands in exactly one block"
    for b in range(st.n_blocks):
        cols = st.col[st.row_ptr[b]:st.row_ptr[b + 1]]
        assert np.all(np.diff(cols) > 0) and b in cols, "columns ascend and the diagonal block is present"
    for k in range(st.nnzb):
        ids = st.contrib[st.contrib_ptr[k]:st.contrib_ptr[k + 1]]
        assert np.all(np.diff(ids) > 0), "contributors ascend"
        r, q = ids >> 2, ids & 3
        row_of = np.where(q < 2, st.u[r], st.v[r])
        col_of = np.where((q == 0) | (q == 2), st.u[r], st.v[r])
        assert np.all(row_of == st.block_row[k]) and np.all(col_of == st.col[k])
    pattern = set(zip(st.block_row.tolist(), st.col.tolist()))
    assert all((c, r) in pattern for r, c in pattern), "the full symmetric pattern is stored"


def dense_from_rows(n_blocks, u, v, rows):
    """(H, g) the way PoseGraph._assemble builds them from 28-double rows: scipy's COO sum, np.add.at."""
    import scipy.sparse as sp
    idx = np.concatenate([3 * u[:, None] + np.arange(3), 3 * v[:, None] + np.arange(3)], axis=1)
    r, c, val = posegraph._blocks_from_normal_equations(rows, idx)
    g = np.zeros(3 * n_blocks)
    np.add.at(g, idx.ravel(), rows[:, 21:27].ravel())
    return sp.coo_matrix((val, (r, c)), shape=(3 * n_blocks, 3 * n_blocks)).tocsc(), g


def assert_matches(st, rows, H, g, cost, what):
    values, grad, c = LR.assemble(st, rows)
    mag_rows = np.abs(rows)
    mag_v, mag_g, mag_c = LR.assemble(st, mag_rows)
    n_v = np.repeat(np.diff(st.contrib_ptr), 9).reshape(-1, 3, 3)
    tol_H = st.to_scipy((K_SUM + 2 * n_v) * LR.U * mag_v).toarray()
    diag = st.block_row == st.col
    n_g = np.zeros(st.n_blocks)
    n_g[st.col[diag]] = np.diff(st.contrib_ptr)[diag]
    tol_g = (K_SUM + 2 * np.repeat(n_g, 3)) * LR.U * mag_g
    err_H, err_g = np.abs(st.to_scipy(values).toarray() - H.toarray()), np.abs(grad - g)
    print("%s: worst |dH| / tol %.3g, |dg| / tol %.3g, |dcost| / tol %.3g" % (
        what, (err_H[tol_H > 0] / tol_H[tol_H > 0]).max(), (err_g[tol_g > 0] / tol_g[tol_g > 0]).max(),
        abs(c - cost) / ((K_SUM + 2 * st.n_rows) * LR.U * mag_c)))
    assert np.all(err_H <= tol_H) and np.all(err_g <= tol_g) and abs(c - cost) <= (K_SUM + 2 * st.n_rows) * LR.U * mag_c
    assert np.abs(H.toarray()).max() > 0


def test_pinned_sum_is_the_stated_order():
    rng = np.random.default_rng(5)
    for n in (0, 1, 63, 64, 65, 128, 129, 300):
        t = rng.normal(size=n) * 10.0 ** rng.uniform(-8, 8, n)
        partial = [0.0] * 64
        for i, v in enumerate(t):
            partial[i % 64] += float(v)
        s = 32
        while s >= 1:
            for l in range(s):
                partial[l] += partial[l + s]
            s //= 2
        assert LR.pinned_sum(t) == partial[0]
    t = np.array([1.0, 2.0 ** -53, 2.0 ** -53] + [0.0] * 61 + [-1.0])
    assert LR.pinned_sum(t) != t.sum() or LR.pinned_sum(t) != float(np.sum(t.astype(LR.LD))), "the case has no teeth"


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_structure_and_reference_assembly_on_random_rows(seed):
    rng = np.random.default_rng(seed)
    nb = int(rng.integers(2, 40))
    R = int(rng.integers(1, 400))
    u = rng.integers(0, nb, R)
    v = (u + rng.integers(1, nb, R)) % nb
    st = linsolve.BlockStructure(nb, u, v)
    check_structure(st)
    rows = LR.random_rows(u, seed)
    H, g = dense_from_rows(nb, u, v, rows)
    assert_matches(st, rows, H, g, 0.5 * float(rows[:, 27].sum()), "random %d" % seed)


def test_structure_without_rows_and_bad_lists():
    st = linsolve.BlockStructure(4, [], [])
    check_structure(st)
    assert st.nnzb == 4 and np.array_equal(st.col, np.arange(4)) and st.n_contrib == 0
    values, grad, cost = LR.assemble(st, np.zeros((0, 28)))
    assert not values.any() and not grad.any() and cost == 0.0
    for u, v in (([0], [0]), ([0], [4]), ([-1], [0]), ([0, 1], [1])):
        with pytest.raises(ValueError):
            linsolve.BlockStructure(4, u, v)


@pytest.mark.parametrize("system", LR.CPU_SYSTEMS[:2])
def test_reference_assembly_equals_the_host_assembly_of_a_graph(systems, system):
    pg, bag, st, rows, _ = systems[system]
    check_structure(st)
    H, g, cost = pg._assemble(pg.poses.copy(), pg._lines(), research=False)
    assert_matches(st, rows, H, g, cost, "graph %r" % (system,))
    assert np.abs(H.toarray()[3 * pg.n:]).max() > 0 and pg.lc.n == 1, "the HITL constraint and the loop closure are part of it"


@pytest.mark.parametrize("system", LR.CPU_SYSTEMS)
def test_reference_pcg_solves_what_spsolve_solves(systems, system):
    from scipy.sparse.linalg import spsolve
    pg, bag, st, rows, (values, grad, cost) = systems[system]
    x, k_ref, rel, flag = LR.pcg(st, values, grad, [0], LAM, FLOOR, TOL, 5000)
    true = LR.true_relative_residual(st, values, grad, [0], LAM, FLOOR, x)
    A, free = LR.damped(st, values, [0], LAM, FLOOR)
    direct = spsolve(A.tocsc(), -grad[free])
    k_scalar = LR.pcg(st, values, grad, [0], LAM, FLOOR, TOL, 5000, "scalar")[1]
    print("PCG %r: k_ref %d (scalar Jacobi %d, cap %d), recursive %.3g, true / tol %.3g, |x - spsolve| max %.3g of %.3g" % (
        system, k_ref, k_scalar, LR.iteration_cap(k_ref), rel, true / TOL, np.abs(x[free] - direct).max(), np.abs(direct).max()))
    assert flag == 0 and rel <= TOL and true <= 10 * TOL
    assert not x[:3].any(), "the fixed block"
    assert LR.iteration_cap(k_ref) < k_scalar, "the cap must tell block Jacobi from scalar Jacobi"
    assert np.abs(x[free] - direct).max() <= 1e-6 * np.abs(direct).max()


def test_reference_pcg_flags():
    u, v = LR.arrow_uv()
    st = linsolve.BlockStructure(71, u, v)
    values, grad, _ = LR.assemble(st, LR.random_rows(u, 7))
    x, k, rel, flag = LR.pcg(st, values, grad, [0], LAM, FLOOR, TOL, 1000)
    assert flag == 0 and k > 3
    x3, k3, _, flag3 = LR.pcg(st, values, grad, [0], LAM, FLOOR, TOL, 3)
    assert (k3, flag3) == (3, 1) and np.isfinite(x3).all()
    assert LR.pcg(st, values, 0 * grad, [0], LAM, FLOOR, TOL, 1000)[1:] == (0, 0.0, 0)
    neg = values.copy()
    neg[np.nonzero((st.block_row == 70) & (st.col == 70))[0][0]] *= -1.0
    xn, kn, _, flagn = LR.pcg(st, neg, grad, [0], LAM, FLOOR, TOL, 1000)
    assert flagn == 2 and np.isfinite(xn).all()


def test_odometry_rows_agree_with_the_host_assembly(systems):
    pg, bag, st, rows, _ = systems[(48, 10)]
    rng = np.random.default_rng(3)
    poses = pg.poses + rng.normal(scale=0.05, size=pg.poses.shape)
    poses[::7, 2] += np.pi  # headings across +-pi
    for fac in (pg.odo, pg.lc):
        r, ji, jj = fac.evaluate(pg.backend, poses)
        got = LR.odometry_rows(r, ji, jj)
        J = np.concatenate([ji, jj], axis=2)
        H = np.einsum("fki,fkj->fij", J, J)
        want = np.concatenate([H[:, LR.IU[0], LR.IU[1]], np.einsum("fki,fk->fi", J, r), (r * r).sum(axis=1)[:, None]], axis=1)
        mag = np.concatenate([np.einsum("fki,fkj->fij", np.abs(J), np.abs(J))[:, LR.IU[0], LR.IU[1]],
                              np.einsum("fki,fk->fi", np.abs(J), np.abs(r)), (r * r).sum(axis=1)[:, None]], axis=1)
        assert np.all(np.abs(got - want) <= (K_SUM + 2 * 3) * LR.U * mag) and np.abs(want).max() > 0


def test_device_solver_needs_a_device_backend(systems):
    pg = systems[(12, 3)][0]
    with pytest.raises(TypeError):
        pg.solve(iterations=1, linear_solver="device")
    with pytest.raises(ValueError):
        pg.solve(iterations=1, linear_solver="gpu")


def test_host_solve_with_reference_pcg_in_place_of_spsolve(systems, monkeypatch):
    """d_ref of tests/test_linsolve_gpu.py's end-to-end test, on the oracle's backend: the largest pose difference between a
    host solve and the same solve with the reference PCG (tol 1e-10) in place of spsolve stays below 1e-6 m."""
    import scipy.sparse.linalg
    pg, bag, st, rows, _ = systems[(48, 10)]
    start = pg.poses.copy()

    def solve():
        pg.poses, pg.hitl[0].chosen_line_pose = start.copy(), np.zeros(3)
        return pg.solve(iterations=4)
    try:
        host, hist = solve()
        counts = []

        def by_pcg(A, b):
            x, k, rel, flag = LR.pcg_matrix(A, b, TOL, 5000)
            counts.append((k, flag))
            return x
        monkeypatch.setattr(scipy.sparse.linalg, "spsolve", by_pcg)
        ref, hist_ref = solve()
    finally:
        pg.poses, pg.hitl[0].chosen_line_pose = start, np.zeros(3)
    d_ref = float(np.abs(ref - host).max())
    print("d_ref %.3g m over %d solves, PCG iterations %r; costs %r / %r" % (d_ref, len(counts), [k for k, _ in counts], hist, hist_ref))
    assert len(counts) == 4 and all(flag == 0 for _, flag in counts)
    assert d_ref < 1e-6
    assert all(b <= a for a, b in zip(hist, hist[1:])) and hist[-1] < hist[0]
