"""The batched inverse-column solver's reference held to the truth on the CPU (tests/covariance_reference.py; DESIGN.md section 8
item 13), so that the GPU tolerances of tests/test_covariance_gpu.py rest on the reference alone; and the host path of
PoseGraph.cross_covariances, which the device path is compared with."""
import functools

import numpy as np
import pytest

from nautilus_amd import linsolve
from tests import covariance_reference as CR
from tests import linsolve_reference as LR
from tests import linsolve_seams as LS


@functools.lru_cache(maxsize=None)
def graph_system(n_scans, window, loop_closure=True):
    """(structure, values, mask, n) of an oracle graph at its odometry poses: the HITL line block is the mask."""
    pg, _ = LR.oracle_graph(n_scans, window)
    if not loop_closure:
        pg.lc = None
    u, v, rows = LR.graph_rows(pg, pg.poses, pg._lines())
    st = linsolve.BlockStructure(pg.n + len(pg.hitl), u, v)
    return st, LR.assemble(st, rows)[0], tuple(range(pg.n, pg.n + len(pg.hitl))), pg.n


def pairs_of(n):
    return [(n - 1, 5), (5, n - 1), (n // 2, n // 2 + 1), (1, n - 1), (n - 2, n // 3)]


@pytest.mark.parametrize("n_scans,window,lc", [(48, 10, True), (200, 3, False)])
def test_restatement_matches_the_dense_inverse(n_scans, window, lc):
    """The restatement at tol = 1e-10 against np.linalg.inv of the cut matrix: the wanted 2 x 2 block within 2^-24 of the
    block's largest entry (measured: 8.0e-12 at most)."""
    st, values, mask, n = graph_system(n_scans, window, lc)
    worst = 0.0
    for s_, t_ in pairs_of(n):
        gauge = max(min(s_, t_) - 1, 0)
        A, free = CR.cut(st, values, mask, gauge)
        inv = np.linalg.inv(A.toarray())
        pos = -np.ones(3 * st.n_blocks, dtype=np.int64)
        pos[free] = np.arange(len(free))
        want = inv[np.ix_([pos[3 * s_], pos[3 * s_ + 1]], [pos[3 * t_], pos[3 * t_ + 1]])]
        got = np.zeros((2, 2))
        for c in range(2):
            x, k, rel, flag = CR.column(st, values, mask, gauge, 3 * t_ + c)
            assert flag == 0
            got[:, c] = x[[3 * s_, 3 * s_ + 1]]
        d = np.abs(got - want).max() / np.abs(want).max()
        print("DENSE %d/%d pair (%d, %d) gauge %d: %d iterations, block error / largest entry %.3g, cond %.3g" % (
            n_scans, window, s_, t_, gauge, k, d, np.linalg.cond(A.toarray())))
        worst = max(worst, d)
        assert d <= 2.0 ** -24
    print("DENSE %d/%d worst %.3g" % (n_scans, window, worst))


def test_iterate_constant_covers_the_restatements_own_error():
    """ITERATE_MEASURED_COLUMNS: the float64 restatement against the longdouble one over the held iterates of every system
    of every batch list, recomputed here."""
    worst, where = 0.0, None
    for name in CR.MATRICES:
        M = CR.matrix(name)
        for g, j, what in M.batch:
            if M.column(g, j)[1] == 0:
                continue
            f = CR.column_iterates(M.st, M.values, M.mask, g, j, CR.K_ITER)
            with np.errstate(all="ignore"):
                ld = CR.column_iterates(M.st, M.values, M.mask, g, j, CR.K_ITER, longdouble=True)
            held = CR.held_iterates(f)
            if not held:
                continue
            d = LS.worst_distance(f, ld, held)
            if d > worst:
                worst, where = d, (name, g, j, what, held[-1])
    print("ITERATE_MEASURED_COLUMNS: measured %.3g at %r; constant %.3g, tolerance %.3g" % (
        worst, where, CR.ITERATE_MEASURED_COLUMNS, CR.ITERATE_TOL_COLUMNS))
    assert worst <= CR.ITERATE_MEASURED_COLUMNS
    assert CR.ITERATE_TOL_COLUMNS == 16 * CR.ITERATE_MEASURED_COLUMNS


def test_batch_lists_hold_what_they_promise():
    for name in CR.MATRICES:
        M = CR.matrix(name)
        a, b = CR.IDENTICAL
        assert M.batch[a][:2] == M.batch[b][:2]
        for i in (CR.MASKED_RHS, CR.GAUGE_RHS):
            assert M.column(*M.batch[i][:2])[1:] == (0, 0.0, 0)
        assert {g for g, _, _ in M.batch} >= {-1, 0, M.nb - 1 - (3 if name == "chain40+3" else 0)}
    M = CR.matrix("chain40+3")
    counts = [M.column(g, j)[1] for g, j, _ in M.batch]
    assert counts[-1] in (1, 2) and counts[-2] in (1, 2) and max(counts) >= 20, "an early end among long runs"
    assert LS.HUB_ROWS[300] > LS.LONG_ROW


def test_iteration_cap_stays_below_scalar_jacobi():
    """Where the cap has teeth: on hubs() and on the oracle graph, whose diagonal blocks are far from diagonal, the cap of
    every system's block-Jacobi count stays below the scalar-Jacobi count of the same system -- a wrong preconditioner
    fails the cap on the GPU.  (On the plain chains the two counts lie within the cap's margin of each other: printed.)"""
    M = CR.matrix("hubs")
    for g, j, what in M.batch:
        k = M.column(g, j)[1]
        if k == 0:
            continue
        ks = M.column(g, j, precond="scalar")[1]
        print("CAP hubs (%d, %d): block %d, cap %d, scalar %d" % (g, j, k, LR.iteration_cap(k), ks))
        assert LR.iteration_cap(k) < ks
    st, values, mask, n = graph_system(48, 10)
    for s_, t_ in pairs_of(n):
        gauge = max(min(s_, t_) - 1, 0)
        k = CR.column(st, values, mask, gauge, 3 * t_)[1]
        ks = CR.column(st, values, mask, gauge, 3 * t_, precond="scalar")[1]
        print("CAP graph 48/10 (%d, %d): block %d, cap %d, scalar %d" % (gauge, 3 * t_, k, LR.iteration_cap(k), ks))
        assert LR.iteration_cap(k) < ks
    M = CR.matrix("chain86")
    for g, j, what in M.batch:
        k = M.column(g, j)[1]
        if k:
            print("CAP chain86 (%d, %d): block %d, cap %d, scalar %d" % (g, j, k, LR.iteration_cap(k), M.column(g, j, precond="scalar")[1]))


def _host_blocks_before_this_keyword(pg, pairs):
    """PoseGraph.cross_covariances as it stood before it took linear_solver and dtype, restated."""
    import scipy.sparse as sp
    from scipy.sparse.linalg import splu
    H, _, _ = pg._assemble(pg.poses, pg._lines(), research=False)
    H = H.tocsc()[:3 * pg.n][:, :3 * pg.n]
    out = np.zeros((len(pairs), 2, 2), dtype=np.float32)
    by_gauge = {}
    for k, (s_, t_) in enumerate(pairs):
        by_gauge.setdefault(max(min(int(s_), int(t_)) - 1, 0), []).append(k)
    for gauge, ks in by_gauge.items():
        free = np.concatenate([np.arange(0, 3 * gauge), np.arange(3 * gauge + 3, 3 * pg.n)])
        pos = -np.ones(3 * pg.n, dtype=np.int64)
        pos[free] = np.arange(len(free))
        lu = splu(H[free][:, free].tocsc() + 1e-12 * sp.identity(len(free), format="csc"))
        for k in ks:
            s_, t_ = int(pairs[k][0]), int(pairs[k][1])
            if s_ == gauge or t_ == gauge:
                continue
            rhs = np.zeros((len(free), 2))
            rhs[pos[3 * t_], 0] = 1.0
            rhs[pos[3 * t_ + 1], 1] = 1.0
            x = lu.solve(rhs)
            out[k] = x[[pos[3 * s_], pos[3 * s_ + 1]], :].astype(np.float32)
    return out


def test_host_path_default_is_unchanged_and_float64_is_its_values_before_the_cast():
    pg, _ = LR.oracle_graph(48, 10)
    pairs = pairs_of(pg.n) + [(7, 0), (0, 9)]
    default = pg.cross_covariances(pairs)
    assert default.dtype == np.float32 and default.shape == (len(pairs), 2, 2)
    assert np.array_equal(default.view(np.int32), _host_blocks_before_this_keyword(pg, pairs).view(np.int32))
    wide = pg.cross_covariances(pairs, dtype=np.float64)
    assert wide.dtype == np.float64
    assert np.array_equal(wide.astype(np.float32).view(np.int32), default.view(np.int32))
    assert np.array_equal(pg.cross_covariances(pairs, linear_solver="host").view(np.int32), default.view(np.int32))
    assert not wide[-2].any() and not wide[-1].any() and np.abs(wide[0]).max() > 0
    with pytest.raises(ValueError):
        pg.cross_covariances(pairs, linear_solver="gpu")
    with pytest.raises(ValueError):
        pg.cross_covariances(pairs, dtype=np.float16)
    with pytest.raises(TypeError):
        pg.cross_covariances(pairs, linear_solver="device")  # (the oracle's backend has no device linear solver)
