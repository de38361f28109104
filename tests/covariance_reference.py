"""The batched inverse-column solver's specification in numpy ("Block-sparse system", section 8 item 13;
kernels nhip_linsolve_columns.hip): one system of nhip_bsr_pcg_columns_dev restated with tests/linsolve_reference.py's PCG, the
matrices and the ONE batch list the CPU and the GPU tests share, and the tolerances.  Nothing here runs on a device."""
import functools

import numpy as np

from nautilus_amd import linsolve
from tests import linsolve_reference as LR
from tests import linsolve_seams as LS

RIDGE, TOL = 1e-12, 1e-10
CT, CB = 64, 32  # nhip_linsolve_columns.hip's tile: systems per workgroup (one wave's lanes), block rows per workgroup
K_ITER = LS.K_ITER

# The largest ||x_k(float64 restatement) - x_k(longdouble restatement)|| / ||x_k|| and the largest relative difference of the
# recursive relative residual over the held iterates (k = 1 .. 8, as far as held_iterates() goes) of every system of
# every batch list of MATRICES (tests/test_covariance_cpu.py measures and prints them): 6.87e-13, x of chain5w2's system
# (last gauge, next to it) at k = 7, two iterations before its 9 free scalars are exhausted; 2.8e-13 on chain256, 3e-15 on
# hubs() -- a unit right-hand side at a chain's end meets the whole spectrum, which the gradient right-hand sides of
# tests/linsolve_seams.py do not (1.8e-15 there).  Rounded up to two digits.
# ITERATE_TOL_COLUMNS is that times 16, linsolve_seams.py's margin: the device orders its sums differently from numpy (a
# lane's blocks in row order, four waves, the per-workgroup partials) and the differences compound over 8 iterations.
# Measured against the restatement at higher precision, never fitted to the kernels' output.
ITERATE_MEASURED_COLUMNS = 6.9e-13
ITERATE_TOL_COLUMNS = 16 * ITERATE_MEASURED_COLUMNS

# An iterate is held to the restatement while the restatement itself means something: once a system's recursive residual
# has fallen below ITERATE_FLOOR the following iterates are CG run on rounding noise (a right-hand side in an isolated
# block is solved by the preconditioner in ONE iteration; a 5-block chain has at most 12 unknowns) and the float64 and the
# longdouble restatements themselves part by O(1) there.  1e-6 leaves ten decades above float64's unit roundoff.
ITERATE_FLOOR = 1e-6


# ------------------------------------------------------------------------------------------------ one system, restated
def cut(st, values, fixed, gauge, ridge=RIDGE):
    """(A over the free scalars, their indices): H cut as LR.damped cuts it, by the shared mask plus the gauge (-1: none),
    with ridge I in place of the lambda term."""
    import scipy.sparse as sp
    held = list(fixed) + ([int(gauge)] if gauge >= 0 else [])
    A, free = LR.damped(st, values, held, 0.0, 0.0)
    return (A + ridge * sp.identity(A.shape[0], format="csr")).tocsr(), free


def unit_rhs(free, j):
    """e_j over the free scalars (zero if j is not among them)."""
    b = np.zeros(len(free))
    b[free == j] = 1.0
    return b


def column(st, values, fixed, gauge, j, ridge=RIDGE, tol=TOL, max_iters=5000, precond="block", trace=None):
    """System (gauge, j) of nhip_bsr_pcg_columns_dev: (x (3 n_blocks,), iterations, relative residual, flag)."""
    A, free = cut(st, values, fixed, gauge, ridge)
    b = unit_rhs(free, j)
    x = np.zeros(3 * st.n_blocks)
    if not b.any():
        return x, 0, 0.0, 0
    xf, k, rel, flag = LR.pcg_matrix(A, b, tol, max_iters, precond, trace=trace)
    x[free] = xf
    return x, k, rel, flag


def column_iterates(st, values, fixed, gauge, j, k_max, ridge=RIDGE, longdouble=False):
    """[(x (3 n_blocks,), ||r|| / ||b||)] of system (gauge, j) with k = 0 .. k_max iterations complete (tol = 0)."""
    A, free = cut(st, values, fixed, gauge, ridge)
    b = unit_rhs(free, j)
    assert b.any(), "the right-hand side lies in a block that is not free"
    if longdouble:
        trace = LR.pcg_matrix_longdouble(A, b, k_max)
    else:
        trace = []
        LR.pcg_matrix(A, b, 0.0, k_max, trace=trace)
    out = []
    for xf, rel in trace:
        x = np.zeros(3 * st.n_blocks, dtype=xf.dtype)
        x[free] = xf
        out.append((x, rel))
    return out


def held_iterates(want, k_max=K_ITER):
    """The iterates k = 1 .. of a reference list that are held: while the iterate's own residual is above ITERATE_FLOOR."""
    ks = []
    for k in range(1, min(k_max, len(want) - 1) + 1):
        if not want[k][1] >= ITERATE_FLOOR:
            break
        ks.append(k)
    return ks


def true_relative_residual(st, values, fixed, gauge, j, x, ridge=RIDGE):
    """||e_j - A x|| / ||e_j|| over the free scalars of system (gauge, j), every product and sum in longdouble."""
    A, free = cut(st, values, fixed, gauge, ridge)
    A = A.tocoo()
    Ax = np.zeros(len(free), dtype=LR.LD)
    np.add.at(Ax, A.row, A.data.astype(LR.LD) * np.asarray(x, dtype=LR.LD)[free][A.col])
    b = unit_rhs(free, j).astype(LR.LD)
    return float(np.sqrt(np.sum((b - Ax) ** 2)) / np.sqrt(np.sum(b ** 2)))


# ------------------------------------------------------------------------------------------------ matrices
class Matrix:
    """A system of tests/linsolve_seams.py as ONE matrix for many systems: its structure, the assembled values (the
    reference assembly: the GPU tests upload these rows and assemble them on the device to the same bits), the shared mask
    and the batch list."""

    def __init__(self, name, system, mask, hub=None, isolated=0):
        self.name, self.s, self.st, self.nb, self.mask = name, system, system.st, system.nb, tuple(mask)
        self.values = LS.reference_assembly(system)[0]
        self.batch = batch_list(self.nb, self.mask, hub=hub, isolated=isolated)

    def column(self, gauge, j, **kw):
        return column(self.st, self.values, self.mask, gauge, j, **kw)


def batch_list(nb, mask, hub=None, isolated=0):
    """THE batch list of one matrix: [(gauge, rhs_index, what)].  `last` is the last block with rows (the `isolated` blocks
    behind it have none); the mask holds one block."""
    last, m = nb - 1 - isolated, mask[0]
    mid = last // 2 if last // 2 != m else last // 2 + 1

    def near(g, step):  # the nearest block with rows beside g, looking first in direction `step`, that is free
        return next(b for d in (step, -step, 2 * step, -2 * step) for b in [g + d] if 0 <= b <= last and b != m)
    out = [(-1, 0, "no gauge, first scalar row"),
           (-1, 3 * last + 2, "no gauge, last scalar row"),
           (0, 3 * near(0, 1), "gauge 0, next to it"),
           (0, 3 * last + 1, "gauge 0, far end"),
           (mid, 3 * near(mid, 1) + 1, "middle gauge, next to it"),
           (mid, 3 * near(mid, -1), "middle gauge, before it"),
           (mid, 0, "middle gauge, first scalar row"),
           (last, 3 * near(last, -1) + 2, "last gauge, next to it"),
           (last, 1, "last gauge, far end"),
           (mid, 3 * mid + 1, "right-hand side in the gauge block"),
           (-1, 3 * m, "right-hand side in a block of the mask"),
           (mid, 3 * near(mid, 1) + 1, "the middle gauge's neighbour once more: two identical systems")]
    if hub is not None:
        out += [(hub, 3 * (hub + 1) + 2, "a long hub as gauge, next to it"),
                (hub, 3 * hub, "a long hub as gauge, right-hand side in it"),
                (-1, 3 * hub + 1, "right-hand side in a long hub's free row")]
    if isolated:
        out += [(-1, 3 * (nb - 1) + 1, "right-hand side in an isolated block: one or two iterations"),
                (mid, 3 * (last + 1), "middle gauge, right-hand side in an isolated block")]
    return out


IDENTICAL = (4, 11)  # the two identical systems of every batch list
MASKED_RHS, GAUGE_RHS = 10, 9  # right-hand sides in blocks that are not free


@functools.lru_cache(maxsize=None)
def window_chain(nb, window):
    u, v = LR.chain_uv(nb, window)
    return LS.System("chain%dw%d" % (nb, window), nb, u, v, 100 * nb + window)


# name -> (what it reaches, builder).  The chains of linsolve_seams.CHAINS below its big ones are the row-tile and
# workgroup edges of nhip_linsolve.hip; 31 / 32 / 33 blocks are one block row short of this solver's tile of CB block rows,
# the tile, and one more (a second workgroup with ONE row); 86 = 2 tiles + 22, 256 = 8 tiles, 257 = 8 tiles + 1, hubs = 20.
# A chain's mask is block 0, the systems' own `fixed` (a mask inside a chain would cut it into parts, as a held line block
# does not cut a trajectory; the gauges cut it anyway, and the last block -- alone in its workgroup on chain33 and chain257 --
# stays free); there gauge 0 changes nothing and "first scalar row" lies in the mask.  hubs() masks a long hub, as the
# covariance caller masks the HITL line blocks, and its block 0 is free.
def _matrices():
    out = {"chain5w2": lambda: Matrix("chain5w2", window_chain(5, 2), (0,))}
    for nb in (CB - 1, CB, CB + 1, 86, 256, 257):
        out["chain%d" % nb] = (lambda nb=nb: Matrix("chain%d" % nb, LS.chain(nb), LS.chain(nb).fixed))
    out["chain40+3"] = lambda: Matrix("chain40+3", LS.chain(40, isolated=3), (0,), isolated=3)
    out["hubs"] = lambda: Matrix("hubs", LS.hubs(), (511,), hub=300)
    return out


MATRICES = tuple(_matrices())


@functools.lru_cache(maxsize=None)
def matrix(name):
    return _matrices()[name]()


N_SYSTEMS = (1, 2, CT - 1, CT, CT + 1, 2 * CT + 1)  # T - 1, T, T + 1, 2 T + 1 for T = 64 systems per workgroup


def cycle(batch, n):
    """n systems: the batch list repeated from its start."""
    return [batch[i % len(batch)] for i in range(n)]
