"""The systems and helpers the seam tests of the device linear solver share (tests/test_linsolve_seams_cpu.py,
tests/test_linsolve_seams_gpu.py; DESIGN.md section 3, "Block-sparse system"; kernels nhip_linsolve.hip): systems sized to
the kernels' constants -- more than one workgroup, rows that straddle workgroups, many long rows of every length around the
thresholds, partial lists longer than a workgroup -- the iterate tolerance, the mutated references that show it has teeth,
and the checks every PCG system gets.  No device code here: the module imports on the CPU."""
import functools

import numpy as np

from nautilus_amd import linsolve
from tests import linsolve_reference as LR

LAM, FLOOR, TOL = 1e-3, 1e-9, 1e-10
LT, LONG_ROW, LONG_WGS = 256, 64, 8  # nhip_linsolve.hip's: threads per workgroup, the longest lane-owned row, long-row workgroups
K_ITER = 8                           # iterates 1 .. K_ITER are held to the reference

# The largest ||x_k(float64 reference) - x_k(longdouble restatement)|| / ||x_k|| and the largest relative difference of the
# recursive relative residual over k = 1 .. 8 on hubs(), chain(86) and chain(257) (tests/test_linsolve_seams_cpu.py measures
# and prints them): 1.72e-15 (the residual of hubs() at k = 8; 3.3e-16 for x), in ITERATE_MEASURED rounded up to two digits.
# ITERATE_TOL is that times 16: the device's three reduction shapes are the 256-lane LDS tree, the per-workgroup partials
# and the long-row deal; each orders sums differently from numpy, and the differences compound over 8 iterations; 16 is
# that allowance.  Measured against the reference at higher precision, never fitted to the kernels' output.
ITERATE_MEASURED = 1.8e-15
ITERATE_TOL = 16 * ITERATE_MEASURED


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ------------------------------------------------------------------------------------------------ systems
class System:
    """n_blocks, the (u, v) of the rows, the rows, the structure; `fixed` is the default fixed set."""

    def __init__(self, name, nb, u, v, seed, fixed=(0,)):
        self.name, self.nb, self.fixed = name, int(nb), tuple(fixed)
        self.u, self.v = np.asarray(u, dtype=np.int64), np.asarray(v, dtype=np.int64)
        self.rows = LR.random_rows(self.u, seed)
        self.st = linsolve.BlockStructure(self.nb, self.u, self.v)

    def row_lengths(self):
        return np.diff(self.st.row_ptr)


PAIR_ROWS = (63, 64, 65, 127, 128, 129, 511, 512, 513, 1025)


@functools.lru_cache(maxsize=None)
def pair(R):
    """2 blocks, R rows on (0, 1): the four stored blocks have contributor lists of R, the cost sums R terms."""
    return System("pair%d" % R, 2, np.zeros(R, dtype=np.int64), np.ones(R, dtype=np.int64), 1000 + R)


# nb: what it reaches (ga = ceil(3 nb / 256) workgroups over the scalar rows, gb = ceil(nb / 256) over the blocks)
CHAINS = {86: "ga = 2, block 85 straddles workgroups 0 and 1", 256: "gb = 1, exactly full", 257: "gb = 2, one live lane in the last",
          21846: "ga = 257: 265 partials of p.q, more than a workgroup", 65537: "gb = 257: r.r and r.z have more partials than a workgroup"}
BIG_CHAINS = (21846, 65537)


@functools.lru_cache(maxsize=None)
def chain(nb, isolated=0):
    """An odometry chain u = 0 .. nb - 2, v = u + 1, and `isolated` more blocks without a row behind it."""
    return System("chain%d" % nb + ("+%d" % isolated if isolated else ""), nb + isolated, np.arange(nb - 1), np.arange(1, nb), nb)


# hub block: the number of stored blocks of its row.  64 is the longest lane-owned row, 65 the shortest long one, 256 / 257
# one / two passes of the long row's deal over the lanes, 514 three; the indices sit on the long-row list builder's seams:
# 63 | 64 a wave edge, 255 | 256 and 511 | 512 chunk edges, 520 .. 612 in the last, partial chunk (612 is the last block).
HUB_ROWS = {10: 90, 63: 64, 64: 65, 100: 130, 200: 150, 255: 256, 256: 257, 300: 300, 400: 200, 511: 514, 512: 66, 520: 67, 600: 100,
            611: 80, 612: 70}
HUBS_NB = 613
LONG_HUBS = tuple(sorted(h for h, n in HUB_ROWS.items() if n > LONG_ROW))


@functools.lru_cache(maxsize=None)
def hubs():
    """A chain of 613 blocks in which the blocks of HUB_ROWS are tied to as many distinct plain blocks as their row needs,
    by rows (hub, other) and (other, hub) in turn."""
    rng = np.random.default_rng(613)
    u, v = list(range(HUBS_NB - 1)), list(range(1, HUBS_NB))
    plain = np.setdiff1d(np.arange(HUBS_NB), list(HUB_ROWS))
    for h, length in sorted(HUB_ROWS.items()):
        near = [b for b in (h - 1, h + 1) if 0 <= b < HUBS_NB]
        others = rng.choice(np.setdiff1d(plain, near), length - 1 - len(near), replace=False)
        for j, o in enumerate(others):
            u.append(h if j % 2 == 0 else int(o))
            v.append(int(o) if j % 2 == 0 else h)
    return System("hubs", HUBS_NB, u, v, 613)


def neighbours(st, b):
    cols = st.col[st.row_ptr[b]:st.row_ptr[b + 1]]
    return [int(c) for c in cols if c != b]


def hubs_fixed_sets():
    """The fixed sets of the hubs system: a long hub (three passes of its deal); block 0, a block that straddles workgroups,
    a hub, a neighbour in the middle of that hub's row and the last block (a hub in a workgroup's partial tail); everything
    but one long hub and its neighbours."""
    st = hubs().st
    near = neighbours(st, 300)
    keep = [64] + neighbours(st, 64)
    return {"long_hub": (511,), "several": (0, 85, 300, near[len(near) // 2], HUBS_NB - 1),
            "all_but_a_hub": tuple(b for b in range(HUBS_NB) if b not in keep)}


PCG_SYSTEMS = ("hubs", "chain86", "chain256", "chain257", "chain21846", "chain65537")


ASSEMBLY_SYSTEMS = tuple("pair%d" % R for R in PAIR_ROWS) + tuple("chain%d" % nb for nb in CHAINS) + ("hubs",)


def system(name):
    """The system of a name of PCG_SYSTEMS or ASSEMBLY_SYSTEMS (built on first use)."""
    return hubs() if name == "hubs" else pair(int(name[4:])) if name.startswith("pair") else chain(int(name[5:]))


# ------------------------------------------------------------------------------------------------ assembly of a chain
def assemble_short_lists(st, rows):
    """LR.assemble for a structure whose contributor lists have at most 2 entries (a chain), vectorised: the pinned sum of
    two terms is (+0.0 + t0) + (+0.0 + t1) with every other partial +0.0, and np.add.at into zeros forms (+0.0 + t0) + t1:
    the same bits, whatever the order (tests/test_linsolve_seams_cpu.py holds it to LR.assemble on chain(257))."""
    lens = np.diff(st.contrib_ptr)
    assert lens.max() <= 2
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 28)
    Q = LR.quadrants(rows)
    G = np.zeros((len(rows), 4, 3))
    G[:, 0], G[:, 3] = rows[:, 21:24], rows[:, 24:27]
    G = G.reshape(-1, 3)
    block = np.repeat(np.arange(st.nnzb), lens)
    values, grad = np.zeros((st.nnzb, 9)), np.zeros((st.n_blocks, 3))
    np.add.at(values, block, Q[st.contrib])
    on = (st.col == st.block_row)[block]
    np.add.at(grad, st.col[block[on]], G[st.contrib[on]])
    return values.reshape(-1, 3, 3), grad.ravel(), 0.5 * float(LR.pinned_sum(rows[:, 27]))


def reference_assembly(s):
    return assemble_short_lists(s.st, s.rows) if s.nb in BIG_CHAINS else LR.assemble(s.st, s.rows)


# ------------------------------------------------------------------------------------------------ iterates
def iterate_distance(got, want):
    """(||x - x_want|| / ||x_want||, |rel - rel_want| / rel_want) of two (x, relative residual), in longdouble."""
    x, w = np.asarray(got[0], dtype=LR.LD), np.asarray(want[0], dtype=LR.LD)
    rel, wrel = LR.LD(got[1]), LR.LD(want[1])
    return float(np.sqrt(np.sum((x - w) ** 2)) / np.sqrt(np.sum(w ** 2))), float(abs(rel - wrel) / wrel)


def worst_distance(got, want, ks=range(1, K_ITER + 1)):
    """The largest of both distances over the iterates `ks` of two lists indexed by k."""
    return max(max(iterate_distance(got[k], want[k])) for k in ks)


def mutated_iterates(s, values, grad, fixed, k_max, mutation=None, where=None):
    """LR.pcg_iterates(...) by a float64 copy of LR.pcg_matrix's loop that can be wrong in the ways a kernel could be
    (mutation None: the same bits as LR.pcg_iterates, which tests/test_linsolve_seams_cpu.py asserts):
      "pq_twice"   p . q counts the three scalars of block `where` twice (a long row summed by its lanes and by its workgroup)
      "rr_short"   r . r omits block `where` (a workgroup's partial dropped)
      "q_stale"    q of block `where` stays at its previous value (a long row nobody took)
      "unfixed"    the fixed block `where` takes part like a free one and its x is zeroed at the end (a fixed column
                   neighbour's p not skipped)"""
    st = s.st
    if mutation == "unfixed":
        fixed = [b for b in fixed if b != where]
    A, free = LR.damped(st, values, fixed, LAM, FLOOR)
    A = A.tocsr()
    b = -np.asarray(grad)[free]
    at = np.nonzero(np.isin(free // 3, [where]))[0] if where is not None else np.zeros(0, dtype=np.int64)
    assert mutation is None or len(at) == 3
    n = len(free)
    D = np.zeros((n // 3, 3, 3))
    blocks = A.tobsr(blocksize=(3, 3))
    rows_of = np.repeat(np.arange(n // 3), np.diff(blocks.indptr))
    on = blocks.indices == rows_of
    D[rows_of[on]] = blocks.data[on]
    Minv = np.linalg.inv(D)
    apply = lambda r: np.einsum("bij,bj->bi", Minv, r.reshape(-1, 3)).ravel()
    keep = np.ones(n, dtype=bool)
    keep[at] = False
    x, r = np.zeros(n), b.copy()
    z = apply(r)
    p, q, bb = np.zeros(n), np.zeros(n), float(b @ b)
    rr, rz, rz_old, out = bb, float(r @ z), 0.0, []
    for k in range(k_max + 1):
        beta = np.float64(rz) / np.float64(rz_old) if k > 0 else 0.0
        full = np.zeros(3 * st.n_blocks)
        full[free] = x
        if mutation == "unfixed":
            full[3 * where:3 * where + 3] = 0.0
        out.append((full, float(np.sqrt(rr) / np.sqrt(bb))))
        if k == k_max:
            break
        p = z.copy() if k == 0 else z + beta * p
        q_new = A @ p
        if mutation == "q_stale":
            q_new[at] = q[at]
        q = q_new
        pq = np.float64(p @ q)
        if mutation == "pq_twice":
            pq = pq + np.float64(p[at] @ q[at])
        alpha = np.float64(rz) / pq
        x = x + alpha * p
        r = r - alpha * q
        z = apply(r)
        rr = float(r[keep] @ r[keep]) if mutation == "rr_short" else float(r @ r)
        rz_old, rz = rz, float(r @ z)
    return out


# ------------------------------------------------------------------------------------------------ what every PCG system gets
def check_pcg(st, system, values, grad, fixed, what):
    """The residual, iteration-cap and fixed-block checks every PCG system gets.  Returns the reference's count."""
    x, res = system.solve(LAM, FLOOR, TOL, 5000)
    k_ref = LR.pcg(st, values, grad, fixed, LAM, FLOOR, TOL, 5000)[1]
    true = LR.true_relative_residual(st, values, grad, fixed, LAM, FLOOR, x)
    print("PCG %s: %r, k_ref %d (cap %d), true residual / tol %.3g" % (what, res, k_ref, LR.iteration_cap(k_ref), true / TOL))
    assert res.flag == 0 and res.relative_residual <= TOL
    assert true <= 10 * TOL
    assert res.iterations <= LR.iteration_cap(k_ref)
    for b in fixed:
        assert np.array_equal(bits(x[3 * b:3 * b + 3]), bits(np.zeros(3))), "x is exactly 0 on a fixed block"
    assert np.abs(x).max() > 0
    return k_ref


def check_iterates(st, system, values, grad, fixed, what, ks=range(1, K_ITER + 1)):
    """tol = 0 and max_iters = k for every k of `ks`: k iterations, flag 1, x and the relative residual within ITERATE_TOL
    of the reference's k-th iterate.  Returns the worst distance."""
    want = LR.pcg_iterates(st, values, grad, fixed, LAM, FLOOR, max(ks))
    worst = 0.0
    for k in ks:
        x, res = system.solve(LAM, FLOOR, 0.0, k)
        dx, drel = iterate_distance((x, res.relative_residual), want[k])
        print("ITERATE %s k %d: |dx| / |x| %.3g, d relres %.3g (of ITERATE_TOL: %.3g, %.3g)" % (
            what, k, dx, drel, dx / ITERATE_TOL, drel / ITERATE_TOL))
        assert (res.iterations, res.flag) == (k, 1)
        assert dx <= ITERATE_TOL and drel <= ITERATE_TOL
        for b in fixed:
            assert np.array_equal(bits(x[3 * b:3 * b + 3]), bits(np.zeros(3))), "x is exactly 0 on a fixed block"
        worst = max(worst, dx, drel)
    return worst
