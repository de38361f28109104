"""The device linear solver at its workgroup and long-row seams (kernels nhip_linsolve.hip, host loop
nhip_host_linsolve.hip; DESIGN.md section 3, "Block-sparse system"): the assembly bit for bit at contributor lists around 64,
128 and the cost wave's 512-row trip, the PCG held to the reference's ITERATES (tests/linsolve_seams.py: ITERATE_TOL, from
the reference's own distance to a longdouble restatement) on systems with more than one workgroup, rows that straddle
workgroups, partial lists longer than a workgroup and fourteen long rows of every length around the thresholds; fixed
blocks anywhere, an isolated block, the host loop at the edges of max_iters and check_every, and sentinels behind every
buffer the kernels write.  The systems and the reference are checked on the CPU by tests/test_linsolve_seams_cpu.py."""
import ctypes as C

import numpy as np
import pytest

from nautilus_amd import _lib, posegraph
from tests import linsolve_seams as S
from tests.linsolve_seams import FLOOR, LAM, TOL, bits

pytestmark = pytest.mark.gpu

SENTINEL, WS_SENTINEL, PAD = -7.25, 0xA5, 256


@pytest.fixture(scope="module")
def backend(gpu):
    return posegraph.HipBackend()


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).to("cuda:0")


def _ok():
    import torch
    info = (C.c_int32 * 4)()
    return _lib.load().nhip_dev_status(C.c_void_p(torch.cuda.current_stream().cuda_stream), info) == _lib.NHIP_OK


def padded_system(backend, st, fixed):
    """A DeviceSystem whose values, gradient, x and workspace have PAD sentinels behind exactly 9 nnzb, 3 n_blocks, 3 n_blocks
    doubles and nhip_bsr_pcg_workspace_bytes bytes (fresh allocations: their bases are aligned like the ones they replace)."""
    import torch
    system = backend.device_system(st, fixed=fixed)
    full = lambda n: torch.full((n + PAD,), SENTINEL, dtype=torch.float64, device="cuda:0")
    system.d_values, system.d_grad, system.d_x = full(9 * st.nnzb), full(3 * st.n_blocks), full(3 * st.n_blocks)
    system.d_ws = torch.full((system.ws_bytes + PAD,), WS_SENTINEL, dtype=torch.uint8, device="cuda:0")
    assert system.d_ws.data_ptr() % 16 == 0
    return system


def assert_sentinels(system, what):
    st = system.st
    for name, t, n, want in (("values", system.d_values, 9 * st.nnzb, SENTINEL), ("grad", system.d_grad, 3 * st.n_blocks, SENTINEL),
                             ("x", system.d_x, 3 * st.n_blocks, SENTINEL), ("workspace", system.d_ws, system.ws_bytes, WS_SENTINEL)):
        tail = t[n:].cpu().numpy()
        assert len(tail) == PAD and np.all(tail == want), "%s: the sentinels behind %s" % (what, name)


class Case:
    """A system assembled on the device: its structure, padded DeviceSystem and the device's own values and gradient."""

    def __init__(self, backend, s):
        self.s, self.st = s, s.st
        self.system = padded_system(backend, s.st, s.fixed)
        self.cost = self.system.assemble(_dev(s.rows))
        self.values, self.grad, cost = self.system.download()
        assert cost == self.cost


@pytest.fixture(scope="module")
def cases(backend):
    cache = {}

    def get(s):
        if s.name not in cache:
            cache[s.name] = Case(backend, s)
        return cache[s.name]
    return get


def same_result(a, b):
    return np.array_equal(bits(a[0]), bits(b[0])) and (a[1].iterations, a[1].flag, a[1].relative_residual) == (
        b[1].iterations, b[1].flag, b[1].relative_residual)


# ------------------------------------------------------------------------------------------------ assembly
@pytest.mark.parametrize("name", S.ASSEMBLY_SYSTEMS)
def test_assembly_is_bit_equal_at_the_list_and_cost_wave_seams(cases, name):
    s = S.system(name)
    c = cases(s)
    want_v, want_g, want_c = S.reference_assembly(s)
    lens = np.diff(s.st.contrib_ptr)
    print("ASSEMBLE %s: %d blocks, %d rows, contributor lists up to %d, cost %.17g" % (s.name, s.st.nnzb, s.st.n_rows, lens.max(), c.cost))
    assert np.array_equal(bits(c.values), bits(want_v)) and np.array_equal(bits(c.grad), bits(want_g))
    assert bits(c.cost) == bits(want_c) and c.cost > 0 and np.abs(want_v).max() > 0
    if s.name.startswith("pair"):
        assert np.all(lens == s.st.n_rows)
    assert_sentinels(c.system, "the first assembly")
    cost_b = c.system.assemble(_dev(s.rows))
    values_b, grad_b, _ = c.system.download()
    assert np.array_equal(bits(values_b), bits(c.values)) and np.array_equal(bits(grad_b), bits(c.grad)) and bits(cost_b) == bits(c.cost)
    assert_sentinels(c.system, "the second assembly")
    assert _ok()


# ------------------------------------------------------------------------------------------------ iterates, convergence
@pytest.mark.parametrize("name", S.PCG_SYSTEMS)
def test_pcg_iterates_follow_the_reference(cases, name):
    c = cases(S.system(name))
    ks = (1, 2, S.K_ITER) if c.s.nb in S.BIG_CHAINS else range(1, S.K_ITER + 1)
    worst = S.check_iterates(c.st, c.system, c.values, c.grad, c.s.fixed, name, ks)
    print("ITERATES %s: worst %.3g = %.3g ITERATE_TOL" % (name, worst, worst / S.ITERATE_TOL))
    assert_sentinels(c.system, name)
    assert _ok()


@pytest.mark.parametrize("name", S.PCG_SYSTEMS)
def test_pcg_converges_within_the_references_cap(cases, name):
    c = cases(S.system(name))
    assert S.check_pcg(c.st, c.system, c.values, c.grad, c.s.fixed, name) > S.K_ITER
    assert_sentinels(c.system, name)
    assert _ok()


# ------------------------------------------------------------------------------------------------ fixed blocks
@pytest.mark.parametrize("which", ["long_hub", "several", "all_but_a_hub"])
def test_fixed_blocks_anywhere(cases, which):
    c = cases(S.hubs())
    st, system = c.st, c.system
    fixed = S.hubs_fixed_sets()[which]
    system.set_fixed(fixed)
    try:
        S.check_iterates(st, system, c.values, c.grad, fixed, "hubs, fixed " + which)
        S.check_pcg(st, system, c.values, c.grad, fixed, "hubs, fixed " + which)
        if which == "long_hub":
            # rows and columns of fixed blocks are skipped: nothing stored in them reaches the solve, not even a NaN
            h = fixed[0]
            clean = system.solve(LAM, FLOOR, TOL, 5000)
            k = np.nonzero((st.block_row == h) | (st.col == h))[0]
            assert len(k) == 2 * S.HUB_ROWS[h] - 1
            at = _dev((9 * k[:, None] + np.arange(9)).ravel())
            saved_v, saved_g = system.d_values.clone(), system.d_grad.clone()
            system.d_values[at] = float("nan")
            system.d_grad[3 * h:3 * h + 3] = float("nan")
            try:
                poisoned = system.solve(LAM, FLOOR, TOL, 5000)
            finally:
                system.d_values.copy_(saved_v)
                system.d_grad.copy_(saved_g)
            print("fixed long hub %d with NaN in its %d stored blocks: %r (clean %r)" % (h, len(k), poisoned[1], clean[1]))
            assert same_result(poisoned, clean)
    finally:
        system.set_fixed(c.s.fixed)
    assert_sentinels(system, which)
    assert _ok()


def test_all_blocks_fixed(cases):
    c = cases(S.chain(257))
    c.system.set_fixed(range(257))
    try:
        x, res = c.system.solve(LAM, FLOOR, TOL, 5000)
    finally:
        c.system.set_fixed(c.s.fixed)
    assert (res.iterations, res.flag, res.relative_residual) == (0, 0, 0.0)
    assert np.array_equal(bits(x), bits(np.zeros(3 * 257)))
    assert_sentinels(c.system, "all fixed")
    assert _ok()


# ------------------------------------------------------------------------------------------------ an isolated block
def test_an_isolated_free_block(cases):
    """Block 257 has a diagonal block without contributors and no gradient.  Damped, its diagonal block is
    lam * diag_floor * I and the solve leaves its x at 0.  With lam = 0 and diag_floor = 0 the block is singular: its inverse
    is not finite, z = M^-1 r is NaN on it, r.z is not finite -- the header's breakdown by a non-finite scalar, found with 0
    iterations complete: flag 2, and x the last iterate, the zeros of the start (np.linalg.inv raises on such a block, so
    this expectation is stated here and not taken from the reference)."""
    c = cases(S.chain(257, isolated=1))
    st = c.st
    assert st.n_blocks == 258 and not c.values[-1].any() and not c.grad[3 * 257:].any()
    S.check_pcg(st, c.system, c.values, c.grad, c.s.fixed, "chain257 and an isolated block")
    S.check_iterates(st, c.system, c.values, c.grad, c.s.fixed, "chain257 and an isolated block", (1, S.K_ITER))
    x, res = c.system.solve(LAM, FLOOR, TOL, 5000)
    assert res.flag == 0 and np.all(x[3 * 257:] == 0.0) and np.abs(x[3:3 * 257]).min() > 0
    x, res = c.system.solve(0.0, 0.0, TOL, 5000)
    print("isolated block, lam = 0, diag_floor = 0: %r" % res)
    assert (res.iterations, res.flag, res.relative_residual) == (0, 2, 1.0)
    assert np.array_equal(bits(x), bits(np.zeros(3 * 258)))
    assert_sentinels(c.system, "isolated")
    assert _ok()


# ------------------------------------------------------------------------------------------------ the host loop
def test_host_loop_at_the_edges_of_max_iters_and_check_every(cases):
    c = cases(S.chain(257))
    solve = lambda max_iters, **kw: c.system.solve(LAM, FLOOR, TOL, max_iters, **kw)
    full = solve(5000)
    k_conv = full[1].iterations
    print("HOST LOOP: k_conv %d, %r" % (k_conv, full[1]))
    assert full[1].flag == 0 and k_conv > 33, "more than one batch at the default check_every"
    x, res = solve(0)
    assert (res.iterations, res.flag, res.relative_residual) == (0, 1, 1.0) and np.array_equal(bits(x), bits(np.zeros(3 * 257)))
    x, res = solve(k_conv - 1)
    assert (res.iterations, res.flag) == (k_conv - 1, 1) and res.relative_residual > TOL
    at = solve(k_conv)  # the closing check tests convergence before it reports the cap
    assert (at[1].iterations, at[1].flag) == (k_conv, 0) and same_result(at, full)
    assert same_result(solve(k_conv + 1), full)
    for every in (1, k_conv - 1, k_conv, k_conv + 1, 5000):
        assert same_result(solve(5000, check_every=every), full), "check_every %d" % every
    assert same_result(solve(k_conv, check_every=k_conv), full)
    assert_sentinels(c.system, "host loop")
    assert _ok()


# ------------------------------------------------------------------------------------------------ bounds and reuse
@pytest.mark.parametrize("name, block", [("hubs", 511), ("chain257", 128)])
def test_solves_stay_inside_their_buffers_and_leave_nothing_behind(cases, name, block):
    c = cases(S.system(name))
    st, system = c.st, c.system
    first = system.solve(LAM, FLOOR, TOL, 5000)
    assert first[1].flag == 0
    assert_sentinels(system, "a converged solve")
    x, res = system.solve(LAM, FLOOR, TOL, 3)
    assert (res.iterations, res.flag) == (3, 1)
    assert_sentinels(system, "a flag-1 solve")
    k = int(np.nonzero((st.block_row == block) & (st.col == block))[0][0])
    system.d_values[9 * k:9 * k + 9] *= -1.0  # one negated diagonal block: p^T A p <= 0
    try:
        x, res = system.solve(LAM, FLOOR, TOL, 5000)
    finally:
        system.d_values[9 * k:9 * k + 9] *= -1.0
    print("BOUNDS %s, diagonal block %d negated: %r" % (name, block, res))
    assert res.flag == 2 and np.isfinite(x).all()
    assert_sentinels(system, "a flag-2 solve")
    assert same_result(system.solve(LAM, FLOOR, TOL, 5000), first), "the set-up resets the end words"
    assert_sentinels(system, "the solve behind it")
    assert _ok()


def test_two_solves_of_the_largest_chain_have_the_same_bits(cases):
    c = cases(S.chain(65537))
    a, b = c.system.solve(LAM, FLOOR, TOL, 5000), c.system.solve(LAM, FLOOR, TOL, 5000)
    print("chain65537 twice: %r" % a[1])
    assert a[1].flag == 0 and same_result(a, b)
    assert_sentinels(c.system, "chain65537")
    assert _ok()
