"""Columns of gauged inverses on the GPU (kernels nhip_linsolve_columns.hip, host loop nhip_host_linsolve.hip; DESIGN.md
section 8 item 13): nhip_bsr_pcg_columns_dev through linsolve.DeviceSystem.inverse_columns and the raw C ABI, held to the
restatement of tests/covariance_reference.py (checked on the CPU by tests/test_covariance_cpu.py) -- its iterates, its
converged solves, its ends -- at the tile's edges in blocks and in systems; the independence of a system's bits from its
batch; isolation of gauged blocks; ids from device memory; sentinels behind what the kernels write; and
PoseGraph.cross_covariances(linear_solver="device") beside the host path."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from nautilus_amd import _lib, hostside, linsolve, posegraph
from tests import covariance_reference as CR
from tests import linsolve_reference as LR
from tests import linsolve_seams as LS
from tests.linsolve_seams import bits

pytestmark = pytest.mark.gpu

SENTINEL, WS_SENTINEL, PAD = -7.25, 0xA5, 256
BAD_SYSTEM_ID, BAD_BLOCK_COLUMN = 8192, 4096


@pytest.fixture(scope="module")
def backend(gpu):
    return posegraph.HipBackend()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@pytest.fixture(scope="module")
def systems(backend):
    """name -> the DeviceSystem of a matrix of CR.MATRICES, assembled on the device from the matrix's rows, its mask set."""
    cache = {}

    def get(name):
        if name not in cache:
            M = CR.matrix(name)
            system = backend.device_system(M.st, fixed=M.mask)
            system.assemble(_dev(M.s.rows))
            assert np.array_equal(bits(system.download()[0]), bits(M.values)), "the device assembles the reference's bits"
            cache[name] = system
        return cache[name]
    return get


@functools.lru_cache(maxsize=None)
def reference(name):
    """Per system of the batch list of a matrix: the converged restatement (x, k, rel, flag) and its iterates 0 .. 8 (None
    for a right-hand side in a block that is not free).  Computed once."""
    M = CR.matrix(name)
    out = []
    for g, j, _ in M.batch:
        conv = M.column(g, j)
        its = CR.column_iterates(M.st, M.values, M.mask, g, j, CR.K_ITER) if conv[1] else None
        out.append((conv, its))
    return out


def run(system, batch, **kw):
    """inverse_columns on [(gauge, rhs, ...)]: (x (3 n_blocks, S) on the host, [(iterations, flag, residual)])."""
    x, res = system.inverse_columns([b[0] for b in batch], [b[1] for b in batch], **kw)
    return x.cpu().numpy(), [(r.iterations, r.flag, r.relative_residual) for r in res]


def pick(batch, n, start=0):
    """n systems of a batch list, cyclically from `start`: ([(gauge, rhs, what)], their indices in the list)."""
    idx = [(start + i) % len(batch) for i in range(n)]
    return [batch[i] for i in idx], idx


def same(a, ia, b, ib):
    """system ia of result a and system ib of result b: the same bits of x, count, flag and residual."""
    return np.array_equal(bits(a[0][:, ia]), bits(b[0][:, ib])) and a[1][ia][:2] == b[1][ib][:2] and \
        np.array_equal(bits([a[1][ia][2]]), bits([b[1][ib][2]]))


def not_free(M, g):
    return sorted(set(M.mask) | ({g} if g >= 0 else set()))


# ------------------------------------------------------------------------------------------------ iterates
@pytest.mark.parametrize("name", CR.MATRICES)
def test_iterates_follow_the_restatement_at_every_batch_size(systems, name):
    """tol = 0, max_iters = k, k = 1 .. 8, at every n_systems around the 64-system tile: k iterations, flag 1, x and the
    relative residual within ITERATE_TOL_COLUMNS of the restatement's k-th iterate, on every system while its iterate is
    held (CR.held_iterates: above the floor under which the restatement itself is rounding noise)."""
    M, system, ref = CR.matrix(name), systems(name), reference(name)
    worst, seen = 0.0, set()
    for n in CR.N_SYSTEMS:
        batch, idx = pick(M.batch, n, start=3 * n)
        for k in range(1, CR.K_ITER + 1):
            x, res = run(system, batch, tol=0.0, max_iters=k)
            for c, i in enumerate(idx):
                conv, its = ref[i]
                for b in not_free(M, batch[c][0]):
                    assert np.array_equal(bits(x[3 * b:3 * b + 3, c]), bits(np.zeros(3))), "x is exactly 0 on a block that is not free"
                if its is None:
                    assert res[c] == (0, 0, 0.0) and not x[:, c].any()
                    continue
                if k not in CR.held_iterates(its):
                    continue
                dx, drel = LS.iterate_distance((x[:, c], res[c][2]), its[k])
                if max(dx, drel) > worst:
                    print("ITERATE %s n %d system %d %r k %d: |dx| / |x| %.3g, d relres %.3g (of the tolerance: %.3g, %.3g)" % (
                        name, n, i, M.batch[i][:2], k, dx, drel, dx / CR.ITERATE_TOL_COLUMNS, drel / CR.ITERATE_TOL_COLUMNS))
                    worst = max(dx, drel)
                assert res[c][:2] == (k, 1)
                assert dx <= CR.ITERATE_TOL_COLUMNS and drel <= CR.ITERATE_TOL_COLUMNS
                seen.add(i)
    print("ITERATE %s: worst distance %.3g = %.3g of ITERATE_TOL_COLUMNS" % (name, worst, worst / CR.ITERATE_TOL_COLUMNS))
    assert seen >= {i for i, (conv, its) in enumerate(ref) if its is not None and CR.held_iterates(its)}


# ------------------------------------------------------------------------------------------------ batch independence
@pytest.mark.parametrize("name", CR.MATRICES)
@pytest.mark.parametrize("kw", [dict(tol=CR.TOL), dict(tol=0.0, max_iters=5)], ids=["converged", "five_iterations"])
def test_a_systems_bits_do_not_depend_on_its_batch(systems, name, kw):
    M, system = CR.matrix(name), systems(name)
    L = len(M.batch)
    base = run(system, M.batch, **kw)
    for i in range(L):  # alone
        assert same(run(system, [M.batch[i]], **kw), 0, base, i), "system %d alone" % i
    for n in CR.N_SYSTEMS:  # every batch size, from another start
        batch, idx = pick(M.batch, n, start=n)
        got = run(system, batch, **kw)
        assert all(same(got, c, base, i) for c, i in enumerate(idx)), "n_systems %d" % n
    got = run(system, M.batch[::-1], **kw)  # reversed
    assert all(same(got, L - 1 - i, base, i) for i in range(L)), "reversed"
    got = run(system, [M.batch[1]] * 70 + list(M.batch) + [M.batch[3]] * 5, **kw)  # padded with copies
    assert all(same(got, 70 + i, base, i) for i in range(L)) and all(same(got, c, base, 1) for c in range(70)), "padded"
    one = linsolve_bytes(system, 1)  # chunked: three systems per call
    got = run(system, M.batch, max_bytes=3 * one, **kw)
    assert all(same(got, i, base, i) for i in range(L)), "chunked"
    for every in (1, 7, 1000):
        got = run(system, M.batch, check_every=every, **kw)
        assert all(same(got, i, base, i) for i in range(L)), "check_every %d" % every
    got = run(system, M.batch, **kw)  # once more
    assert all(same(got, i, base, i) for i in range(L)), "two runs"
    a, b = CR.IDENTICAL
    assert same(base, a, base, b), "two identical systems"


def linsolve_bytes(system, n):
    st = system.st
    return int(system.lib.nhip_bsr_pcg_columns_workspace_bytes(st.n_blocks, st.nnzb, n)) + 8 * 3 * st.n_blocks * n


# ------------------------------------------------------------------------------------------------ converged solves
@pytest.mark.parametrize("name", CR.MATRICES)
def test_converged_solves(systems, name):
    M, system, ref = CR.matrix(name), systems(name), reference(name)
    x, res = run(system, M.batch, tol=CR.TOL)
    for i, (g, j, what) in enumerate(M.batch):
        (xr, k_ref, rel_ref, flag_ref), its = ref[i]
        for b in not_free(M, g):
            assert np.array_equal(bits(x[3 * b:3 * b + 3, i]), bits(np.zeros(3))), "x is exactly 0 on a block that is not free"
        if its is None:
            assert res[i] == (0, 0, 0.0) and not x[:, i].any(), what
            continue
        true = CR.true_relative_residual(M.st, M.values, M.mask, g, j, x[:, i])
        print("COLUMN %s (%d, %d) %s: %r, k_ref %d (cap %d), true residual / tol %.3g, |x - x_ref| / |x_ref| %.3g" % (
            name, g, j, what, res[i], k_ref, LR.iteration_cap(k_ref), true / CR.TOL, np.linalg.norm(x[:, i] - xr) / np.linalg.norm(xr)))
        assert res[i][1] == 0 and res[i][2] <= CR.TOL
        assert true <= 10 * CR.TOL
        assert res[i][0] <= LR.iteration_cap(k_ref)
        assert np.abs(x[:, i]).max() > 0
    if name == "chain40+3":
        for i in (len(M.batch) - 2, len(M.batch) - 1):  # the right-hand sides in an isolated block end at once ...
            assert res[i][0] == ref[i][0][1] and res[i][0] in (1, 2)
        assert max(r[0] for r in res) >= 20  # ... while their neighbours in the batch run on


# ------------------------------------------------------------------------------------------------ ends
@pytest.mark.parametrize("name", ["chain5w2", "chain33", "hubs"])
def test_ends(backend, systems, name):
    M, system, ref = CR.matrix(name), systems(name), reference(name)
    zero_rhs = [its is None for _, its in ref]
    x, res = run(system, M.batch, tol=CR.TOL, max_iters=0)
    assert not x.any()
    assert all(r == ((0, 0, 0.0) if z else (0, 1, 1.0)) for r, z in zip(res, zero_rhs))
    _, conv = run(system, M.batch, tol=CR.TOL)
    k_conv = max(r[0] for r in conv)
    _, res = run(system, M.batch, tol=CR.TOL, max_iters=k_conv - 1)
    for r, c in zip(res, conv):
        assert r[:2] == ((k_conv - 1, 1) if c[0] == k_conv else (c[0], 0))
    # every block in the mask
    held = system.fixed
    system.set_fixed(range(M.nb))
    try:
        x, res = run(system, M.batch, tol=CR.TOL)
    finally:
        system.set_fixed(held)
    assert not x.any() and all(r == (0, 0, 0.0) for r in res)
    assert system.fixed == tuple(M.mask)
    with pytest.raises(ValueError):
        system.set_fixed([M.nb])
    with pytest.raises(ValueError):
        system.set_fixed([-1])
    assert system.fixed == tuple(M.mask)
    x, res = system.inverse_columns([], [])
    assert tuple(x.shape) == (3 * M.nb, 0) and res == []


# ------------------------------------------------------------------------------------------------ isolation
@pytest.mark.parametrize("name", ["chain86", "hubs"])
def test_a_gauged_block_is_never_read(systems, name):
    """Every stored block of block g's row and column overwritten with NaN, then g's diagonal block negated: no bit of the
    systems gauged at g changes; the others break down (NaN: all of them, at once) with a finite x."""
    M, system = CR.matrix(name), systems(name)
    st = M.st
    g = M.batch[4][0]  # the middle gauge
    zero_rhs = [its is None for _, its in reference(name)]
    base = run(system, M.batch, tol=CR.TOL)
    touched = np.nonzero((st.block_row == g) | (st.col == g))[0]
    diag = int(np.nonzero((st.block_row == g) & (st.col == g))[0][0])
    saved = system.d_values.clone()
    try:
        v = system.d_values.view(-1, 9)
        v[_dev(touched)] = float("nan")
        got = run(system, M.batch, tol=CR.TOL)
        for i, (gi, j, what) in enumerate(M.batch):
            if gi == g or zero_rhs[i]:
                assert same(got, i, base, i), what
            else:
                assert got[1][i][1] == 2 and np.isfinite(got[0][:, i]).all(), what
        system.d_values.copy_(saved)
        v[diag] = -v[diag]
        got = run(system, M.batch + [(-1, 3 * g + 1, "right-hand side in the negated block")], tol=CR.TOL)
        for i, (gi, j, what) in enumerate(M.batch):
            if gi == g:
                assert same(got, i, base, i), what
            assert np.isfinite(got[0][:, i]).all(), what
        assert got[1][-1][:2] == (0, 2) and not got[0][:, -1].any(), "p . q < 0 in the first iteration: x is untouched"
    finally:
        system.d_values.copy_(saved)
    assert all(same(run(system, M.batch, tol=CR.TOL), i, base, i) for i in range(len(M.batch)))


# ------------------------------------------------------------------------------------------------ the raw ABI
def raw(system, gauge, rhs, tol=CR.TOL, max_iters=5000, check_every=32, pad=True, ws_short=0, ws_offset=0, n_systems=None,
        ridge=CR.RIDGE):
    """nhip_bsr_pcg_columns_dev with PAD sentinels behind x and behind exactly the workspace's bytes:
    (rc, x (3 n_blocks, S), [(iterations, flag, residual)], status info, sentinels intact)."""
    import torch
    st, lib = system.st, system.lib
    S = len(gauge) if n_systems is None else n_systems
    n = 3 * st.n_blocks * len(gauge)
    ws_bytes = int(lib.nhip_bsr_pcg_columns_workspace_bytes(st.n_blocks, st.nnzb, len(gauge)))
    d_x = torch.full((n + PAD,), SENTINEL, dtype=torch.float64, device="cuda:0")
    d_ws = torch.full((ws_bytes + PAD + 16,), WS_SENTINEL, dtype=torch.uint8, device="cuda:0")
    assert d_ws.data_ptr() % 16 == 0
    d_g, d_r = _dev(np.asarray(gauge, dtype=np.int32)), _dev(np.asarray(rhs, dtype=np.int32))
    stats = (_lib.PcgStats * max(len(gauge), 1))()
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.nhip_bsr_pcg_columns_dev(system.d_row_ptr.data_ptr(), system.d_col.data_ptr(), system.d_values.data_ptr(),
                                      system.d_fixed.data_ptr(), st.n_blocks, st.nnzb, d_g.data_ptr(), d_r.data_ptr(), S,
                                      ridge, tol, max_iters, check_every, d_x.data_ptr(), d_ws.data_ptr() + ws_offset,
                                      ws_bytes - ws_short, stats, sp)
    info = (C.c_int32 * 4)()
    lib.nhip_dev_status(sp, info)
    intact = bool((d_x[n:] == SENTINEL).all()) and bool((d_ws[ws_bytes + ws_offset:] == WS_SENTINEL).all())
    x = d_x[:n].cpu().numpy().reshape(3 * st.n_blocks, len(gauge))
    return rc, x, [(s.iterations, s.flag, s.relative_residual) for s in stats][:len(gauge)], list(info), intact


@pytest.mark.parametrize("name", ["chain33", "chain257", "hubs"])
def test_nothing_is_written_behind_x_or_the_workspace(systems, name):
    M, system = CR.matrix(name), systems(name)
    g, r = [b[0] for b in M.batch], [b[1] for b in M.batch]
    base = run(system, M.batch, tol=CR.TOL)
    for n in (1, CR.CT - 1, CR.CT, CR.CT + 1):
        gg, rr = [g[i % len(g)] for i in range(n)], [r[i % len(r)] for i in range(n)]
        rc, x, res, info, intact = raw(system, gg, rr)  # converged
        assert rc == 0 and intact and info[0] == 0
        assert all(same((x, res), c, base, c % len(g)) for c in range(n))
        rc, x, res, info, intact = raw(system, gg, rr, tol=0.0, max_iters=3)  # flag 1
        assert rc == 0 and intact and all(f in (0, 1) for _, f, _ in res)
    saved = system.d_values.clone()
    try:
        system.d_values.view(-1, 9)[:] = float("nan")  # flag 2
        rc, x, res, info, intact = raw(system, g, r)
        zero_rhs = [its is None for _, its in reference(name)]
        assert rc == 0 and intact and all(r_ == (0, 0, 0.0) if z else r_[1] == 2 for r_, z in zip(res, zero_rhs))
        assert np.isfinite(x).all()
    finally:
        system.d_values.copy_(saved)


def test_ids_from_device_memory_are_checked(systems):
    M, system = CR.matrix("chain86"), systems("chain86")
    nb = M.nb
    g, r = [b[0] for b in M.batch], [b[1] for b in M.batch]
    base = run(system, M.batch, tol=CR.TOL)
    for bad_g, bad_r, value in ((nb, 3, nb), (-2, 3, -2), (1, -1, -1), (1, 3 * nb, 3 * nb), (2 ** 31 - 1, 0, 2 ** 31 - 1)):
        at = 5
        gg, rr = g[:at] + [bad_g] + g[at:], r[:at] + [bad_r] + r[at:]
        rc, x, res, info, intact = raw(system, gg, rr)
        assert rc == 0 and intact
        assert res[at] == (0, 2, 0.0) and not x[:, at].any()
        assert info[0] == BAD_SYSTEM_ID and info[1:] == [BAD_SYSTEM_ID, np.int32(value), at], info
        for i in range(len(g)):
            assert same((x, res), i + (i >= at), base, i)
    # every system bad
    rc, x, res, info, intact = raw(system, [nb] * 3, [0] * 3)
    assert rc == 0 and intact and not x.any() and res == [(0, 2, 0.0)] * 3 and info[0] == BAD_SYSTEM_ID
    with pytest.raises(_lib.NhipError, match="gauge or right-hand-side index"):
        system.inverse_columns([nb], [0])
    # a block column outside the blocks: reported, skipped, nothing faults
    saved = system.d_col.clone()
    try:
        k = int(M.st.row_ptr[41]) - 1  # the last stored block of row 40
        for bad in (nb + 5, -3):
            system.d_col[k] = bad
            rc, x, res, info, intact = raw(system, g, r, max_iters=200)
            assert rc == 0 and intact and info[0] == BAD_BLOCK_COLUMN and info[2:] == [bad, k], info
            assert np.isfinite(x).all()
    finally:
        system.d_col.copy_(saved)
    assert all(same(run(system, M.batch, tol=CR.TOL), i, base, i) for i in range(len(g)))


def test_argument_errors_have_codes_and_messages(systems):
    import torch
    system = systems("chain33")
    lib, st = system.lib, system.st
    g, r = [-1, 0], [3, 4]
    err = lambda: lib.nhip_last_error().decode()
    for kw, word in ((dict(tol=-1.0), "tol"), (dict(ridge=-1e-12), "ridge"), (dict(ridge=float("nan")), "ridge"),
                     (dict(ridge=float("inf")), "ridge"), (dict(max_iters=-1), "max_iters"), (dict(check_every=0), "check_every"),
                     (dict(ws_short=1), "workspace"), (dict(ws_offset=8), "aligned"), (dict(n_systems=-1), "size")):
        rc, x, res, info, intact = raw(system, g, r, **kw)
        assert rc == _lib.NHIP_ERR_ARG and word in err() and intact, (kw, err())
        assert np.all(x == SENTINEL)
    null = lambda **kw: lib.nhip_bsr_pcg_columns_dev(*[kw.get(k, 16) for k in ("row_ptr", "col", "values", "fixed")], st.n_blocks, st.nnzb,
                                                     kw.get("gauge", 16), kw.get("rhs", 16), 2, 1e-12, 1e-10, 10, 32, kw.get("x", 16),
                                                     kw.get("ws", 16), 1 << 40, kw.get("stats", (_lib.PcgStats * 2)()), None)
    for name in ("row_ptr", "col", "values", "fixed", "gauge", "rhs", "x", "ws", "stats"):
        assert null(**{name: None}) == _lib.NHIP_ERR_ARG and "null" in err(), name
    stats = (_lib.PcgStats * 2)()
    big = lambda nb, S: lib.nhip_bsr_pcg_columns_dev(16, 16, 16, 16, nb, 0, 16, 16, S, 1e-12, 1e-10, 10, 32, 16, 16, 1 << 40, stats, None)
    assert big((1 << 29) + 1, 1) == _lib.NHIP_ERR_ARG and "size" in err()
    assert big(1 << 29, 2) == _lib.NHIP_ERR_ARG and "2^31" in err()
    assert big(0, 2) == _lib.NHIP_OK and big(5, 0) == _lib.NHIP_OK  # nothing launched
    assert lib.nhip_bsr_pcg_columns_workspace_bytes(33, 97, 0) >= 256
    assert lib.nhip_bsr_pcg_columns_workspace_bytes(33, 97, 65) > lib.nhip_bsr_pcg_columns_workspace_bytes(33, 97, 64)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ cross_covariances
PAIRS = [(30, 5), (5, 30), (12, 13), (1, 39), (7, 0)]


def ulps32(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    def key(v):
        i = np.ascontiguousarray(v).view(np.int32).astype(np.int64)
        return np.where(i < 0, -2 ** 31 - i, i)
    return np.abs(key(a) - key(b))


def check_cross_covariances(pg, pairs, candidates, source):
    host64 = pg.cross_covariances(pairs, dtype=np.float64)
    for k in pg.linear_stats:
        pg.linear_stats[k] = 0
    dev64 = pg.cross_covariances(pairs, linear_solver="device", dtype=np.float64)
    stats = dict(pg.linear_stats)
    assert dev64.dtype == np.float64 and dev64.shape == (len(pairs), 2, 2)
    worst = 0.0
    for (s_, t_), h, d in zip(pairs, host64, dev64):
        if max(min(s_, t_) - 1, 0) in (s_, t_):
            assert not h.any() and np.array_equal(bits(d), bits(np.zeros((2, 2)))), "a gauge pair gives exact zeros"
            continue
        rel = np.abs(d - h).max() / np.abs(h).max()
        print("CROSS (%d, %d): device - host %.3g of the block's largest entry %.3g" % (s_, t_, rel, np.abs(h).max()))
        worst = max(worst, rel)
        assert rel <= 2.0 ** -24
    print("CROSS worst %.3g; covariance_stats %r; linear_stats %r" % (worst, pg.covariance_stats, stats))
    host32, dev32 = pg.cross_covariances(pairs), pg.cross_covariances(pairs, linear_solver="device")
    assert host32.dtype == dev32.dtype == np.float32
    assert np.array_equal(dev32.view(np.int32), dev64.astype(np.float32).view(np.int32))
    assert ulps32(host32, dev32).max() <= 1
    assert all(f == 0 for f in pg.covariance_stats["flags"]) and pg.covariance_stats["systems"] == len(pg.covariance_stats["flags"])
    assert stats["solves"] == pg.covariance_stats["systems"] and stats["not_converged"] == stats["breakdowns"] == 0
    assert stats["iterations"] == sum(pg.covariance_stats["iterations"]) > 0
    device_fn = lambda p: pg.cross_covariances(p, linear_solver="device")
    for be in (None, pg.backend):
        assert hostside.lc_possible_matches(source, candidates, pg.poses, device_fn, backend=be) == \
            hostside.lc_possible_matches(source, candidates, pg.poses, pg.cross_covariances, backend=be)
    return dev64


def test_cross_covariances_on_the_device_beside_the_host_path(backend):
    """The graph of test_cross_covariance_blocks_match_dense_inverse (40 scans, window 3, solved 3 iterations), its five pairs."""
    from nautilus_amd import csm, synth
    bag = synth.SynthBag(40, dense=True)
    xy, off = csm.pack_scans(bag.scans)
    nrm = np.concatenate(bag.normals).astype(np.float32)
    pg = posegraph.PoseGraph(xy, nrm, off, bag.odom, window=3, kind=_lib.NHIP_LIDAR_NORMAL, backend=backend)
    pg.solve(iterations=3)
    check_cross_covariances(pg, PAIRS, [5, 12, 30, 39], 30)
    # two systems per distinct (gauge, target): (30, 5) and (5, 30) share a gauge but not a target; duplicates are solved once
    pg.cross_covariances(PAIRS + PAIRS + [(31, 5)], linear_solver="device")
    assert pg.covariance_stats["systems"] == 2 * 4
    assert not pg.cross_covariances([(7, 0), (0, 3)], linear_solver="device").any() and pg.covariance_stats["systems"] == 0
    assert pg._device_system().fixed == (0,)
    with pytest.raises(ValueError):
        pg.cross_covariances([(40, 1)], linear_solver="device")


def test_cross_covariances_with_a_loop_closure_and_a_line_block(backend):
    """The 48-scan window-10 graph with a loop closure and a device HITL constraint: the line block is held constant, pose 0
    is not; every system converges; the mask is back afterwards -- a following solve gives the bits it gives without."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import slam_loop
    from nautilus_amd import csm, synth
    bag = synth.SynthBag(48, dense=True)
    xy, off = csm.pack_scans(bag.scans)
    nrm = np.concatenate(bag.normals).astype(np.float32)
    start = np.array(bag.odom, dtype=np.float64)
    pg = posegraph.PoseGraph(xy, nrm, off, bag.odom, window=10, kind=_lib.NHIP_LIDAR_NORMAL, backend=backend)
    pg.add_loop_closures([47], [0], [bag.true_relative(47, 0)])
    lines = hostside.hitl_segments(slam_loop.synthetic_hitl_message(bag, start, 2, 45))
    con = backend.hitl_select(xy, off, start, lines[0], lines[1])
    pg.add_hitl(con)

    def solve():
        pg.poses, con.chosen_line_pose = start.copy(), np.zeros(3)
        return pg.solve(iterations=2, linear_solver="device")[0], con.chosen_line_pose.copy()
    without = solve()
    pg.poses, con.chosen_line_pose = start.copy(), np.zeros(3)
    pairs = [(30, 5), (5, 30), (12, 13), (1, 47), (7, 0), (47, 2)]
    check_cross_covariances(pg, pairs, [5, 12, 30, 47], 30)
    system = pg._device_system()
    assert system.fixed == (0,), "the mask is restored"
    held = system.fixed
    # pose 0 was free and the line block held during the call: gauge 4's column at pose 0 is not zero
    system.set_fixed([pg.n])
    try:
        x, res = system.inverse_columns([4], [3 * 30])
        x = x.cpu().numpy()
        assert res[0].flag == 0 and np.abs(x[:3, 0]).max() > 0 and not x[3 * pg.n:, 0].any() and not x[12:15, 0].any()
    finally:
        system.set_fixed(held)
    after = solve()
    assert np.array_equal(bits(after[0]), bits(without[0])) and np.array_equal(bits(after[1]), bits(without[1]))


# ------------------------------------------------------------------------------------------------ the example's gate
def test_the_examples_chi_square_gate_keeps_the_same_pairs_on_both_solvers(backend):
    """examples/slam_loop.py --lc-gate chi-square at test size (the loop of test_same_loop_on_the_cpu_backend_agrees): LCMatcher's
    walk with the covariance blocks from the host path and from the device path keeps the same pairs; the default gate's
    output has none of the new keys."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import slam_loop
    kw = dict(n_scans=200, window=3, min_scatter_score=0.3, cell_bits=8, spacing=0.4, hitl=False, backend=backend)
    plain = slam_loop.run(**kw)
    assert not any(k.startswith("lc_gate") for k in plain) and "lc_gate" not in plain["pcg_by_phase"]
    kept = []
    for max_score in (5000.0, 1e5, 1e7):  # LCMatcher's threshold, and two that keep pairs of this tightly pinned room
        host = slam_loop.run(lc_gate="chi-square", lc_max_score=max_score, **kw)
        dev = slam_loop.run(lc_gate="chi-square", lc_max_score=max_score, linear_solver="device", **kw)
        print("GATE at %g: geometric %d pairs; chi-square host %r; device %r" % (
            max_score, plain["lc_candidates"], {k: v for k, v in host.items() if k.startswith("lc_")},
            {k: v for k, v in dev.items() if k.startswith("lc_")}))
        for out in (host, dev):
            assert out["lc_gate"] == "chi-square" and out["lc_gate_s"] > 0 and out["lc_gate_max_score"] == max_score
            assert out["lc_gate_pairs"] == out["lc_candidates"]
            assert out["lc_gate_pairs_walked"] == out["lc_candidate_scans"] * (out["lc_candidate_scans"] - 1)
        assert host["lc_gate_pairs"] == dev["lc_gate_pairs"] and host.get("lc_accepted") == dev.get("lc_accepted")
        assert "lc_gate_pcg" not in host and host["pcg_by_phase"]["lc_gate"] == [0, 0]
        pcg = dev["lc_gate_pcg"]
        assert pcg["systems"] == dev["pcg_by_phase"]["lc_gate"][0] > 0 and pcg["not_converged"] == 0
        assert pcg["iterations_min_median_max"][0] > 0 and len(pcg["us_per_iteration_per_batch"]) == pcg["batches"] >= 1
        kept.append(dev["lc_gate_pairs"])
    assert kept == sorted(kept) and kept[-1] > 0, "a higher threshold keeps no fewer pairs, and the highest keeps some"
    with pytest.raises(ValueError):
        slam_loop.run(lc_gate="covariance", **kw)
