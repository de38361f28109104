"""The correspondence search at its pass, stage, bucket and path seams (nhip_corr.hip, K5: corr_search_kernel in both
instantiations, corr_scan_kernel, corr_compact_kernel): the blocks of tests/corr_seams.py through nhip_corr_search_dev and
nhip_corr_search_normals_dev (cos 20 deg), then nhip_corr_compact_dev, every byte against the CPU oracle's rows
(oracle.corr_search_batch / corr_search_gated_batch).  The padded rows behind every block's count and behind the last block,
and everything behind counts, block_offsets, the compacted rows and corr_block, must still hold the sentinel they were filled
with.  No tolerance anywhere.  Which seam each family crosses: tests/corr_seams.py; that each input is the case it claims to
be: tests/test_corr_seams_cpu.py."""
import ctypes as C

import numpy as np
import pytest

from nautilus_amd import _lib
from tests import corr_seams as S

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.25)
INT_SENTINEL = -99
TAIL = 64  # rows (or entries) of sentinel behind every output


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _status():
    info = (C.c_int32 * 4)()
    return _lib.load().nhip_dev_status(_stream(), info), list(info)


def _dev(a, dtype):
    """A device copy; an empty array still gets an address (the entry points refuse NULL)."""
    import torch
    a = np.array(a, dtype=dtype).reshape(-1)
    return torch.from_numpy(a).to("cuda:0") if a.size else torch.zeros(2, dtype=torch.from_numpy(np.zeros(1, dtype)).dtype, device="cuda:0")


def _first_difference(got, want, cap):
    row = int(np.nonzero((got.view(np.int32) != want.view(np.int32)).any(axis=1))[0][0])
    b = int(np.searchsorted(cap, row, side="right") - 1)
    return "first differing padded row %d: block %d, row %d of it: got %s want %s" % (row, b, row - cap[min(b, len(cap) - 1)], got[row], want[row])


def search_and_compact(case, gated):
    """One search launch and one compaction over all blocks of the case, into sentinel-filled buffers: host copies of
    (padded rows, counts, block_offsets, compacted rows, corr_block), each with its TAIL."""
    import torch
    lib = _lib.load()
    _, _, cap = S.expected(case.name, gated)
    nb, capacity = case.n_blocks, int(cap[-1])
    d_xy, d_nrm, d_off = _dev(case.xy, np.float32), _dev(case.nrm, np.float32), _dev(case.off, np.int32)
    d_bs, d_bt, d_aff, d_cap = _dev(case.bs, np.int32), _dev(case.bt, np.int32), _dev(case.aff, np.float32), _dev(cap, np.int64)
    f = lambda n: torch.full((n,), float(SENTINEL), dtype=torch.float32, device="cuda:0")
    i = lambda n: torch.full((n,), INT_SENTINEL, dtype=torch.int32, device="cuda:0")
    d_padded, d_counts = f(8 * (capacity + TAIL)), i(nb + TAIL)
    d_boff, d_corr, d_cblock = i(nb + 1 + TAIL), f(8 * (capacity + TAIL)), i(capacity + TAIL)
    head = (d_xy.data_ptr(), d_nrm.data_ptr(), d_off.data_ptr(), len(case.scans), d_bs.data_ptr(), d_bt.data_ptr(), nb, d_aff.data_ptr())
    out = (d_cap.data_ptr(), d_padded.data_ptr(), d_counts.data_ptr(), _stream())
    if gated:
        _lib.check(lib.nhip_corr_search_normals_dev(*head, case.thr, S.MIN_COS, *out))
    else:
        _lib.check(lib.nhip_corr_search_dev(*head, case.thr, *out))
    _lib.check(lib.nhip_corr_compact_dev(d_padded.data_ptr(), d_cap.data_ptr(), d_counts.data_ptr(), nb, d_boff.data_ptr(), d_corr.data_ptr(),
                                         d_cblock.data_ptr(), _stream()))
    torch.cuda.synchronize()
    return (d_padded.cpu().numpy().reshape(-1, 8), d_counts.cpu().numpy(), d_boff.cpu().numpy(), d_corr.cpu().numpy().reshape(-1, 8),
            d_cblock.cpu().numpy())


def assert_equals_the_oracle(case, gated):
    rows, counts, cap = S.expected(case.name, gated)
    boff, packed, cblock = S.compacted(case.name, gated)
    nb, capacity, n = case.n_blocks, int(cap[-1]), int(boff[-1])
    got_padded, got_counts, got_boff, got_corr, got_cblock = search_and_compact(case, gated)
    assert np.array_equal(got_counts[:nb], counts), "counts differ first at block %d" % np.nonzero(got_counts[:nb] != counts)[0][0]
    assert np.all(got_counts[nb:] == INT_SENTINEL)
    # every block's kept rows, and the sentinel in rows [counts[b], capacity_b) and behind the last block
    width = np.diff(cap)
    kept = (np.arange(capacity) - np.repeat(cap[:-1], width)) < np.repeat(counts, width)
    want_padded = np.full((capacity + TAIL, 8), SENTINEL, dtype=np.float32)
    want_padded[:capacity][kept] = rows[kept]
    assert got_padded.tobytes() == want_padded.tobytes(), _first_difference(got_padded, want_padded, cap)
    # the compaction
    assert np.array_equal(got_boff[:nb + 1], boff) and np.all(got_boff[nb + 1:] == INT_SENTINEL)
    assert got_corr[:n].tobytes() == packed.tobytes() and np.all(got_corr[n:].view(np.int32) == SENTINEL.view(np.int32))
    assert np.array_equal(got_cblock[:n], cblock) and np.all(got_cblock[n:] == INT_SENTINEL)
    assert _status() == (_lib.NHIP_OK, [0, 0, 0, 0])
    return nb, n


@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
def test_a_source_ladder_and_keep_masks(gpu, gated):
    """`for s0 = 0; s0 < ns; s0 += CT * MAX_PER_LANE`, `SRC_INDEX(k) < hi`, `__ballot(keep[k])`, `s_scan[k * (CT / 64) + wv]`,
    `pos += round_total`, `written = pos`: sources of 0 .. 4097 points whose kept rows are all, none, every other, a random
    half, or ONE row at the last lane of a wave (63), the first of the next (64), the last of a round (255), the first of the
    next (256), the last of a pass (2047), the first of the next (2048) and the last point."""
    nb, n = assert_equals_the_oracle(S.family_a(), gated)
    print("family a %s: %d blocks, %d rows equal" % ("gated" if gated else "plain", nb, n))


@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
def test_b_target_ladder(gpu, gated):
    """`nt <= TGT_CHUNK`, the staging rounds `i = tid + k * CT; if (i < nt)`, `s_sorted[slot] = (uint16_t)i`, and the exhaustive
    scan's `for t0 = 0; t0 < nt; t0 += TGT_CHUNK` with `idx = t0 + i`: targets of 0 .. 4097 points whose matched point is the
    last one, point 0, or the lower of two coincident points at 2047 | 2048, 4095 | 4096 or 0 | nt - 1 (a tie that went to
    the higher one would show in the row's target normal)."""
    nb, n = assert_equals_the_oracle(S.family_b(), gated)
    print("family b %s: %d blocks, %d rows equal" % ("gated" if gated else "plain", nb, n))


@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
@pytest.mark.parametrize("thr", S.C_THRESHOLDS)
def test_c_neighbour_cells_of_the_two_run_visit(gpu, thr, gated):
    """`two = (lo >> 2) != (hi2 >> 2)`, `cell_hash(lo, icy + oy)`, `b0 | 3u`, `b0 + 2u`, `group_hash(hi2 >> 2, icy + oy)` with
    `b0 + (hi2 & 3u)`, `cx >> 2` of negative cells: 90 queries at cell centres, cx = -5 .. 4, whose only target in reach lies
    in one designed cell of the nine."""
    nb, n = assert_equals_the_oracle(S.family_c(thr), gated)
    assert n == 90
    print("family c thr %g %s: %d block, %d rows equal" % (thr, "gated" if gated else "plain", nb, n))


@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
def test_d_bucket_extremes(gpu, gated):
    """`for i = s_start[b0]; i < e; i++` over ONE bucket that holds all 2,048 staged points (the counting sort's scan ends at
    `s_start[NB] = run` = 2048; `s_sorted[i] < s_sorted[bi[k]]` among coincident points at distance 0), and over 2,048 cells of
    one point each."""
    nb, n = assert_equals_the_oracle(S.family_d(), gated)
    print("family d %s: %d blocks, %d rows equal" % ("gated" if gated else "plain", nb, n))


@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
def test_e_path_switches(gpu, gated):
    """`scan_all = !hashed || __syncthreads_or(hashed ? big : 0)` decided pass by pass over a HASHED target: the scan then runs
    over s_tgt in bucket order with `idx = (int32_t)s_sorted[i]` and `(uint32_t)idx < (uint32_t)bi[k]` among four coincident
    targets at scattered indices; a block whose first pass scans and whose second walks, and the reverse, with `written`
    carried between them; a query at 3e7 that switches the path and matches nothing; `hashed = !__syncthreads_or(big)` for a
    target with one point beyond the limit."""
    nb, n = assert_equals_the_oracle(S.family_e(), gated)
    print("family e %s: %d blocks, %d rows equal" % ("gated" if gated else "plain", nb, n))


@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
def test_g_the_nearest_target_fails_the_gate(gpu, gated):
    """`ok = float_norm_root(d2) < thr && fabsf(dot2(...)) > min_cos` inside the walk: gated, the second nearest target is the
    match of every query; plain, the nearest."""
    c = S.family_g()
    nb, n = assert_equals_the_oracle(c, gated)
    assert n == S.G_SOURCES
    print("family g %s: %d block, %d rows equal" % ("gated" if gated else "plain", nb, n))


@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
@pytest.mark.parametrize("n_blocks", S.F_BLOCKS)
def test_f_block_count_ladder(gpu, n_blocks, gated):
    """corr_scan_kernel, `for base = 0; base < n_blocks; base += 1024`: one ragged step (1023), one full step (`s[1023]` is the
    total), a second step of one lane, two full steps, a third step, 2,500; `carry` across runs of blocks without rows on both
    sides of every seam and at both ends.  corr_compact_kernel with `n == 0`.  block_offsets, compacted rows, corr_block."""
    nb, n = assert_equals_the_oracle(S.family_f(n_blocks), gated)
    print("family f %s: %d blocks, %d rows equal" % ("gated" if gated else "plain", nb, n))
