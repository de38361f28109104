"""The pose graph's linear system on the device ("Block-sparse system"; kernels nhip_linsolve.hip, K11).

  BlockStructure   the block-sparse pattern of a graph, built ONCE per graph on the host in numpy from the (u, v) unknown
                   blocks of its 28-double rows: what nhip_bsr_assemble_dev and nhip_bsr_pcg_dev take
  DeviceSystem     the device arrays of one structure -- values, gradient, x, the PCG workspace -- and the calls: assemble,
                   solve, and inverse_columns (many unit right-hand sides on the assembled matrix, each system with a gauge
                   block of its own: nhip_bsr_pcg_columns_dev)  (HipBackend.device_system makes one)

Unknown blocks are 3 wide.  Row r couples blocks u[r] != v[r]; its 6 x 6 is ordered [u | v] and lands in four stored
blocks: quadrant 0 in (u, u), 1 in (u, v), 2 (= 1 transposed) in (v, u), 3 in (v, v).  The full symmetric pattern is stored,
so the matrix-vector product needs no transposed pass.
"""
import ctypes as C
import time

import numpy as np

from . import _lib
from ._lib import check


class BlockStructure:
    """row_ptr (n_blocks + 1), col (nnzb; ascending within a block row, the diagonal block always present), contrib_ptr
    (nnzb + 1), contrib (entries 4 r + q, ascending within a block): all int32."""

    def __init__(self, n_blocks, u, v):
        nb = int(n_blocks)
        u, v = np.asarray(u, dtype=np.int64).ravel(), np.asarray(v, dtype=np.int64).ravel()
        if len(u) != len(v):
            raise ValueError("BlockStructure: %d u for %d v" % (len(u), len(v)))
        if nb < 0 or 4 * len(u) >= 2 ** 31:
            raise ValueError("BlockStructure: bad size")
        if len(u) and (min(u.min(), v.min()) < 0 or max(u.max(), v.max()) >= nb or np.any(u == v)):
            raise ValueError("BlockStructure: every row couples two different blocks of [0, %d)" % nb)
        self.n_blocks, self.n_rows, self.u, self.v = nb, len(u), u, v
        # every (block row, block column, contributor), and one entry without a contributor per diagonal block
        br, bc = np.stack([u, u, v, v], axis=1).ravel(), np.stack([u, v, u, v], axis=1).ravel()
        key = np.concatenate([br * nb + bc, np.arange(nb, dtype=np.int64) * (nb + 1)])
        cid = np.concatenate([np.arange(4 * len(u), dtype=np.int64), np.full(nb, -1, dtype=np.int64)])
        order = np.lexsort((cid, key))
        key, cid = key[order], cid[order]
        first = np.ones(len(key), dtype=bool)
        first[1:] = key[1:] != key[:-1]
        blocks = key[first]
        self.nnzb = len(blocks)
        self.block_row = (blocks // max(nb, 1)).astype(np.int32)
        self.col = (blocks % max(nb, 1)).astype(np.int32)
        self.row_ptr = np.searchsorted(self.block_row, np.arange(nb + 1)).astype(np.int32)
        real = cid >= 0
        self.contrib = cid[real].astype(np.int32)
        counts = np.bincount((np.cumsum(first) - 1)[real], minlength=self.nnzb)
        self.contrib_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        self.n_contrib = len(self.contrib)

    def to_scipy(self, values):
        """The stored blocks (nnzb, 3, 3) or (9 nnzb,) as a scipy.sparse CSC matrix of 3 n_blocks rows."""
        import scipy.sparse as sp
        n = 3 * self.n_blocks
        data = np.asarray(values, dtype=np.float64).reshape(self.nnzb, 3, 3)
        return sp.bsr_matrix((data, self.col, self.row_ptr), shape=(n, n)).tocsc()


class PcgResult:
    def __init__(self, iterations, flag, relative_residual):
        self.iterations, self.flag, self.relative_residual = int(iterations), int(flag), float(relative_residual)

    def __repr__(self):
        return "PcgResult(iterations=%d, flag=%d, relative_residual=%.3g)" % (self.iterations, self.flag, self.relative_residual)


class DeviceSystem:
    """values (9 nnzb), grad (3 n_blocks), x (3 n_blocks), cost (1), fixed (n_blocks, uint8) and the PCG workspace of one
    BlockStructure on the device; torch tensors are only the allocator."""

    def __init__(self, backend, structure, fixed=()):
        torch, st = backend.torch, structure
        self.torch, self.dev, self.lib, self.st = torch, backend.dev, backend.lib, st
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev) if len(a) else torch.zeros(1, dtype=torch.int32, device=self.dev)
        self.d_row_ptr, self.d_col, self.d_contrib_ptr, self.d_contrib = up(st.row_ptr), up(st.col), up(st.contrib_ptr), up(st.contrib)
        e = lambda n, dt: torch.empty(max(int(n), 1), dtype=dt, device=self.dev)
        self.d_values, self.d_grad, self.d_x, self.d_cost = e(9 * st.nnzb, torch.float64), e(3 * st.n_blocks, torch.float64), \
            e(3 * st.n_blocks, torch.float64), e(1, torch.float64)
        self.ws_bytes = int(self.lib.nhip_bsr_pcg_workspace_bytes(st.n_blocks, st.nnzb))
        self.d_ws = e(self.ws_bytes, torch.uint8)
        self.set_fixed(fixed)

    def set_fixed(self, blocks):
        """The blocks held constant by solve and inverse_columns from now on (ValueError for a block outside the structure)."""
        blocks = np.asarray(list(blocks), dtype=np.int64).reshape(-1)
        if len(blocks) and (blocks.min() < 0 or blocks.max() >= self.st.n_blocks):
            raise ValueError("set_fixed: block %d outside [0, %d)" % (
                blocks[(blocks < 0) | (blocks >= self.st.n_blocks)][0], self.st.n_blocks))
        mask = np.zeros(max(self.st.n_blocks, 1), dtype=np.uint8)
        mask[blocks] = 1
        self._fixed = tuple(int(b) for b in np.nonzero(mask[:self.st.n_blocks])[0])
        self.d_fixed = self.torch.from_numpy(mask).to(self.dev)

    @property
    def fixed(self):
        """The blocks of the current mask, ascending (what set_fixed takes back)."""
        return self._fixed

    def _max_iters(self, max_iters):  # solve's and inverse_columns' cap on the PCG's iterations
        return max(200, 3 * self.st.n_blocks) if max_iters is None else int(max_iters)

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.dev).cuda_stream)

    def assemble(self, d_rows, sync=True):
        """values, grad and cost from the (n_rows, 28) float64 device tensor `d_rows`; returns the cost (one double comes
        down; the ids the kernels read from device memory are checked there: nhip_dev_status)."""
        st = self.st
        if d_rows.shape[0] != st.n_rows or d_rows.dtype != self.torch.float64 or not d_rows.is_contiguous():
            raise ValueError("assemble: rows must be a contiguous (%d, 28) float64 tensor" % st.n_rows)
        sp = self._stream()
        check(self.lib.nhip_bsr_assemble_dev(d_rows.data_ptr(), st.n_rows, self.d_row_ptr.data_ptr(), self.d_col.data_ptr(),
                                             self.d_contrib_ptr.data_ptr(), self.d_contrib.data_ptr(), st.n_blocks, st.nnzb,
                                             st.n_contrib, self.d_values.data_ptr(), self.d_grad.data_ptr(),
                                             self.d_cost.data_ptr(), sp))
        if not sync:
            return None
        cost = float(self.d_cost.cpu().numpy()[0])
        check(self.lib.nhip_dev_status(sp, None))
        return cost

    def solve(self, lam, diag_floor=1e-9, tol=1e-10, max_iters=None, check_every=32):
        """(H + lam diag(diag(H) + diag_floor)) x = -g over the free blocks by block-Jacobi PCG (nhip_bsr_pcg_dev):
        (x (3 n_blocks,) float64 on the host, PcgResult)."""
        st, max_iters = self.st, self._max_iters(max_iters)
        stats, sp = _lib.PcgStats(), self._stream()
        check(self.lib.nhip_bsr_pcg_dev(self.d_row_ptr.data_ptr(), self.d_col.data_ptr(), self.d_values.data_ptr(),
                                        self.d_grad.data_ptr(), self.d_fixed.data_ptr(), st.n_blocks, st.nnzb, float(lam),
                                        float(diag_floor), float(tol), int(max_iters), int(check_every), self.d_x.data_ptr(),
                                        self.d_ws.data_ptr(), self.ws_bytes, C.byref(stats), sp))
        x = self.d_x[:3 * st.n_blocks].cpu().numpy()
        check(self.lib.nhip_dev_status(sp, None))
        return x, PcgResult(stats.iterations, stats.flag, stats.relative_residual)

    def inverse_columns(self, gauge, rhs_index, ridge=1e-12, tol=1e-10, max_iters=None, check_every=32, max_bytes=1 << 30):
        """Columns of inverses of the matrix the last assemble left on the device (nhip_bsr_pcg_columns_dev): system s solves
        (H + ridge I) x = e_j, j = rhs_index[s], over the blocks that are neither in the fixed mask nor block gauge[s] (-1:
        none), by the block-Jacobi PCG of solve.  Returns (x, [PcgResult]): x a (3 n_blocks, S) float64 DEVICE tensor, column
        s the solution of system s (zero on the blocks that are not free).  The systems are solved in chunks so that one
        call's x and workspace stay within max_bytes (at least one system per call); a system's bits do not depend on the
        chunking.  .column_batches lists the calls: (systems, the iterations of the slowest, seconds)."""
        st, torch = self.st, self.torch
        gauge = np.ascontiguousarray(gauge, dtype=np.int32).reshape(-1)
        rhs_index = np.ascontiguousarray(rhs_index, dtype=np.int32).reshape(-1)
        if len(gauge) != len(rhs_index):
            raise ValueError("inverse_columns: %d gauges for %d right-hand sides" % (len(gauge), len(rhs_index)))
        max_iters = self._max_iters(max_iters)
        S, n3 = len(gauge), 3 * st.n_blocks
        x = torch.zeros((n3, S), dtype=torch.float64, device=self.dev)
        results, self.column_batches = [], []
        if S == 0 or n3 == 0:
            return x, results
        need = lambda n: int(self.lib.nhip_bsr_pcg_columns_workspace_bytes(st.n_blocks, st.nnzb, n))
        chunk = S
        while chunk > 1 and need(chunk) + 8 * n3 * chunk > max_bytes:
            chunk = (chunk + 1) // 2
        chunk = min(chunk, max((2 ** 31 - 1) // n3, 1))
        sp = self._stream()
        for s0 in range(0, S, chunk):
            n = min(chunk, S - s0)
            d_gauge = torch.from_numpy(gauge[s0:s0 + n]).to(self.dev)
            d_rhs = torch.from_numpy(rhs_index[s0:s0 + n]).to(self.dev)
            whole = n == S
            d_x = x if whole else torch.empty((n3, n), dtype=torch.float64, device=self.dev)
            ws_bytes = need(n)
            d_ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.dev)
            stats = (_lib.PcgStats * n)()
            t0 = time.perf_counter()
            check(self.lib.nhip_bsr_pcg_columns_dev(self.d_row_ptr.data_ptr(), self.d_col.data_ptr(), self.d_values.data_ptr(),
                                                    self.d_fixed.data_ptr(), st.n_blocks, st.nnzb, d_gauge.data_ptr(),
                                                    d_rhs.data_ptr(), n, float(ridge), float(tol), int(max_iters),
                                                    int(check_every), d_x.data_ptr(), d_ws.data_ptr(), ws_bytes, stats, sp))
            self.column_batches.append((n, max(r.iterations for r in stats), time.perf_counter() - t0))  # (returns drained)
            if not whole:
                x[:, s0:s0 + n] = d_x
            results += [PcgResult(r.iterations, r.flag, r.relative_residual) for r in stats]
        check(self.lib.nhip_dev_status(sp, None))
        return x, results

    def download(self):
        """(values (nnzb, 3, 3), grad (3 n_blocks,), cost) on the host."""
        st = self.st
        return (self.d_values[:9 * st.nnzb].cpu().numpy().reshape(st.nnzb, 3, 3), self.d_grad[:3 * st.n_blocks].cpu().numpy(),
                float(self.d_cost.cpu().numpy()[0]))
