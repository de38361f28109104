"""The branch-and-bound matcher at the limit of its LDS.  What a launch of csm_bnb_kernel asks for is computed on the host
(nhip_bnb_params.h lds_bytes: first region + 512 bytes per rotation + the queue's space + the tail), and so is the choice
between the instantiations that stage the pooled table in LDS and those that read it from global memory; a wrong byte
count fails no assertion inside the kernel, it reads or writes LDS out of bounds.  These are the smallest searches that
sit on both sides of each threshold.  The constants, as they stand in nhip_bnb_params.h and nhip_bnb_host.hip:

    first region   max(pooled table if staged, ORG_LDS = 8 waves * 17 chunks * 64 words * 4 = 34,816)
    bounds         512 * n_theta
    queue + tail   QCAP * 8 + 64 = 8,256   (the split form: QSPACE_SPLIT * 8 + 64 = 8,240, never more)
    limit          160 * 1024 = 163,840

On the 1,200-cell grid of _specs() (30 m at 0.05 m, max_shift 40) the pooled table has 35,712 bytes, so
    staged:      35,712 + 512 n + 8,256 <= 163,840  <=>  n <= 234  (234: 163,776 bytes; 235: 164,288)
    not staged:  34,816 + 512 n + 8,256 <= 163,840  <=>  n <= 235  (235: 163,392 bytes; 236: 163,904)
A search has an odd number of rotations (check_search of nhip_csm_plan.hip requires it, and so does the oracle), so the cases are the odd counts
on either side: 233 rotations are the last that run with POOL_LDS = true (163,264 bytes), 235 the last the matcher admits
and the first with POOL_LDS = false (163,392 bytes, the largest launch there is), 237 go to the kernel that performs every
add.  Three pairs, a 9 x 9 lattice of translations, both cell widths; every form through the environment hooks, the
every-add kernels and the oracle: records and sums byte-equal.

The pairs go through the device-pointer entry point with a workspace of the test's own: the handle API prices its
workspace at 64 rotations (nhip_csm_workspace_bytes), where the split form's state of three pairs at 235 rotations --
3,072 + 3 * (22 + 512 * 235) bytes per round, rounded up to 364,544 -- does not fit, and the hooks would quietly get the
fused form.  4 MiB hold two rounds' state and more."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from nautilus_amd import _lib, csm
from oracle import oracle as O

pytestmark = pytest.mark.gpu

DEG = math.radians(1.0)
ORG_LDS, PER_ROTATION, QUEUE_AND_TAIL, LDS_MAX = 8 * 17 * 64 * 4, 128 * 4, 1024 * 8 + 64, 160 * 1024
WORKSPACE = 4 << 20
N_PAIRS = 3

# (environment, form id nhip_csm_last_launch reports): the forms of tests/test_csm_gpu.py _check_pairs, with rounds of two
# pairs so that three pairs take every split form, and the instrumented build (its launchers size the LDS the same way)
FORMS = [
    ({}, 0),
    ({"NHIP_BNB_KERNELS": "1"}, 0),
    ({"NHIP_BNB_KERNELS": "1", "NHIP_BNB_LEVELS": "1"}, 0),
    ({"NHIP_BNB_KERNELS": "1", "NHIP_BNB_QUEUE": "1"}, 0),
    ({"NHIP_BNB_KERNELS": "2", "NHIP_BNB_LEVELS": "1"}, 0),
    ({"NHIP_BNB_KERNELS": "2", "NHIP_BNB_HEAVY_MIN": "1", "NHIP_BNB_KEEP_RANKS": "0"}, 0),
    ({"NHIP_BNB_KERNELS": "1", "NHIP_BNB_SPLIT": "1"}, 1),
    ({"NHIP_BNB_KERNELS": "1", "NHIP_BNB_SPLIT": "1", "NHIP_BNB_SPLIT_BATCH": "2", "NHIP_BNB_SPLIT_MIN": "1",
      "NHIP_BNB_SPLIT_MAX": "5"}, 3),
    ({"NHIP_BNB_KERNELS": "1", "NHIP_BNB_SPLIT": "1", "NHIP_BNB_SPLIT_BATCH": "2", "NHIP_BNB_SPLIT_OVERLAP": "0",
      "NHIP_BNB_LEVELS": "1"}, 2),
    ({"NHIP_BNB_INSTRUMENT": "1", "NHIP_BNB_KERNELS": "1"}, 0),
    ({"NHIP_BNB_INSTRUMENT": "1", "NHIP_BNB_KERNELS": "1", "NHIP_BNB_SPLIT": "1"}, 1),
]


def _last_admitted(first_region):
    return (LDS_MAX - QUEUE_AND_TAIL - first_region) // PER_ROTATION


class _World:
    """Three pairs of the small bag on device tables of one cell width, and the oracle's tables (built once per width)."""

    def __init__(self, bag, cell_bits):
        import torch
        dev = torch.device("cuda:0")
        self.t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.lib = lib = _lib.load()
        # (16-bit slots with their skip maps, which the handle API would add late: the strip kernel reads them unless DENSE)
        self.spec = csm.grid_spec(30.0, 0.05, 2.0, 1e-10, 40, cell_bits, skip_map=cell_bits == 16)
        self.ospec = O.grid_spec(30.0, 0.05, 2.0, 1e-10, cell_bits)
        src, tgt, self.th0 = (a[:N_PAIRS] for a in bag.sample_pairs(per_target=2, targets=[9, 30], min_sep=2))
        self.ids = np.unique(tgt).astype(np.int32)
        self.src, self.slot = np.asarray(src, np.int32), np.searchsorted(self.ids, tgt).astype(np.int32)
        self.xy, self.off = csm.pack_scans(bag.scans)
        self.n_scans = len(bag.scans)
        self.d_xy, self.d_off = self.t(self.xy), self.t(self.off)
        n = len(self.ids)
        self.G = torch.empty(lib.nhip_grids_bytes(C.byref(self.spec), n), dtype=torch.uint8, device=dev)
        ws_g = lib.nhip_grid_workspace_bytes(C.byref(self.spec), n)
        W = torch.zeros(ws_g, dtype=torch.uint8, device=dev)
        self.sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.info = (C.c_int32 * 4)()
        d_ids = self.t(self.ids)
        _lib.check(lib.nhip_grid_build_dev(self.d_xy.data_ptr(), self.d_off.data_ptr(), self.n_scans, d_ids.data_ptr(), n,
                                           C.byref(self.spec), self.G.data_ptr(), W.data_ptr(), ws_g, self.sp))
        assert lib.nhip_dev_status(self.sp, self.info) == _lib.NHIP_OK
        self.d_src, self.d_slot, self.d_rot0 = self.t(self.src), self.t(self.slot), self.t(csm.rot0_table(self.th0))
        self.d_keys = torch.empty(N_PAIRS, dtype=torch.int64, device=dev)
        self.d_out = torch.empty((N_PAIRS, 4), dtype=torch.int32, device=dev)
        self.d_sums = torch.empty(N_PAIRS, dtype=torch.int32, device=dev)
        assert WORKSPACE >= lib.nhip_csm_workspace_bytes(N_PAIRS)
        self.d_ws = torch.empty(WORKSPACE, dtype=torch.uint8, device=dev)
        self.ogr = O.grid_build_batch(self.xy, self.off, self.ids, self.ospec)

    def match(self, search, env=()):
        d_delta = self.t(csm.delta_table(search))
        self.d_out.fill_(-7)
        self.d_sums.fill_(-7)
        os.environ.update(env)
        try:
            _lib.check(self.lib.nhip_csm_match_dev(
                self.d_xy.data_ptr(), self.d_off.data_ptr(), self.n_scans, self.G.data_ptr(), len(self.ids), C.byref(self.spec),
                self.d_src.data_ptr(), self.d_slot.data_ptr(), self.d_rot0.data_ptr(), d_delta.data_ptr(), None, N_PAIRS,
                C.byref(search), self.d_keys.data_ptr(), self.d_out.data_ptr(), self.d_sums.data_ptr(), self.d_ws.data_ptr(),
                WORKSPACE, self.sp))
            launch = csm.last_launch()
        finally:
            for k in env:
                os.environ.pop(k, None)
        assert self.lib.nhip_dev_status(self.sp, self.info) == _lib.NHIP_OK
        return self.d_out.cpu().numpy().copy().view(csm.MATCH_DTYPE).reshape(-1), self.d_sums.cpu().numpy().copy(), launch


@pytest.fixture(scope="module", params=[8, 16], ids=["8bit", "16bit"])
def world(request, gpu, small_bag):
    return _World(small_bag, request.param)


@pytest.mark.parametrize("n_theta,admitted", [(233, True), (235, True), (237, False)])
def test_rotation_counts_at_the_lds_limit(world, n_theta, admitted):
    w = world
    pool = csm.grid_layout(w.spec).pool_bytes
    assert pool == 35712 and pool > ORG_LDS and pool % 16 == 0
    # the arithmetic of the docstring, from the constants: up to 234 rotations staged, up to 235 admitted
    assert (_last_admitted(pool), _last_admitted(ORG_LDS)) == (234, 235)
    assert admitted == (n_theta <= _last_admitted(ORG_LDS))
    search = csm.search_spec(n_theta, 9, 9, DEG)
    got, sums, _ = w.match(search)
    for env, form in FORMS:
        got_v, sums_v, launch = w.match(search, env)
        assert got_v.tobytes() == got.tobytes() and np.array_equal(sums_v, sums), env
        if admitted:  # (the branch-and-bound matcher ran, in the form the hooks ask for)
            assert launch["form_id"] == form and launch["n_pairs"] == N_PAIRS, (env, launch)
            assert launch["instrumented"] == ("NHIP_BNB_INSTRUMENT" in env), (env, launch)
    # the kernels that perform every add: lanes are poses (9 x 9 <= 256), the strip kernel, and that with every zero strip
    ex = csm.search_spec(n_theta, 9, 9, DEG, exhaustive=True)
    for env in ({}, {"NHIP_CSM_SMALL": "0"}, {"NHIP_CSM_DENSE": "1"}):
        got_e, sums_e, _ = w.match(ex, env)
        assert got_e.tobytes() == got.tobytes() and np.array_equal(sums_e, sums), env
    want = O.csm_match_batch(w.xy, w.off, w.ogr, w.ospec, w.src, w.slot, w.th0, O.search_spec(n_theta, 9, 9, DEG))
    for f in ("itheta", "ix", "iy"):
        assert np.array_equal(got[f], want[f]), (f, got[f], want[f])
    assert np.array_equal(sums, want["sum"])
    assert np.array_equal(got["score"], want["score"].astype(np.float32))
    assert sums.min() > 0  # (the pairs do score)
