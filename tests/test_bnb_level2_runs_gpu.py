"""The candidates' strip bounds from runs of level-2 entries (nhip_bnb_origin.h cache_origins, nhip_bnb_bounds.h
strip_bounds_c<RunList>) against the per-cell path, the kernels that perform every add, and the oracle -- on the smallest
scans at which the run list can go wrong.  tests/level2_runs.py places them (and states the list in numpy);
tests/test_bnb_level2_runs_cpu.py shows that each sits where it claims: scans of 1 .. 1088 points, a run across a chunk
start, 64 | 65 and 512 | 513 runs (513: more than the list holds), a 20 cm patch with 512 points in one group of 8 lanes and
its neighbours at exactly 257 and 258 (the 16-bit fields' limit), cells either side of an entry's edge, both alignments
of the strip load.

The hand-placed sources are built from the cells of scan 3 and matched to scan 9, which sees the same walls, at theta0 = 0
(the pair's true offset is 1.3 degrees: a landscape that leaves the candidates' kernel work) on a 17 x 17 lattice -- three
blocks per row, so that strips of one, two and three blocks can form where the bounds leave them -- with three rotations 1e-6 rad apart:
all three see the same cells, so every rotation pass of a pair does what the numpy statement says of it.  Ordinary pairs of
the small bag run at 1 degree, five rotations, 9 x 9.  1,200-cell grid, both cell widths, the device-pointer entry point with
the test's own workspace.  Every form through the hooks, each with and without NHIP_BNB_L2_RUNS=0, each once in the
instrumented build: records and sums byte-equal among all of them, to the every-add kernels and to the oracle.  Then pair by
pair in the instrumented build, where out[16..18] of nhip_bnb_stats_levels count the rotation passes that took the run list,
fell back on the field check, fell back on capacity: a case that only ever ran the fall-back would otherwise prove nothing."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from nautilus_amd import _lib, csm
from oracle import oracle as O
from tests import level2_runs as M

pytestmark = pytest.mark.gpu

WORKSPACE = 8 << 20
SRC_SCAN, TGT_SCAN = 3, 9
KIND = {"runs": "passes_l2_runs", "field": "passes_per_cell_field", "capacity": "passes_per_cell_capacity"}

SPLIT_ONE = {"NHIP_BNB_KERNELS": "1", "NHIP_BNB_SPLIT": "1"}
HAND_OVER = {"NHIP_BNB_KERNELS": "2", "NHIP_BNB_HEAVY_MIN": "1", "NHIP_BNB_KEEP_RANKS": "0"}
# (environment, form id nhip_csm_last_launch reports): fused, fused with everything handed over, split in one round, split
# in rounds of two pairs with a pair shared by up to five workgroups
FORMS = [
    ({"NHIP_BNB_KERNELS": "1"}, 0),
    (HAND_OVER, 0),
    (SPLIT_ONE, 1),
    ({"NHIP_BNB_KERNELS": "1", "NHIP_BNB_SPLIT": "1", "NHIP_BNB_SPLIT_BATCH": "2", "NHIP_BNB_SPLIT_MIN": "1",
      "NHIP_BNB_SPLIT_MAX": "5"}, 3),
]
INSTR = {"NHIP_BNB_INSTRUMENT": "1", "NHIP_BNB_STATS": "1"}
OFF = {"NHIP_BNB_L2_RUNS": "0"}

GROUPS = {
    "lengths": ["len1", "len63", "len64", "len65", "len1081", "len1088", "straddle", "boundary"],
    "seams": ["alt64", "alt65", "alt512", "alt513", "patch", "group257", "group258"],
}


class _World:
    """The small bag's scans and the hand-placed ones on device, tables of two targets of one cell width, the oracle's."""

    def __init__(self, bag, cell_bits):
        import torch
        dev = torch.device("cuda:0")
        self.t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.lib = lib = _lib.load()
        self.spec = csm.grid_spec(30.0, 0.05, 2.0, 1e-10, 40, cell_bits, skip_map=cell_bits == 16)
        self.ospec = O.grid_spec(30.0, 0.05, 2.0, 1e-10, cell_bits)
        self.cases = M.cases(bag.scans[SRC_SCAN])
        self.scan_of = {name: len(bag.scans) + i for i, name in enumerate(self.cases)}
        self.xy, self.off = csm.pack_scans(list(bag.scans) + [c[0] for c in self.cases.values()])
        self.n_scans = len(self.off) - 1
        self.ids = np.array([TGT_SCAN, 30], dtype=np.int32)
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
        self.d_ws = torch.empty(WORKSPACE, dtype=torch.uint8, device=dev)
        self.ogr = O.grid_build_batch(self.xy, self.off, self.ids, self.ospec)
        # the ordinary pairs: three of the bag's, at their own theta0
        src, tgt, th0 = (a[:3] for a in bag.sample_pairs(per_target=2, targets=[9, 30], min_sep=2))
        self.ordinary = (np.asarray(src, np.int32), np.searchsorted(self.ids, tgt).astype(np.int32), np.asarray(th0, np.float64))

    def group(self, names):
        src = np.array([self.scan_of[n] for n in names], np.int32)
        return src, np.zeros(len(names), np.int32), np.zeros(len(names))

    def match(self, pairs, search, env=()):
        import torch
        src, slot, th0 = pairs
        n = len(src)
        assert WORKSPACE >= self.lib.nhip_csm_workspace_bytes(n)
        d_src, d_slot, d_rot0, d_delta = self.t(src), self.t(slot), self.t(csm.rot0_table(th0)), self.t(csm.delta_table(search))
        d_keys = torch.empty(n, dtype=torch.int64, device=d_src.device)
        d_out = torch.full((n, 4), -7, dtype=torch.int32, device=d_src.device)
        d_sums = torch.full((n,), -7, dtype=torch.int32, device=d_src.device)
        os.environ.update(env)
        try:
            _lib.check(self.lib.nhip_csm_match_dev(
                self.d_xy.data_ptr(), self.d_off.data_ptr(), self.n_scans, self.G.data_ptr(), len(self.ids), C.byref(self.spec),
                d_src.data_ptr(), d_slot.data_ptr(), d_rot0.data_ptr(), d_delta.data_ptr(), None, n, C.byref(search),
                d_keys.data_ptr(), d_out.data_ptr(), d_sums.data_ptr(), self.d_ws.data_ptr(), WORKSPACE, self.sp))
            launch = csm.last_launch()
        finally:
            for k in env:
                os.environ.pop(k, None)
        assert self.lib.nhip_dev_status(self.sp, self.info) == _lib.NHIP_OK
        return d_out.cpu().numpy().copy().view(csm.MATCH_DTYPE).reshape(-1), d_sums.cpu().numpy().copy(), launch

    def oracle(self, pairs, n_theta, nxy, step):
        src, slot, th0 = pairs
        return O.csm_match_batch(self.xy, self.off, self.ogr, self.ospec, src, slot, th0, O.search_spec(n_theta, nxy, nxy, step))


@pytest.fixture(scope="module", params=[8, 16], ids=["8bit", "16bit"])
def world(request, gpu, small_bag):
    return _World(small_bag, request.param)


def _all_forms_agree(w, pairs, n_theta, nxy, step):
    search = csm.search_spec(n_theta, nxy, nxy, step)
    got, sums, _ = w.match(pairs, search)
    for env, form in FORMS:
        for extra in ({}, OFF, INSTR, dict(INSTR, **OFF)):
            e = dict(env, **extra)
            got_v, sums_v, launch = w.match(pairs, search, e)
            assert got_v.tobytes() == got.tobytes() and np.array_equal(sums_v, sums), e
            assert launch["form_id"] == form and launch["n_pairs"] == len(pairs[0]), (e, launch)
            assert launch["l2_runs"] == ("NHIP_BNB_L2_RUNS" not in e) and launch["instrumented"] == ("NHIP_BNB_INSTRUMENT" in e), (e, launch)
    ex = csm.search_spec(n_theta, nxy, nxy, step, exhaustive=True)
    for env in ({}, {"NHIP_CSM_SMALL": "0"}, {"NHIP_CSM_DENSE": "1"}):
        got_e, sums_e, _ = w.match(pairs, ex, env)
        assert got_e.tobytes() == got.tobytes() and np.array_equal(sums_e, sums), env
    want = w.oracle(pairs, n_theta, nxy, step)
    for f in ("itheta", "ix", "iy"):
        assert np.array_equal(got[f], want[f]), (f, got[f], want[f])
    assert np.array_equal(sums, want["sum"])
    assert np.array_equal(got["score"], want["score"].astype(np.float32))
    return got, sums


def _passes(w, pairs, search, env):
    """Rotation passes by strip path of one instrumented launch."""
    csm.bnb_stats_levels()  # (reset)
    got, sums, launch = w.match(pairs, search, dict(env, **INSTR))
    assert launch["instrumented"]
    lv = csm.bnb_stats_levels()
    return got, sums, {k: int(lv[v]) for k, v in KIND.items()}


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_hand_placed_scans_every_form(world, group):
    w = world
    pairs = w.group(GROUPS[group])
    got, sums = _all_forms_agree(w, pairs, 3, 17, 1e-6)
    assert sums.max() > 0
    # pair by pair: the path every rotation pass took, in the candidates' kernel and in the hand-over kernel
    search = csm.search_spec(3, 17, 17, 1e-6)
    for i, name in enumerate(GROUPS[group]):
        what = w.cases[name][1]
        one = tuple(a[i:i + 1] for a in pairs)
        for env in (SPLIT_ONE, HAND_OVER):
            got_1, sums_1, n = _passes(w, one, search, env)
            print(name, what, sorted(env)[-1], n)
            assert got_1.tobytes() == got[i:i + 1].tobytes() and sums_1[0] == sums[i], (name, env)
            assert n[what] >= 1, (name, env, n, "no rotation pass reached the kernels that keep a run list")
            assert all(v == 0 for k, v in n.items() if k != what), (name, env, n)
            _, _, n_off = _passes(w, one, search, dict(env, **OFF))
            assert not any(n_off.values()), (name, env, n_off)


def test_ordinary_pairs_take_the_run_path(world):
    w = world
    _all_forms_agree(w, w.ordinary, 5, 9, math.radians(1.0))
    search = csm.search_spec(5, 9, 9, math.radians(1.0))
    for env in (SPLIT_ONE, HAND_OVER):
        _, _, n = _passes(w, w.ordinary, search, env)
        print("ordinary", sorted(env)[-1], n)
        assert n["runs"] >= 1 and n["field"] == 0 and n["capacity"] == 0, (env, n)
