"""The free-space check on the GPU (K15, nhip_freespace.hip) against its numpy reference (tests/freespace_reference.py):
planes and counts must be array_equal.  A 120-cell grid (range 3 m, res 0.05, max_shift 8), lattices 1 x 1 x 1 and
3 x 3 x 3 with pair_origin choosing the pose, scans built from cell centres; one 1200-cell target for the band seams."""
import ctypes as C
import functools

import numpy as np
import pytest

from nautilus_amd import _lib, csm, freespace
from tests import freespace_reference as R

pytestmark = pytest.mark.gpu


class Rig:
    """Scans on the device, the tables of `targets` (scan ids) built by nhip_grid_build_dev, their free planes traced."""

    def __init__(self, scans, targets, grid_spec, device="cuda:0"):
        import torch
        self.torch, self.lib, self.dev, self.spec = torch, _lib.load(), torch.device(device), grid_spec
        self.L = csm.grid_layout(grid_spec)
        xy, off = R.pack(scans)
        self.n_scans, self.n_slots = len(off) - 1, len(targets)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self.t = t
        self.d_xy = t(xy) if len(xy) else torch.zeros((1, 2), dtype=torch.float32, device=self.dev)
        self.d_off, self.d_ids = t(off), t(np.asarray(targets, dtype=np.int32))
        self.sp = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)
        self.d_grids = torch.empty(self.lib.nhip_grids_bytes(C.byref(grid_spec), self.n_slots), dtype=torch.uint8, device=self.dev)
        self.d_grids[-256:].zero_()
        ws = self.lib.nhip_grid_workspace_bytes(C.byref(grid_spec), self.n_slots)
        d_ws = torch.empty(ws, dtype=torch.uint8, device=self.dev)
        _lib.check(self.lib.nhip_grid_build_dev(self.d_xy.data_ptr(), self.d_off.data_ptr(), self.n_scans, self.d_ids.data_ptr(),
                                                self.n_slots, C.byref(grid_spec), self.d_grids.data_ptr(), d_ws.data_ptr(), ws, self.sp))
        _lib.check(self.lib.nhip_dev_status(self.sp, None))
        self.d_free = self.trace()

    def trace(self, d_ids=None):
        return freespace.trace_on_device(self.d_xy, self.d_off, self.n_scans, self.d_ids if d_ids is None else d_ids, self.n_slots,
                                         self.spec, self.d_grids)

    def plane(self, slot, d_free=None):
        raw = (self.d_free if d_free is None else d_free).cpu().numpy()
        return freespace.plane_cells(raw[slot * self.L.hits_bytes:(slot + 1) * self.L.hits_bytes], self.L)

    def counts(self, src, slot, theta0, poses, lattice, fs, origin=None):
        """(counts (n, 8), info of nhip_dev_status, its return code)"""
        n, search = len(src), csm.search_spec(*lattice)
        rec = R.records(poses)
        d_m = self.t(rec.view(np.int32).reshape(-1, 4)) if n else self.torch.zeros((1, 4), dtype=self.torch.int32, device=self.dev)
        i32 = lambda a: self.t(np.asarray(a, dtype=np.int32)) if n else self.torch.zeros(2, dtype=self.torch.int32, device=self.dev)
        rot0 = csm.rot0_table(np.asarray(theta0, dtype=np.float64)) if n else np.zeros((1, 2))
        d_counts = freespace.check_on_device(self.d_xy, self.d_off, self.n_scans, self.d_grids, self.n_slots, self.spec, i32(src), i32(slot),
                                             self.t(rot0), self.t(csm.delta_table(search)), None if origin is None else i32(origin), n,
                                             search, self.d_free, d_m, freespace.spec(hit_radius=fs[0], end_margin=fs[1]))
        info = (C.c_int32 * 4)()
        rc = self.lib.nhip_dev_status(self.sp, info)
        return d_counts.cpu().numpy(), list(info), rc


@functools.lru_cache(maxsize=None)
def plane_rig():
    cases = R.plane_cases()
    names = sorted(cases)
    return names, Rig([cases[k] for k in names], list(range(len(names))), R.small_grid_spec())


@pytest.mark.parametrize("name", sorted(R.plane_cases()))
def test_free_plane(gpu, name):
    """A cell that ends one beam and lies on another, the rims and corners, duplicate ends, the sensor's own cell, NaN, +-inf and
    out-of-grid points, scans of 0 .. 1300 points."""
    names, rig = plane_rig()
    want = R.free_plane(R.plane_cases()[name], R.SIDE, R.RES)
    got = rig.plane(names.index(name))
    assert got.shape == want.shape and np.array_equal(got, want)
    # what the plane is made from: the slot's hit raster holds the end cells, and none of them is free
    hits = R.cells_of_keys(R.target_sets(R.plane_cases()[name], R.SIDE, R.RES)[0], R.SIDE)
    assert not (got & hits).any()


def test_free_plane_bytes_are_whole_and_repeatable(gpu):
    """Every byte of the planes is written (border and tail zero), and two traces give identical bytes."""
    names, rig = plane_rig()
    a = rig.torch.full((freespace.planes_bytes(rig.spec, rig.n_slots),), 0xFF, dtype=rig.torch.uint8, device=rig.dev)
    _lib.check(rig.lib.nhip_freespace_trace_dev(rig.d_xy.data_ptr(), rig.d_off.data_ptr(), rig.n_scans, rig.d_ids.data_ptr(), rig.n_slots,
                                                C.byref(rig.spec), rig.d_grids.data_ptr(), a.data_ptr(), rig.sp))
    b = rig.trace()
    raw, L = a.cpu().numpy(), rig.L
    assert raw.tobytes() == b.cpu().numpy().tobytes() == rig.trace().cpu().numpy().tobytes()
    for s in range(rig.n_slots):
        slot = raw[s * L.hits_bytes:(s + 1) * L.hits_bytes]
        rows = np.unpackbits(slot[:L.hits_pitch * (L.side + 64)].reshape(L.side + 64, L.hits_pitch), axis=1, bitorder="little")
        inner = np.zeros_like(rows)
        inner[32:32 + L.side, 32:32 + L.side] = 1
        assert not (rows & (1 - inner)).any() and not slot[L.hits_pitch * (L.side + 64):].any()


def test_free_plane_across_band_seams(gpu):
    """A 1200-cell grid is four bands of raster rows: rays cross from one band's last row into the next at many slopes."""
    pts = R.seam_target()
    spec = csm.grid_spec(30.0, 0.05, 2.0, 1e-10, 8, 16)
    rig = Rig([pts], [0], spec)
    want = R.free_plane(pts, 1200, 0.05)
    got = rig.plane(0)
    assert want[363:365].sum() > 50 and want[759:761].sum() > 50 and want[1155:1157].sum() > 10
    assert np.array_equal(got, want)


def test_a_stale_target_id_is_reported_and_its_plane_empty(gpu):
    names, rig = plane_rig()
    ids = np.arange(rig.n_slots, dtype=np.int32)
    ids[3] = rig.n_scans + 5
    d_free = rig.trace(rig.t(ids))
    info = (C.c_int32 * 4)()
    assert rig.lib.nhip_dev_status(rig.sp, info) == _lib.NHIP_ERR_ARG and info[1] == 1 and info[2] == rig.n_scans + 5 and info[3] == 3
    assert not rig.plane(3, d_free).any()
    for s in (2, 4):
        assert np.array_equal(rig.plane(s, d_free), rig.plane(s))


@functools.lru_cache(maxsize=None)
def case_rig(name):
    case = next(c for c in R.check_cases() if c["name"] == name)
    targets = sorted(set(case["tgt"].tolist()))
    return case, targets, Rig(case["scans"], targets, R.small_grid_spec())


@pytest.mark.parametrize("name", [c["name"] for c in R.check_cases()])
def test_counts(gpu, name):
    """Classes at every bit offset, radius and rim; hit before free; shifts out of the grid; all 61 rotations; through at the
    margin's edge and with rays outside; sources of 0 .. 1300 points; lists of 1 .. 17 pairs with rejected records between."""
    case, targets, rig = case_rig(name)
    slot = np.searchsorted(targets, case["tgt"])
    for fs in case["fs"]:
        want = R.case_counts(case, fs)
        got, info, rc = rig.counts(case["src"], slot, case["theta0"], case["poses"], case["lattice"], fs, case["origin"])
        assert rc == _lib.NHIP_OK, info
        assert got.dtype == np.int32 and np.array_equal(got, want), (name, fs, got[:4], want[:4])


def test_stale_ids_are_reported_and_the_other_pairs_right(gpu):
    case, targets, rig = case_rig("list_17")
    slot = np.searchsorted(targets, case["tgt"])
    want = R.case_counts(case, (2, 3))
    live = [i for i in range(17) if want[i, 0] >= 0]
    for where, (array, value) in {live[0]: ("src", rig.n_scans), live[2]: ("slot", -1), live[4]: ("slot", rig.n_slots), live[5]: ("itheta", 3),
                                  live[6]: ("ix", 3), live[7]: ("iy", -2)}.items():
        src, sl, poses = case["src"].copy(), slot.copy(), list(case["poses"])
        if array == "src":
            src[where] = value
        elif array == "slot":
            sl[where] = value
        else:
            k, ix, iy = poses[where]
            poses[where] = (value, ix, iy) if array == "itheta" else (k, value, iy) if array == "ix" else (k, ix, value)
        got, info, rc = rig.counts(src, sl, case["theta0"], poses, case["lattice"], (2, 3), case["origin"])
        assert rc == _lib.NHIP_ERR_ARG and info[0] == info[1] == 32768 and info[3] == where, (array, info)
        assert b"nhip_freespace_check_dev" in rig.lib.nhip_last_error()
        assert not got[where].any()
        keep = np.arange(17) != where
        assert np.array_equal(got[keep], want[keep])
    assert rig.lib.nhip_dev_status(rig.sp, None) == _lib.NHIP_OK  # (the record was consumed)


def test_two_runs_give_identical_bytes(gpu):
    case, targets, rig = case_rig("lattice_3x3x3")
    slot = np.searchsorted(targets, case["tgt"])
    runs = [rig.counts(case["src"], slot, case["theta0"], case["poses"], case["lattice"], (2, 3), case["origin"])[0].tobytes() for _ in range(3)]
    assert runs[0] == runs[1] == runs[2]


@pytest.mark.parametrize("name", ["lattice_3x3x3", "list_17", "shift_out_of_the_grid", "through_rays_outside", "source_sizes"])
def test_handle_form_agrees_with_the_dev_form(gpu, name):
    case, targets, rig = case_rig(name)
    slot = np.searchsorted(targets, case["tgt"])
    xy, off = R.pack(case["scans"])
    st = csm.ScanTable(xy, off)
    grids = csm.LikelihoodGrids(st, np.asarray(targets, dtype=np.int32), R.small_grid_spec())
    search = csm.search_spec(*case["lattice"])
    for fs in case["fs"]:
        dev, _, rc = rig.counts(case["src"], slot, case["theta0"], case["poses"], case["lattice"], fs, case["origin"])
        assert rc == _lib.NHIP_OK
        for _ in range(2):  # (the first call traces the handle's planes, the second finds them)
            got = freespace.check_pairs(st, grids, case["src"], slot, case["theta0"], search, R.records(case["poses"]), case["origin"],
                                        freespace.spec(hit_radius=fs[0], end_margin=fs[1]))
            assert np.array_equal(got, dev) and np.array_equal(got, R.case_counts(case, fs))
    # ids out of range are the host's to refuse here
    bad = slot.copy()
    bad[0] = len(targets)
    with pytest.raises(_lib.NhipError, match="slot"):
        freespace.check_pairs(st, grids, case["src"], bad, case["theta0"], search, R.records(case["poses"]), case["origin"])
    grids.close()
    st.close()


def test_a_submap_handle_is_refused(gpu):
    case, targets, rig = case_rig("lattice_3x3x3")
    xy, off = R.pack(case["scans"])
    st = csm.ScanTable(xy, off)
    aff = np.array([[1, 0, 0, 0], [1, 0, 0.1, 0]], np.float32)
    grids = csm.LikelihoodGrids.from_submaps(st, [0, 1], aff, [0, 2], R.small_grid_spec())
    with pytest.raises(_lib.NhipError) as e:
        freespace.check_pairs(st, grids, [1], [0], [0.0], csm.search_spec(1, 1, 1), R.records([(0, 0, 0)]))
    assert e.value.code == _lib.NHIP_ERR_STATE and "submap" in str(e.value)
    grids.close()
    st.close()


def test_bad_specs_are_refused_without_a_launch(gpu):
    case, targets, rig = case_rig("lattice_3x3x3")
    import torch
    d_counts = torch.full((27, 8), 77, dtype=torch.int32, device=rig.dev)
    search = csm.search_spec(3, 3, 3)
    z = torch.zeros(64, dtype=torch.int32, device=rig.dev)
    d_rot, d_m = torch.zeros(64, dtype=torch.float64, device=rig.dev), torch.zeros((27, 4), dtype=torch.int32, device=rig.dev)
    for kw in (dict(hit_radius=17), dict(hit_radius=-1), dict(end_margin=65), dict(end_margin=-1), dict(flags=4), dict(reserved=1)):
        rc = rig.lib.nhip_freespace_check_dev(rig.d_xy.data_ptr(), rig.d_off.data_ptr(), rig.n_scans, rig.d_grids.data_ptr(), rig.n_slots,
                                              C.byref(rig.spec), z.data_ptr(), z.data_ptr(), d_rot.data_ptr(), d_rot.data_ptr(), None, 27,
                                              C.byref(search), rig.d_free.data_ptr(), d_m.data_ptr(), C.byref(freespace.spec(**kw)),
                                              d_counts.data_ptr(), rig.sp)
        assert rc == _lib.NHIP_ERR_ARG and next(iter(kw)) in rig.lib.nhip_last_error().decode()
    torch.cuda.synchronize()
    assert (d_counts.cpu().numpy() == 77).all()
    assert rig.lib.nhip_dev_status(rig.sp, None) == _lib.NHIP_OK
