"""The exact-score pass (NHIP_SEARCH_EXACT_SCORE: csm_exact_score_kernel, nhip_csm_score.hip) at every blur radius class,
window position, point count and pair count at which it can go wrong, against its definition in numpy with a longdouble
mean.  tests/exact_score_cases.py places the inputs and states the definition and the bound;
tests/test_exact_score_cases_cpu.py shows that each input sits where it claims and that the oracle agrees.

Per blur radius -- R = 2 and 8 and 15 (the generic instantiation: 5 rows, 17 bits, the 31-bit mask), 3 (<7>), 6 (<13>) --
every list runs on 8- and 16-bit cells, with and without the row-major image (NHIP_GRID_NO_IMAGE, where all scans are short),
through the device-pointer entry point, twice: a record's score must lie in the closed float interval
[float32(ref - w), float32(ref + w)], w = |ref| (K + n) 2**-53 -- one float unless the definition sits on a rounding
boundary --, the same bits on the second run, and for a forced pose the same bits in all four kinds of slot.  Searched
lists return the indices and sums of the search without the flag (and the oracle's), and their score is the definition's AT
THE RETURNED POSE.  Sentinels behind `out` and `sums` stay.  Then the gate one float step either side of a score, centres
at and beyond max_shift, and a radius-16 grid, which the flagged call refuses before anything is launched."""
import ctypes as C
import math

import numpy as np
import pytest

from nautilus_amd import _lib, csm
from tests import exact_score_cases as X

pytestmark = pytest.mark.gpu

CONFIGS = [(8, False), (16, False), (8, True), (16, True)]  # (cell_bits, no_image)
TAIL = 8
SENTINEL = -7


class _World:
    """The target of one blur radius and the scans of all its lists on the device; tables built on demand."""

    def __init__(self, sigma):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda:0")
        self.lib = _lib.load()
        self.sigma = sigma
        self.lists = X.lists(sigma)
        scans, self.base = [X.target(sigma)], {}
        for name, L in self.lists.items():
            self.base[name] = len(scans)
            scans += L.scans
        self.xy, self.off = csm.pack_scans(scans)
        self.n_scans = len(scans)
        self.d_xy, self.d_off = self.t(self.xy if len(self.xy) else np.zeros((1, 2), np.float32)), self.t(self.off)
        self.sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.info = (C.c_int32 * 4)()
        self.tables = {}
        self.refs = {}

    def t(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def table(self, cell_bits, no_image, floor_p):
        key = (cell_bits, no_image, floor_p)
        if key not in self.tables:
            torch, lib = self.torch, self.lib
            spec = X.spec(self.sigma, cell_bits, no_image, floor_p)
            G = torch.zeros(lib.nhip_grids_bytes(C.byref(spec), 1), dtype=torch.uint8, device=self.dev)
            ws = lib.nhip_grid_workspace_bytes(C.byref(spec), 1)
            W = torch.zeros(ws, dtype=torch.uint8, device=self.dev)
            ids = self.t(np.zeros(1, np.int32))
            _lib.check(lib.nhip_grid_build_dev(self.d_xy.data_ptr(), self.d_off.data_ptr(), self.n_scans, ids.data_ptr(), 1,
                                               C.byref(spec), G.data_ptr(), W.data_ptr(), ws, self.sp))
            assert lib.nhip_dev_status(self.sp, self.info) == _lib.NHIP_OK
            self.tables[key] = (spec, G)
        return self.tables[key]

    def match(self, L, cell_bits, no_image, exact=True, min_score=-math.inf, expect=_lib.NHIP_OK):
        """(records, sums, keys' sentinel intact) of list L through nhip_csm_match_gated_dev; the TAIL entries behind both
        arrays must come back untouched."""
        torch, lib = self.torch, self.lib
        spec, G = self.table(cell_bits, no_image, L.floor_p)
        n = len(L.src)
        n_theta, nx, ny, step = L.lattice
        # (the caller's promise that no scan is long, as the handle call makes it from the lengths it knows: slots without an image need it)
        search = csm.search_spec(n_theta, nx, ny, step, exact_score=exact, short_scans=L.short)
        d_src, d_slot = self.t((self.base[L.name] + L.src).astype(np.int32)), self.t(np.zeros(n, np.int32))
        d_rot0, d_delta = self.t(csm.rot0_table(L.theta0)), self.t(csm.delta_table(search))
        d_org = None if L.origin is None else self.t(L.origin)
        d_keys = torch.full((n,), SENTINEL, dtype=torch.int64, device=self.dev)
        d_out = torch.full((n + TAIL, 4), SENTINEL, dtype=torch.int32, device=self.dev)
        d_sums = torch.full((n + TAIL,), SENTINEL, dtype=torch.int32, device=self.dev)
        ws = lib.nhip_csm_workspace_bytes(n)
        d_ws = torch.empty(ws, dtype=torch.uint8, device=self.dev)
        rc = lib.nhip_csm_match_gated_dev(self.d_xy.data_ptr(), self.d_off.data_ptr(), self.n_scans, G.data_ptr(), 1, C.byref(spec),
                                          d_src.data_ptr(), d_slot.data_ptr(), d_rot0.data_ptr(), d_delta.data_ptr(),
                                          None if d_org is None else d_org.data_ptr(), n, C.byref(search), d_keys.data_ptr(),
                                          d_out.data_ptr(), d_sums.data_ptr(), d_ws.data_ptr(), ws, self.sp, float(min_score))
        assert rc == expect, (rc, lib.nhip_last_error())
        assert lib.nhip_dev_status(self.sp, self.info) == _lib.NHIP_OK
        out, sums, keys = d_out.cpu().numpy(), d_sums.cpu().numpy(), d_keys.cpu().numpy()
        assert np.all(out[n:] == SENTINEL) and np.all(sums[n:] == SENTINEL), "a write behind the records"
        return out[:n].copy().view(csm.MATCH_DTYPE).reshape(-1), sums[:n].copy(), bool(np.all(keys == SENTINEL))

    def reference(self, L, i, pose):
        key = (L.name, i, pose)
        if key not in self.refs:
            self.refs[key] = X.reference(L, i, pose)
        return self.refs[key]


@pytest.fixture(scope="module", params=X.SIGMAS, ids=["R%d" % X.radius(s) for s in X.SIGMAS])
def world(request, gpu):
    return _World(request.param)


def _poses(rec):
    return [(int(r["itheta"]), int(r["ix"]), int(r["iy"])) for r in rec]


def _check_scores(w, L, rec, tally):
    """Every record's score in its interval at the record's pose; tally: [cases, wide intervals, worst ratio]."""
    for i, pose in enumerate(_poses(rec)):
        n = int(L.n_points[i])
        ref = w.reference(L, i, pose)
        lo, hi = X.interval(ref, n)
        got = rec["score"][i]
        # how far the record is from the definition, in units of what the bound and the float's rounding allow
        allowed = abs(ref) * X.LD((X.K_EXACT + n) * X.U) + X.LD(np.spacing(np.abs(np.float32(ref)))) / 2
        ratio = float(abs(X.LD(got) - ref) / allowed) if allowed > 0 else float(got != 0)
        tally[0] += 1
        tally[1] += int(lo != hi)
        tally[2] = max(tally[2], ratio)
        assert lo <= got <= hi, (L.name, i, L.tags[i], pose, n, float(got).hex(), float(lo).hex(), float(hi).hex(), ratio)


def test_every_list_in_every_kind_of_slot(world):
    w = world
    tally = [0, 0, 0.0]
    Lf32 = np.float32(math.log(X.FLOOR_P))
    for name, L in w.lists.items():
        scores = {}
        for cfg in CONFIGS:
            if cfg[1] and not L.short:
                continue  # (slots without an image serve scans of at most 1088 points: counts*_short is that list without the long one)
            rec, sums, _ = w.match(L, *cfg)
            rec2, sums2, _ = w.match(L, *cfg)
            assert rec.tobytes() == rec2.tobytes() and np.array_equal(sums, sums2), (name, cfg, "a second run differs")
            if name == "shift_beyond":  # a centre the border cannot cover scores nothing: pose 0, the floor, sum 0
                assert _poses(rec) == [(0, 0, 0)] * len(rec) and np.all(rec["score"] == Lf32) and np.all(sums == 0), (cfg, rec, sums)
                continue
            if L.forced:
                assert _poses(rec) == [(0, 0, 0)] * len(rec), (name, cfg)
            else:
                plain, plain_sums, _ = w.match(L, *cfg, exact=False)
                for f in ("itheta", "ix", "iy"):
                    assert np.array_equal(rec[f], plain[f]), (name, cfg, f)
                assert np.array_equal(sums, plain_sums), (name, cfg)
                want = [X.oracle_pose(L, i, cfg[0]) for i in range(len(L.src))]
                assert _poses(rec) == [p for p, _ in want] and sums.tolist() == [s for _, s in want], (name, cfg)
            _check_scores(w, L, rec, tally)
            scores[cfg] = rec["score"].tobytes()
        if L.forced:  # the exact score does not depend on how the cells are stored
            assert len(scores) == len(CONFIGS) and len(set(scores.values())) == 1, (name, "the score depends on the cells' storage")
    probes = w.lists["probes"]
    rec, _, _ = w.match(probes, 16, False)
    tags = np.array(probes.tags)
    assert np.all(rec["score"][tags == "empty"] == Lf32)
    assert (rec["score"][tags == "block"] == 0.0).sum() >= 1
    print("R = %d: %d records, worst |got - ref| / (bound + half a float step) = %.3f, %d intervals of more than one float"
          % (X.radius(w.sigma), tally[0], tally[2], tally[1]))
    assert tally[0] > 3000 and tally[1] < 0.01 * tally[0]


def test_pairs_land_in_their_own_records(world):
    """Lists of 1, 7, 8, 9, 15, 17 pairs with pairwise different scores: a wrong pair <-> workgroup mapping is a permutation."""
    w = world
    for n in X.PAIR_LISTS:
        L = w.lists["pairs%d" % n]
        rec, sums, _ = w.match(L, 16, False)
        assert _poses(rec) == [(0, 0, 0)] * n
        want = [X.interval(w.reference(L, i, (0, 0, 0)), int(L.n_points[i])) for i in range(n)]
        assert len(set(want)) == n and all(lo == hi for lo, hi in want)
        assert rec["score"].tolist() == [lo for lo, _ in want], (n, rec["score"], want)


def _gated(rec, sums, m):
    """The contract: kept unchanged when (double)score >= min_score, else the rejected record."""
    rec, sums = rec.copy(), sums.copy()
    out = rec["score"].astype(np.float64) < m
    rec[out] = (-1, -1, -1, -np.inf)
    sums[out] = -1
    return rec, sums


def test_gate_one_float_step_either_side_of_a_score(world):
    w = world
    L = w.lists["pairs17"]
    for cfg in ((16, False), (8, False)):
        rec, sums, _ = w.match(L, *cfg)
        order = np.argsort(rec["score"])
        for j in (order[0], order[len(order) // 2]):
            s = rec["score"][j]
            up = np.nextafter(s, np.float32(np.inf))
            kept, kept_sums, _ = w.match(L, *cfg, min_score=float(s))
            want = _gated(rec, sums, float(s))
            assert not csm.rejected(kept)[j] and kept.tobytes() == want[0].tobytes() and np.array_equal(kept_sums, want[1]), (cfg, j)
            gone, gone_sums, _ = w.match(L, *cfg, min_score=float(up))
            want = _gated(rec, sums, float(up))
            assert csm.rejected(gone)[j] and gone_sums[j] == -1 and gone["score"][j] == -np.inf
            assert gone.tobytes() == want[0].tobytes() and np.array_equal(gone_sums, want[1]), (cfg, j)
            assert np.count_nonzero(csm.rejected(gone)) == np.count_nonzero(csm.rejected(kept)) + 1  # every other record as it was
        assert not csm.rejected(w.match(L, *cfg, min_score=float(rec["score"][order[0]]))[0]).any()


def test_public_call_refuses_a_centre_beyond_max_shift(world):
    w = world
    L_ok, L_far = w.lists["shift_ok"], w.lists["shift_beyond"]
    st = csm.ScanTable(w.xy, w.off)
    grids = csm.LikelihoodGrids(st, np.zeros(1, np.int32), X.spec(w.sigma, 16))
    try:
        search = csm.search_spec(*L_ok.lattice, exact_score=True)
        rec, sums = csm.match_pairs(st, grids, w.base["shift_ok"] + L_ok.src, np.zeros(4, np.int32), L_ok.theta0, search, pair_origin=L_ok.origin)
        dev, dev_sums, _ = w.match(L_ok, 16, False)
        assert rec.tobytes() == dev.tobytes() and np.array_equal(sums, dev_sums)
        with pytest.raises(_lib.NhipError, match="max_shift") as e:
            csm.match_pairs(st, grids, w.base["shift_beyond"] + L_far.src, np.zeros(3, np.int32), L_far.theta0, search, pair_origin=L_far.origin)
        assert e.value.code == _lib.NHIP_ERR_ARG
    finally:
        grids.close()
        st.close()


def test_radius_16_is_refused_before_anything_is_launched(gpu):
    """sigma 5.3 (R = 16) is a grid the layout admits and the search takes; the exact-score pass reads windows of at most 31
    bits, so the flagged call is an argument error -- with the records, the sums and the keys as the caller left them."""
    w = _World(5.3)
    assert csm.grid_layout(X.spec(5.3)).blur_radius == 16
    for name in ("pairs9", "counts0"):
        L = w.lists[name]
        for cfg in ((16, False), (8, True)):
            if cfg[1] and not L.short:
                continue
            rec, sums, keys_intact = w.match(L, *cfg, exact=False)
            assert not keys_intact and np.all(rec["itheta"] >= 0) and np.all(sums >= 0) and sums.max() > 0
            rec, sums, keys_intact = w.match(L, *cfg, exact=True, expect=_lib.NHIP_ERR_ARG)
            assert "radius 16" in w.lib.nhip_last_error().decode()
            assert keys_intact and np.all(rec.view(np.int32) == SENTINEL) and np.all(sums == SENTINEL), "a refused call wrote"
    # the handle call: the same error, the caller's arrays untouched
    st = csm.ScanTable(w.xy, w.off)
    grids = csm.LikelihoodGrids(st, np.zeros(1, np.int32), X.spec(5.3, 16))
    try:
        L = w.lists["pairs9"]
        src, slot = w.base["pairs9"] + L.src, np.zeros(9, np.int32)
        plain, _ = csm.match_pairs(st, grids, src, slot, L.theta0, csm.search_spec(*L.lattice), pair_origin=L.origin)
        assert np.all(plain["itheta"] == 0)
        out = np.zeros(9, dtype=csm.MATCH_DTYPE)
        out[:] = (7, 7, 7, 7.0)
        sums = np.full(9, 7, np.int32)
        search = csm.search_spec(*L.lattice, exact_score=True)
        rc = w.lib.nhip_csm_match(st._h, grids._h, _lib.ptr(np.ascontiguousarray(src, np.int32)), _lib.ptr(slot), _lib.ptr(L.theta0),
                                  _lib.ptr(L.origin), 9, C.byref(search), _lib.ptr(out), _lib.ptr(sums))
        assert rc == _lib.NHIP_ERR_ARG and "radius 16" in w.lib.nhip_last_error().decode()
        assert np.all(out["itheta"] == 7) and np.all(out["score"] == 7.0) and np.all(sums == 7)
    finally:
        grids.close()
        st.close()
