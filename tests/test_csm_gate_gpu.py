"""The matcher's score gate (nhip_csm_match_gated / match_pairs(min_score=...)): a gated call returns what the same call
without a gate returns, with every record whose score is below min_score replaced by the rejected record
{-1, -1, -1, -inf} and its sum by -1 -- byte for byte, in every form the matcher runs in (include/nautilus_hip.h;
DESIGN.md section 3, item 9).  And the work it lets the matcher skip does go away."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from nautilus_amd import _lib, csm
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEG = math.radians(1.0)
LF = math.log(1e-10)


def gate(recs, sums, min_score):
    """What a gated call must return, from the ungated records: the contract, in numpy."""
    recs, sums = recs.copy(), sums.copy()
    out = recs["score"].astype(np.float64) < min_score
    recs[out] = (-1, -1, -1, -np.inf)
    sums[out] = -1
    return recs, sums


@pytest.fixture(scope="module")
def lists():
    """configs[1] (bench.Workload("weak", 1): 10 sources per target within 3.5 m) -- a sample of whole targets -- and a
    configs[3]-style list: 3 targets x 100 sources up to 3.5 m away, flat landscapes and about half the pairs below -5."""
    sys.path.insert(0, ROOT)
    import bench
    wl = bench.Workload("weak", 1)
    c1 = (wl.src[:400], wl.tgt[:400], wl.th0[:400])
    t3 = np.linspace(0, wl.n_scans - 1, 5).astype(np.int32)[1:-1]
    c3 = wl.bag.sample_pairs(per_target=100, targets=t3, max_dist=3.5, min_sep=20, seed=4242)
    st = csm.ScanTable(wl.xy, wl.off)
    yield wl, st, {"configs[1]": c1, "configs[3]-style": c3}
    st.close()


def _grids(st, tgt, cell_bits):
    ids = np.unique(tgt)
    return csm.LikelihoodGrids(st, ids, csm.grid_spec(30.0, 0.05, 2.0, 1e-10, 40, cell_bits)), np.searchsorted(ids, tgt)


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("cell_bits", [16, 8])
@pytest.mark.parametrize("exact", [False, True])
def test_gated_equals_gate_of_ungated(gpu, lists, cell_bits, exact):
    wl, st, L = lists
    search = csm.search_spec(61, 81, 81, DEG, exact_score=exact)
    for name, (src, tgt, th0) in L.items():
        grids, slot = _grids(st, tgt, cell_bits)
        try:
            plain = csm.match_pairs(st, grids, src, slot, th0, search)
            scores = plain[0]["score"]
            if name == "configs[3]-style":  # (the list is what it claims to be: pairs on both sides of -5)
                assert 0 < np.count_nonzero(scores < -5.0) < len(src)
            kept = float(np.sort(scores)[len(scores) // 2])  # the exact float score of an ungated record
            for m in (-5.0, -8.0, LF, 0.0, kept, math.nextafter(kept, math.inf)):
                got = csm.match_pairs(st, grids, src, slot, th0, search, min_score=m)
                assert _same(got, gate(*plain, m)), (name, m)
            # the record whose score is the threshold is kept; one ulp (of a double) above it, rejected
            at = np.flatnonzero(scores == np.float32(kept))[0]
            assert not csm.rejected(csm.match_pairs(st, grids, src, slot, th0, search, min_score=kept)[0])[at]
            assert csm.rejected(csm.match_pairs(st, grids, src, slot, th0, search, min_score=math.nextafter(kept, math.inf))[0])[at]
        finally:
            grids.close()


FORMS = [  # (environment, pairs of the configs[3]-style list, form id nhip_csm_last_launch reports, hand-over kernel)
    ({}, 150, 0, True),
    ({"NHIP_BNB_KERNELS": "1"}, 150, 0, False),
    ({"NHIP_BNB_KERNELS": "2", "NHIP_BNB_HEAVY_MIN": "1", "NHIP_BNB_KEEP_RANKS": "0"}, 150, 0, True),
    ({"NHIP_BNB_KERNELS": "1", "NHIP_BNB_QUEUE": "1"}, 150, 0, False),
    ({}, 300, 1, None),
    ({"NHIP_BNB_KERNELS": "1", "NHIP_BNB_SPLIT": "1"}, 150, 1, None),
    ({"NHIP_BNB_KERNELS": "1", "NHIP_BNB_SPLIT": "1", "NHIP_BNB_SPLIT_BATCH": "40", "NHIP_BNB_SPLIT_OVERLAP": "0"}, 150, 2, None),
    ({"NHIP_BNB_KERNELS": "1", "NHIP_BNB_SPLIT": "1", "NHIP_BNB_SPLIT_BATCH": "40", "NHIP_BNB_SPLIT_MIN": "1",
      "NHIP_BNB_SPLIT_MAX": "5"}, 150, 3, None),
]


def _with_env(env, fn):
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k in env:
            os.environ.pop(k, None)


@pytest.mark.parametrize("cell_bits", [16, 8])
def test_every_form(gpu, lists, cell_bits):
    wl, st, L = lists
    src, tgt, th0 = L["configs[3]-style"]
    grids, slot = _grids(st, tgt, cell_bits)
    try:
        for exact in (False, True):
            search = csm.search_spec(61, 81, 81, DEG, exact_score=exact)
            for env, n, form, second in FORMS:
                args = (st, grids, src[:n], slot[:n], th0[:n], search)
                plain = _with_env(env, lambda: csm.match_pairs(*args))
                launch = csm.last_launch()
                assert launch["form_id"] == form and (second is None or launch["hand_over_kernel"] == second), (env, launch)
                for m in (-5.0, -8.0):
                    got = _with_env(env, lambda: csm.match_pairs(*args, min_score=m))
                    assert csm.last_launch() == launch, (env, m)
                    assert _same(got, gate(*plain, m)), (env, m, exact)
        # the strip kernels (both cell widths: this grid's), and the kernel whose lanes are poses on a few pairs
        # (one pair of 61 x 81 x 81 fits the tiles of rows; 13 x 13 planes take that kernel whole)
        for search, n in ((csm.search_spec(61, 81, 81, DEG, exhaustive=True), 60),
                          (csm.search_spec(61, 81, 81, DEG, exhaustive=True, exact_score=True), 60),
                          (csm.search_spec(61, 81, 81, DEG, exhaustive=True, latency=True), 1),
                          (csm.search_spec(61, 81, 81, DEG, exhaustive=True, latency=True, exact_score=True), 1),
                          (csm.search_spec(9, 13, 13, DEG, exhaustive=True), 60)):
            args = (st, grids, src[:n], slot[:n], th0[:n], search)
            plain = csm.match_pairs(*args)
            for m in (-5.0, -8.0, 0.0):
                assert _same(csm.match_pairs(*args, min_score=m), gate(*plain, m)), (search.flags, m)
        # a list with search centres (the fine level of a coarse-to-fine search)
        org = np.random.default_rng(9).integers(-20, 21, (len(src), 2)).astype(np.int32)
        for exact in (False, True):
            s_ = csm.search_spec(61, 41, 41, DEG, exact_score=exact)
            plain = csm.match_pairs(st, grids, src, slot, th0, s_, org)
            for m in (-5.0, -8.0):
                assert _same(csm.match_pairs(st, grids, src, slot, th0, s_, org, min_score=m), gate(*plain, m)), (exact, m)
    finally:
        grids.close()


def test_against_the_oracle(gpu, lists):
    wl, st, L = lists
    src, tgt, th0 = L["configs[3]-style"]
    sel = np.random.default_rng(2).choice(len(src), 24, replace=False)
    src, tgt, th0 = src[sel], tgt[sel], th0[sel]
    for cell_bits in (16, 8):
        grids, slot = _grids(st, tgt, cell_bits)
        try:
            got, sums = csm.match_pairs(st, grids, src, slot, th0, csm.search_spec(61, 81, 81, DEG), min_score=-5.0)
        finally:
            grids.close()
        ids = np.unique(tgt)
        ospec = O.grid_spec(30.0, 0.05, 2.0, 1e-10, cell_bits)
        og = O.grid_build_batch(wl.xy, wl.off, ids, ospec)
        want = O.csm_match_batch(wl.xy, wl.off, og, ospec, src, slot, th0, O.search_spec(61, 81, 81, DEG))
        rec = np.zeros(len(src), dtype=csm.MATCH_DTYPE)
        for f in ("itheta", "ix", "iy"):
            rec[f] = want[f]
        rec["score"] = want["score"].astype(np.float32)
        rec, wsums = gate(rec, np.asarray(want["sum"], np.int32), -5.0)
        assert 0 < np.count_nonzero(csm.rejected(rec)) < len(src)
        assert got.tobytes() == rec.tobytes() and np.array_equal(sums, wsums), cell_bits


def test_edge_cases(gpu, lists):
    import torch
    wl, st, L = lists
    src, tgt, th0 = L["configs[3]-style"]
    src, tgt, th0 = src[:40], tgt[:40], th0[:40]
    grids, slot = _grids(st, tgt, 16)
    lib = _lib.load()
    search = csm.search_spec(61, 81, 81, DEG)
    try:
        plain = csm.match_pairs(st, grids, src, slot, th0, search)
        assert _same(csm.match_pairs(st, grids, src, slot, th0, search, min_score=-math.inf), plain)
        out = np.zeros(len(src), dtype=csm.MATCH_DTYPE)
        out[:] = (7, 7, 7, 7.0)
        sums = np.full(len(src), 7, np.int32)
        s32, g32 = np.ascontiguousarray(src, np.int32), np.ascontiguousarray(slot, np.int32)
        t64 = np.ascontiguousarray(th0, np.float64)
        rc = lib.nhip_csm_match_gated(st._h, grids._h, _lib.ptr(s32), _lib.ptr(g32), _lib.ptr(t64), None, len(src),
                                      C.byref(search), _lib.ptr(out), _lib.ptr(sums), float("nan"))
        assert rc == _lib.NHIP_ERR_ARG and np.all(out["itheta"] == 7) and np.all(sums == 7)
    finally:
        grids.close()
    # the device-pointer entry point: NaN writes nothing; a stale id is reported and its record (floor score) gated
    dev = torch.device("cuda:0")
    spec = csm.grid_spec(30.0, 0.05, 2.0, 1e-10, 40, 16)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    n_scans = wl.n_scans
    d_xy, d_off = t(wl.xy), t(wl.off)
    ids = np.unique(tgt).astype(np.int32)
    n = len(ids)
    G = torch.empty(lib.nhip_grids_bytes(C.byref(spec), n), dtype=torch.uint8, device=dev)
    ws_g = lib.nhip_grid_workspace_bytes(C.byref(spec), n)
    W = torch.zeros(ws_g, dtype=torch.uint8, device=dev)
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    info = (C.c_int32 * 4)()
    d_ids = t(ids)
    _lib.check(lib.nhip_grid_build_dev(d_xy.data_ptr(), d_off.data_ptr(), n_scans, d_ids.data_ptr(), n, C.byref(spec),
                                       G.data_ptr(), W.data_ptr(), ws_g, sp))
    assert lib.nhip_dev_status(sp, info) == _lib.NHIP_OK
    n_pairs = len(src)
    d_rot0 = t(csm.rot0_table(th0))
    d_delta = t(csm.delta_table(search))
    d_keys = torch.empty(n_pairs, dtype=torch.int64, device=dev)
    d_out = torch.empty((n_pairs, 4), dtype=torch.int32, device=dev)
    d_sums = torch.empty(n_pairs, dtype=torch.int32, device=dev)
    ws = lib.nhip_csm_workspace_bytes(n_pairs)
    d_ws = torch.empty(ws, dtype=torch.uint8, device=dev)

    def match(src_, fn, *gate_arg):
        d_src, d_slot = t(np.asarray(src_, np.int32)), t(np.asarray(slot, np.int32))
        d_out.fill_(-7)
        d_sums.fill_(-7)
        rc = fn(d_xy.data_ptr(), d_off.data_ptr(), n_scans, G.data_ptr(), n, C.byref(spec), d_src.data_ptr(), d_slot.data_ptr(),
                d_rot0.data_ptr(), d_delta.data_ptr(), None, n_pairs, C.byref(search), d_keys.data_ptr(), d_out.data_ptr(),
                d_sums.data_ptr(), d_ws.data_ptr(), ws, sp, *gate_arg)
        rc2 = lib.nhip_dev_status(sp, info)
        return rc, rc2, d_out.cpu().numpy().copy().view(csm.MATCH_DTYPE).reshape(-1), d_sums.cpu().numpy().copy()

    rc, rc2, ref, ref_sums = match(src, lib.nhip_csm_match_dev)
    assert rc == rc2 == _lib.NHIP_OK
    assert ref.tobytes() == plain[0].tobytes() and np.array_equal(ref_sums, plain[1])
    rc, rc2, rec, s_ = match(src, lib.nhip_csm_match_gated_dev, -math.inf)
    assert rc == rc2 == _lib.NHIP_OK and rec.tobytes() == ref.tobytes() and np.array_equal(s_, ref_sums)
    rc, rc2, rec, s_ = match(src, lib.nhip_csm_match_gated_dev, float("nan"))
    assert rc == _lib.NHIP_ERR_ARG and rc2 == _lib.NHIP_OK
    assert np.all(rec.view(np.int32) == -7) and np.all(s_ == -7), "NaN: nothing is written"
    bad = np.array(src, np.int32)
    bad[5] = n_scans + 3
    rc, rc2, rec_u, s_u = match(bad, lib.nhip_csm_match_dev)
    assert rc == _lib.NHIP_OK and rc2 == _lib.NHIP_ERR_ARG and info[0] == 2
    assert rec_u["score"][5] == np.float32(LF) and s_u[5] == 0
    for m in (-5.0, LF):
        rc, rc2, rec, s_ = match(bad, lib.nhip_csm_match_gated_dev, m)
        assert rc == _lib.NHIP_OK and rc2 == _lib.NHIP_ERR_ARG and info[0] == 2 and info[3] == 5, list(info)
        want = gate(rec_u, s_u, m)
        assert rec.tobytes() == want[0].tobytes() and np.array_equal(s_, want[1]), m
        assert csm.rejected(rec)[5] == (m > LF)
    torch.cuda.synchronize()


def test_the_work_goes_away(gpu, lists):
    """Instrumented runs on the configs[3]-style list at -5: fewer candidate blocks refined and fewer blocks evaluated
    gated than ungated, and pairs settled right after their bounds."""
    wl, st, L = lists
    src, tgt, th0 = L["configs[3]-style"]
    grids, slot = _grids(st, tgt, 16)
    search = csm.search_spec(61, 81, 81, DEG, exact_score=True)
    env = {"NHIP_BNB_INSTRUMENT": "1", "NHIP_BNB_STATS": "1"}
    try:
        def run(m):
            csm.bnb_stats_levels()  # (reset)
            rec = csm.match_pairs(st, grids, src, slot, th0, search, min_score=m)
            assert csm.last_launch()["instrumented"]
            return rec, csm.bnb_stats_levels()
        (p, lv_p), (g, lv_g) = _with_env(env, lambda: (run(None), run(-5.0)))
        assert _same(g, gate(*p, -5.0))
        ev = lambda lv: lv["blocks_whole"] + lv["sub_blocks"] / 4
        assert lv_g["candidates_refined"] < lv_p["candidates_refined"], (lv_g, lv_p)
        assert ev(lv_g) < ev(lv_p)
        assert lv_p["pairs_settled_by_gate"] == 0 and lv_g["pairs_settled_by_gate"] >= 1
    finally:
        grids.close()


def test_cpp_adapter(gpu, lists, tmp_path):
    """CorrelativeScanMatcherBatch with and without min_score (adapters/gate_test.cc) returns what the Python gated call
    returns, pair for pair; a rejected pair is {-inf, (0, 0), 0}."""
    wl, st, L = lists
    src, tgt, th0 = L["configs[3]-style"]
    sel = np.arange(0, len(src), 10)
    src, tgt = src[sel], tgt[sel]
    clouds = sorted(set(src.tolist()) | set(tgt.tolist()))
    idx = {c: i for i, c in enumerate(clouds)}
    rot = wl.bag.odom[clouds, 2]
    with open(tmp_path / "clouds.txt", "w") as f:
        f.write("%d\n" % len(clouds))
        for c in clouds:
            pts = wl.bag.scans[c]
            f.write("%d\n" % len(pts))
            for x, y in np.asarray(pts, np.float32):
                f.write("%s %s\n" % (float(x).hex(), float(y).hex()))
    with open(tmp_path / "pairs.txt", "w") as f:
        f.write("%d\n" % len(src) + "".join("%d %d\n" % (idx[s], idx[t]) for s, t in zip(src, tgt)))
    with open(tmp_path / "rotations.txt", "w") as f:
        f.write("%d\n" % len(rot) + "".join("%s\n" % float(r).hex() for r in rot))
    with open(tmp_path / "params.txt", "w") as f:
        f.write("30 0.05 61 81 81 %s -5\n" % DEG.hex())
    adapters = os.path.join(ROOT, "nautilus_amd", "adapters")
    subprocess.check_call(["make", "-C", adapters, "gate_test"], stdout=subprocess.DEVNULL)
    p = subprocess.run([os.path.join(adapters, "gate_test"), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr

    def read(name):
        return np.array([[float.fromhex(v) for v in line.split()] for line in open(tmp_path / name)])

    cpp_plain, cpp_gated = read("ungated.txt"), read("gated.txt")
    # the Python side: the same clouds, pairs and headings through match_pairs
    th = csm.angle_mod(rot[[idx[s] for s in src]] - rot[[idx[t] for t in tgt]])
    ids = np.unique(tgt)
    spec = csm.grid_spec(30.0, 0.05, 2.0, 1e-10, 40, 16)
    search = csm.search_spec(61, 81, 81, DEG)
    grids = csm.LikelihoodGrids(st, ids, spec)
    try:
        slot = np.searchsorted(ids, tgt)
        py = {m: csm.match_pairs(st, grids, src, slot, th, search, min_score=m)[0] for m in (None, -5.0)}
    finally:
        grids.close()
    assert np.count_nonzero(csm.rejected(py[-5.0])) > 0
    for m, cpp in ((None, cpp_plain), (-5.0, cpp_gated)):
        for i, r in enumerate(py[m]):
            if csm.rejected(py[m])[i]:
                assert list(cpp[i]) == [-math.inf, 0.0, 0.0, 0.0], (m, i)
                continue
            tx, ty, t_ = csm.match_to_transform(r, spec, search, th[i])
            assert list(cpp[i]) == [float(r["score"]), float(tx), float(ty), float(t_)], (m, i, cpp[i], r)
    kept = ~csm.rejected(py[-5.0])
    assert np.array_equal(cpp_gated[kept], cpp_plain[kept])
