"""Range signatures on the GPU (K21): anchors, map signatures, scan signatures and records bit-equal to the slow statement of the
spec (tests/rangesig_reference.py) at the smallest shapes that can go wrong, the capacity rule, a grid at an odd address, a
crafted ray table, crafted bytes through the match, the smallest workspace, and the host form."""
import ctypes as C

import numpy as np
import pytest

from nautilus_amd import _lib, rangesig
from tests import rangesig_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MAP_CASES, MATCH_CASES = R.map_cases(), R.match_cases()


def product_spec(spec):
    s = rangesig.default_spec()
    for f in R.FIELDS:
        setattr(s, f, getattr(spec, f))
    return s


def status(torch):
    info = (C.c_int32 * 4)()
    rc = _lib.load().nhip_dev_status(C.c_void_p(torch.cuda.current_stream().cuda_stream), info)
    return rc, list(info)


def device_map(torch, grid, ps, rays=None, max_anchors=None, d_grid=None):
    """anchors and map signatures through the two _dev calls: (anchors, sig, stats, status) as host arrays"""
    d_grid = torch.from_numpy(np.ascontiguousarray(grid, dtype=np.int8)).to(DEV) if d_grid is None else d_grid
    d_anchors, d_stats, n = rangesig.anchors_on_device(d_grid, ps, max_anchors)
    d_rays = None if rays is None else torch.tensor(rays, dtype=torch.int32, device=DEV)
    d_sig = rangesig.map_signatures_on_device(d_grid, ps, d_anchors, n, d_stats, d_rays)
    st = status(torch)
    return d_anchors[:n].cpu().numpy(), d_sig[:n].cpu().numpy(), d_stats.cpu().numpy(), st


@pytest.mark.parametrize("case", MAP_CASES, ids=[c[0] for c in MAP_CASES])
def test_anchors_and_map_signatures_equal_reference(gpu, case):
    import torch
    name, grid, spec, rays = case
    ps = product_spec(spec)
    want_a, want_sig, want_stats = R.map_results()[name]
    a, sig, stats, st = device_map(torch, grid, ps, rays)
    assert st[0] == _lib.NHIP_OK, st
    assert np.array_equal(a, want_a) and a.shape == want_a.shape, name
    assert sig.tobytes() == want_sig.tobytes(), (name, np.argwhere(sig != want_sig)[:5])
    assert stats.tolist() == want_stats.tolist(), name
    assert stats[3:6].sum() == 64 * spec.rays_per_sector * len(want_a)  # every ray of every anchor ends in one of the three ways
    # the grid tensor at an odd byte offset: the same bits
    buf = torch.zeros(grid.size + 3, dtype=torch.int8, device=DEV)
    odd = buf[1:1 + grid.size].view(spec.height, spec.width)
    odd.copy_(torch.from_numpy(np.ascontiguousarray(grid, dtype=np.int8)))
    assert odd.data_ptr() % 2 == 1
    a2, sig2, stats2, st2 = device_map(torch, grid, ps, rays, d_grid=odd)
    assert st2[0] == _lib.NHIP_OK and a2.tobytes() == a.tobytes() and sig2.tobytes() == sig.tobytes() and stats2.tolist() == stats.tolist()


@pytest.mark.parametrize("short", [0, 1])
def test_max_anchors_exact_and_one_short(gpu, short):
    import torch
    name, grid, spec, rays = next(c for c in MAP_CASES if c[0] == "rooms 37x29 stride 3 m 2 L 7")
    ps = product_spec(spec)
    n_all = len(R.map_results()[name][0])
    cap = n_all - short
    want_a, want_sig, want_stats = R.anchors_and_signatures(grid, spec, rays, max_anchors=cap)
    a, sig, stats, st = device_map(torch, grid, ps, rays, max_anchors=cap)
    assert np.array_equal(a, want_a) and sig.tobytes() == want_sig.tobytes() and stats.tolist() == want_stats.tolist()
    if short:
        assert st[0] == _lib.NHIP_ERR_ARG and st[1][1] == rangesig.KIND_ANCHORS and st[1][2] == n_all and st[1][3] == cap and stats[2] == 1
    else:
        assert st[0] == _lib.NHIP_OK and stats[2] == 0
    # a capacity above the anchors found: the entries behind them are four -1, their signatures 255, and they are in no record
    d_grid = torch.from_numpy(grid).to(DEV)
    d_anchors, d_stats, n = rangesig.anchors_on_device(d_grid, ps, n_all + 70)
    d_sig = rangesig.map_signatures_on_device(d_grid, ps, d_anchors, n, d_stats)
    assert status(torch)[0] == _lib.NHIP_OK
    assert (d_anchors[n_all:].cpu().numpy() == -1).all() and (d_sig[n_all:].cpu().numpy() == 255).all()
    full = R.map_results()[name]
    assert d_sig[:n_all].cpu().numpy().tobytes() == full[1].tobytes() and d_stats.cpu().numpy().tolist() == full[2].tolist()
    q = torch.from_numpy(full[1][:3].copy()).to(DEV)
    rec, _ = rangesig.match_on_device(q, 3, d_sig, d_anchors, n, ps, d_stats)
    want, _ = R.match(full[1][:3], full[1], full[0], spec)
    assert status(torch)[0] == _lib.NHIP_OK and np.array_equal(rec.cpu().numpy(), want)


def test_ray_table_entries_are_checked(gpu):
    """an entry of a table in device memory that is not a ray ends at once (255), is reported, and nothing is read outside"""
    import torch
    name, grid, spec, rays = next(c for c in MAP_CASES if c[0] == "rdiv halves")
    ps = product_spec(spec)
    bad = [list(r) for r in rays]
    bad[3] = [4, 2, 0, 30000]            # no step
    bad[5] = [10 ** 6, 2, 4, 30000]      # a step beyond n
    bad[7] = [4, 2, 4, 2 ** 30]          # k scale beyond 2^31
    bad[9] = [4, 2, 10 ** 6, 1]          # longer than any ray
    a, sig, stats, st = device_map(torch, grid, ps, bad)
    assert st[0] == _lib.NHIP_ERR_ARG and st[1][1] == rangesig.KIND_ANCHORS and st[1][3] in (3, 5, 7, 9)
    want = R.map_results()[name][1].copy()
    want[:, [3, 5, 7, 9]] = 255
    assert sig.tobytes() == want.tobytes() and stats[3:6].sum() == 64 * len(a)
    assert device_map(torch, grid, ps, rays)[3][0] == _lib.NHIP_OK  # (the next call is not affected)


def test_scan_signatures_equal_reference(gpu):
    import torch
    xy, off, spec = R.scan_case()
    ps = product_spec(spec)
    d_xy, d_off = torch.from_numpy(xy).to(DEV), torch.from_numpy(off).to(DEV)
    got = rangesig.scan_signatures_on_device(d_xy, d_off, len(off) - 1, ps).cpu().numpy()
    assert status(torch)[0] == _lib.NHIP_OK
    want = R.scan_result()
    assert got.tobytes() == want.tobytes(), np.argwhere(got != want)[:5]
    assert want[7, 31] == 0 and want[7, 32] == 8  # the origin in sector 31; (-1, +-0) in sector 32, 1 m = 8 units
    assert (want[0] == 255).all() and (want[1] != 255).sum() == 1 and (want[6] != 255).all()
    # offsets that are not a scan: all 255, reported, the other scans as they were
    bad = off.copy()
    bad[3] = -5
    got = rangesig.scan_signatures_on_device(d_xy, torch.from_numpy(bad).to(DEV), len(off) - 1, ps).cpu().numpy()
    rc, info = status(torch)
    assert rc == _lib.NHIP_ERR_ARG and info[1] == 16384 and info[2] == -5
    assert (got[2] == 255).all() and (got[3] == 255).all() and got[4:].tobytes() == want[4:].tobytes() and got[:2].tobytes() == want[:2].tobytes()
    assert rangesig.scan_signatures_on_device(d_xy, d_off, 0, ps).shape == (1, 64) and status(torch)[0] == _lib.NHIP_OK


@pytest.mark.parametrize("case", MATCH_CASES, ids=[c[0] for c in MATCH_CASES])
def test_match_on_crafted_bytes_equals_reference(gpu, case):
    import torch
    name, qs, ms, an, spec = case
    ps = product_spec(spec)
    want, (none, written) = R.match_results()[name]
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if a.size else torch.zeros((1,) + a.shape[1:], dtype=dt, device=DEV)
    d_q, d_m, d_a = t(qs, torch.uint8), t(ms, torch.uint8), t(an, torch.int32)
    rec, stats = rangesig.match_on_device(d_q, len(qs), d_m, d_a, len(ms), ps)
    assert status(torch)[0] == _lib.NHIP_OK
    assert np.array_equal(rec.cpu().numpy(), want), name
    assert stats.cpu().numpy()[6:].tolist() == [none, written]
    # the smallest workspace -- one row of keys -- against the full one: the same records
    one_row = 4 * ((max(len(ms), 1) + 63) // 64 * 64)
    rec1, stats1 = rangesig.match_on_device(d_q, len(qs), d_m, d_a, len(ms), ps, workspace=one_row)
    assert status(torch)[0] == _lib.NHIP_OK and np.array_equal(rec1.cpu().numpy(), want) and stats1.cpu().numpy()[6:].tolist() == [none, written]


def test_host_form_equals_dev_form(gpu):
    import torch
    name, grid, spec, rays = next(c for c in MAP_CASES if c[0] == "rooms 37x29 stride 3 m 4 L 600")
    ps = product_spec(spec)
    xy, off, _ = R.scan_case()
    dev = rangesig.candidates(grid, ps, xy, off, DEV)
    n = dev["n_anchors"]
    want_a, want_sig, want_stats = R.map_results()[name]
    assert n == len(want_a) and np.array_equal(dev["anchors"], want_a) and dev["map_sig"].tobytes() == want_sig.tobytes()
    assert dev["scan_sig"].tobytes() == R.scan_result().tobytes()
    want_rec, (none, written) = R.match(dev["scan_sig"], want_sig, want_a, spec)
    assert np.array_equal(dev["records"], want_rec) and dev["stats"].tolist() == want_stats[:6].tolist() + [none, written]
    for cap in (n, n + 9, n - 1):
        host = rangesig.candidates_host_form(grid, ps, xy, off, cap)
        rc, info = status(torch)
        if cap >= n:
            assert rc == _lib.NHIP_OK
            for k in ("records", "anchors", "map_sig", "scan_sig", "stats"):
                assert np.asarray(host[k]).tobytes() == np.asarray(dev[k]).tobytes(), (k, cap)
        else:
            assert rc == _lib.NHIP_ERR_ARG and info[1] == rangesig.KIND_ANCHORS and host["n_anchors"] == cap and host["stats"][2] == 1
            assert np.array_equal(host["records"], R.match(dev["scan_sig"], want_sig[:cap], want_a[:cap], spec)[0])
