"""Transient returns on the GPU (K19, nhip_transient.hip) against the numpy statement of the spec
(tests/transient_reference.py).  Everything the device computes after the cells is integer and the packing is a stable
compaction: labels, out_xy, out_offsets, out_index and stats are compared for EQUALITY of their bytes.  The cases are the ones
tests/test_transient_cpu.py holds hostside.transient_filter to: a handful of scans of at most a few hundred points in windows
of at most 64 x 64 cells, at the wave and workgroup seams of the ballot compaction, the clipped neighbourhoods, both threshold
edges, the int64 products, the invalid points and the bad offsets."""
import ctypes as C

import numpy as np
import pytest

from nautilus_amd import _lib, csm, occupancy, transient
from tests import occupancy_reference as OR
from tests import transient_reference as R

pytestmark = pytest.mark.gpu

BAD_MAP_SCAN_OFFSETS = 16384
CASES = R.shared_cases()


def product_spec(spec):
    return transient.spec(**{f: getattr(spec, f) for f in R.FIELDS})


@pytest.fixture(scope="module")
def wanted():
    """the reference's result of every shared case, computed once"""
    return {c[0]: R.transient_filter(*c[1:]) for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_device_equals_reference(gpu, wanted, case):
    """planes on the device: the call reads them and leaves them bit-unchanged"""
    import torch
    name, xy, off, poses, spec, hits, misses = case
    planes = tuple(torch.from_numpy(p.copy()).to("cuda:0") for p in (hits, misses))
    got = transient.filter(xy, off, poses, product_spec(spec), planes)
    R.same(got, wanted[name], name)
    assert planes[0].cpu().numpy().tobytes() == hits.tobytes() and planes[1].cpu().numpy().tobytes() == misses.tobytes()
    again = transient.filter(xy, off, poses, product_spec(spec), (hits, misses))  # host planes; the same bits every run
    for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes()


def test_threshold_edges_by_hand(gpu):
    for case, want in [R.case_thresholds()] + R.case_thresholds_one_above():
        name, xy, off, poses, spec, hits, misses = case
        assert transient.filter(xy, off, poses, product_spec(spec), (hits, misses)).labels.tolist() == want, name


@pytest.mark.parametrize("case", R.bad_offset_cases(), ids=[c[0] for c in R.bad_offset_cases()])
def test_bad_scan_offsets_are_empty_scans(gpu, case):
    """each kind is reported with kind 16384 and the offset at fault of the FIRST bad scan; the other scans and the planes
    are as without it"""
    import torch
    name, xy, off, poses, spec, hits, misses, bad, first = case
    s = product_spec(spec)
    with pytest.raises(_lib.NhipError, match="scan offset"):
        transient.filter(xy, off, poses, s, (hits, misses))
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    n_scans, n_points = len(off) - 1, len(xy)
    d_xy, d_off, d_aff, d_hits, d_misses = t(xy), t(off), t(transient.pose_affines(poses)), t(hits), t(misses)
    d_labels = torch.full((n_points,), 77, dtype=torch.uint8, device=dev)
    d_out_xy = torch.full((n_points, 2), -1.0, dtype=torch.float32, device=dev)
    d_out_off = torch.full((n_scans + 1,), -1, dtype=torch.int32, device=dev)
    d_out_idx = torch.full((n_points,), -1, dtype=torch.int32, device=dev)
    d_stats = torch.full((8,), -1, dtype=torch.int64, device=dev)
    lib = _lib.load()
    rc = lib.nhip_transient_filter_dev(d_xy.data_ptr(), d_off.data_ptr(), n_scans, n_points, d_aff.data_ptr(), C.byref(s),
                                       d_hits.data_ptr(), d_misses.data_ptr(), d_labels.data_ptr(), d_out_xy.data_ptr(),
                                       d_out_off.data_ptr(), d_out_idx.data_ptr(), d_stats.data_ptr(), None)
    info = (C.c_int32 * 4)()
    rc_status = lib.nhip_dev_status(None, info)
    assert rc == 0 and rc_status == _lib.NHIP_ERR_ARG and b"nhip_transient_filter_dev" in lib.nhip_last_error(), lib.nhip_last_error()
    assert list(info) == [BAD_MAP_SCAN_OFFSETS, BAD_MAP_SCAN_OFFSETS, first[0], first[1]]
    want = R.transient_filter(xy, off, poses, spec, hits, misses)
    assert want[4][5] == len(bad)
    out_off = d_out_off.cpu().numpy()
    kept = int(out_off[-1])
    got = (d_out_xy[:kept].cpu().numpy(), out_off, d_out_idx[:kept].cpu().numpy(), d_labels.cpu().numpy(), d_stats.cpu().numpy())
    R.same(got, want, name)
    assert (d_out_idx[kept:].cpu().numpy() == -1).all()  # nothing is written behind the kept points
    assert d_hits.cpu().numpy().tobytes() == hits.tobytes() and d_misses.cpu().numpy().tobytes() == misses.tobytes()
    assert lib.nhip_dev_status(None, info) == 0  # (the record was consumed)


def test_handle_form_equals_device_form(gpu, wanted):
    for name in ("seams", "invalid", "traced", "keep patterns"):
        _, xy, off, poses, spec, hits, misses = next(c for c in CASES if c[0] == name)
        scans = csm.ScanTable(xy, off)
        got = transient.filter_on_handle(scans, poses, product_spec(spec), (hits, misses))
        scans.close()
        R.same(got, wanted[name], name)


def test_in_stream_after_the_trace_on_a_second_stream(gpu):
    """nhip_occupancy_dev, then the filter, on a stream that is not the default one and with nothing waiting in between
    (transient.static_scans): the filter reads the planes the trace wrote.  Also the planes of the device trace stand in for
    the reference's in the shared case "traced"."""
    import torch
    name, xy, off, poses, occ = R.case_traced()
    want = R.static_scans(xy, off, poses, occ)
    s = occupancy.spec(**{f: getattr(occ, f) for f in OR.FIELDS})
    stream = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(stream):
        got = transient.static_scans(xy, off, poses, s)
        d_xy, d_off = torch.from_numpy(xy).to("cuda:0"), torch.from_numpy(off).to("cuda:0")
        on_dev = transient.static_scans_on_device(d_xy, d_off, len(off) - 1, poses, s, min_through=1)
    stream.synchronize()
    R.same(got[:5], want[:5], name)
    assert got.occupancy_stats.tobytes() == want[5].tobytes() and got.hits.tobytes() == want[6].tobytes() and got.misses.tobytes() == want[7].tobytes()
    assert got.stats[1] == 4  # the post of the first scan: seen through by the five others
    R.same(on_dev[:5], R.static_scans(xy, off, poses, occ, min_through=1)[:5], name + " min_through 1")
    # filter_on_device on the planes the trace returned
    f = transient.filter_on_device(d_xy, d_off, len(off) - 1, poses, transient.spec_from(s), (got.hits, got.misses))
    R.same(f, want[:5], name + " filter_on_device")
