"""Match refinement on the GPU (K22): the refined records and the traces of nhip_refine_icp_dev equal the restatement
(tests/refine_reference.py) byte for byte on the shared case list -- source and target lengths at every pass, stage and
min_corr seam, iteration counts, one pair per flag, poisoned coordinates and normals, exact ties, a correspondence one float
either side of the threshold, the exhaustive search paths -- and the forms agree with each other."""
import ctypes as C

import numpy as np
import pytest
import torch

from nautilus_amd import _lib, refine
from tests import refine_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASE_NAMES = [c.name for c in R.cases()]


def same_bytes(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def status():
    info = (C.c_int32 * 4)()
    rc = _lib.load().nhip_dev_status(C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream), info)
    return rc, list(info)


class OnDevice:
    """A case's arrays as device tensors."""

    def __init__(self, cs, pair_src=None, pair_tgt=None):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        self.xy, self.normals, self.off = t(cs.xy), t(cs.normals), t(cs.offsets)
        if len(cs.xy) == 0:
            self.xy, self.normals = torch.zeros((1, 2), dtype=torch.float32, device=DEV), torch.zeros((1, 2), dtype=torch.float32, device=DEV)
        self.src = t(cs.pair_src if pair_src is None else np.asarray(pair_src, np.int32))
        self.tgt = t(cs.pair_tgt if pair_tgt is None else np.asarray(pair_tgt, np.int32))
        self.pose0 = t(cs.pose0)
        self.n_scans, self.n = len(cs.offsets) - 1, len(cs.pair_src)
        self.spec = refine.spec(**cs.spec_kw)

    def run(self, lo=0, hi=None):
        hi = self.n if hi is None else hi
        d_out, d_trace = refine.icp_on_device(self.xy, self.normals, self.off, self.n_scans, self.src[lo:hi], self.tgt[lo:hi],
                                              self.pose0[lo:hi], hi - lo, self.spec, trace=True)
        return d_out, d_trace


def fetch(d_out, d_trace):
    return refine.records_from(d_out), d_trace.cpu().numpy()


@pytest.mark.parametrize("name", CASE_NAMES)
def test_device_equals_the_restatement(name):
    cs = R.case(name)
    want, want_trace = R.reference(name)
    got, got_trace = fetch(*OnDevice(cs).run())
    assert status()[0] == _lib.NHIP_OK
    if not same_bytes(got, want):
        for f in got.dtype.names:
            assert same_bytes(got[f], want[f]), (f, got[f][:4], want[f][:4])
    assert same_bytes(got, want) and same_bytes(got_trace, want_trace)


def test_one_launch_equals_the_pairs_one_by_one():
    dev = OnDevice(R.case("pairs300"))
    whole, whole_trace = fetch(*dev.run())
    parts = [dev.run(i, i + 1) for i in range(dev.n)]
    single, single_trace = fetch(torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]))
    assert status()[0] == _lib.NHIP_OK
    assert same_bytes(whole, single) and same_bytes(whole_trace, single_trace)
    assert same_bytes(whole, R.reference("pairs300")[0])


def test_two_runs_give_the_same_bytes():
    for name in ("pairs300", "src4100", "far_target"):
        dev = OnDevice(R.case(name))
        a, b = fetch(*dev.run()), fetch(*dev.run())
        assert same_bytes(a[0], b[0]) and same_bytes(a[1], b[1])


@pytest.mark.parametrize("name", ["src2049", "tgt2048", "poison_target", "iter16", "skipped", "pairs300"])
def test_host_form_equals_the_device_form(name):
    cs = R.case(name)
    dev_out, dev_trace = fetch(*OnDevice(cs).run())
    out, trace = refine.icp(cs.xy, cs.normals, cs.offsets, cs.pair_src, cs.pair_tgt, cs.pose0, refine.spec(**cs.spec_kw), trace=True)
    assert same_bytes(out, dev_out) and same_bytes(trace, dev_trace)
    assert same_bytes(refine.icp(cs.xy, cs.normals, cs.offsets, cs.pair_src, cs.pair_tgt, cs.pose0, refine.spec(**cs.spec_kw)), dev_out)


def test_ids_out_of_range_cost_an_error_code_and_nothing_else():
    cs = R.case("pairs300")
    good, good_trace = fetch(*OnDevice(cs).run(0, 8))
    assert status()[0] == _lib.NHIP_OK
    src, tgt = cs.pair_src.copy(), cs.pair_tgt.copy()
    src[2], tgt[5], src[6] = len(cs.offsets) - 1, -1, 1 << 30
    got, got_trace = fetch(*OnDevice(cs, src, tgt).run(0, 8))
    rc, info = status()
    assert rc == _lib.NHIP_ERR_ARG and info[0] == refine.KIND_SCAN_ID and info[1] == refine.KIND_SCAN_ID
    assert info[3] in (2, 5, 6) and b"nhip_refine_icp_dev" in _lib.load().nhip_last_error()
    assert status()[0] == _lib.NHIP_OK  # (the record was consumed)
    for i in range(8):
        if i in (2, 5, 6):  # matches nothing: FEW, the start pose, zeros
            assert got["flags"][i] == refine.FEW and got["n_corr"][i] == 0 and got["iterations"][i] == 0
            assert same_bytes([got["c"][i], got["s"][i], got["tx"][i], got["ty"][i]], cs.pose0[i]) and not got_trace[i].any()
        else:
            assert same_bytes(got[i:i + 1], good[i:i + 1]) and same_bytes(got_trace[i], good_trace[i])
    with pytest.raises(_lib.NhipError):  # (the host form checks its ids on the host)
        refine.icp(cs.xy, cs.normals, cs.offsets, src[:8], tgt[:8], cs.pose0[:8])


def test_no_pairs_and_no_trace():
    cs = R.case("iter1")
    dev = OnDevice(cs)
    d_out = refine.icp_on_device(dev.xy, dev.normals, dev.off, dev.n_scans, dev.src, dev.tgt, dev.pose0, 1, dev.spec)
    assert same_bytes(refine.records_from(d_out), R.reference("iter1")[0])
    assert len(refine.icp_on_device(dev.xy, dev.normals, dev.off, dev.n_scans, dev.src, dev.tgt, dev.pose0, 0, dev.spec)) == 0
    assert status()[0] == _lib.NHIP_OK
