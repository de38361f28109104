"""The loop-closure pair gate at one-ulp threshold edges: pairs of poses whose float distance is the last float that passes
`dist < max_range` or the first that does not (tests/threshold_edges.py), beside pairs at the same offsets that fail on
separation alone and pairs with a == b.  Host-pointer form at 128 thresholds, device-pointer form at the eight named ones."""
import ctypes as C

import numpy as np
import pytest

from nautilus_amd import _lib, posegraph
from tests import threshold_edges as E

pytestmark = pytest.mark.gpu


def _report(what, results):
    n_cases = sum(r[1] for r in results)
    flipped = [(T, f) for T, _, f, _ in results if f]
    failed = [T for T, _, _, same in results if not same]
    print("%s: %d of %d designed pairs decided differently from the oracle, at %d of %d thresholds %s" % (
        what, sum(f for _, f in flipped), n_cases, len(failed), len(results), flipped[:8]))
    assert not failed and n_cases >= 12 * len(results)


def _flipped(c, got):
    lo, a, b = c["is_lo"], c["a"], c["b"]
    return int((got[a, b].astype(bool) != lo).sum() + (got[b, a].astype(bool) != lo).sum())


def test_pair_gate_at_threshold_edges(gpu):
    be = posegraph.HipBackend()
    results = []
    for T in E.thresholds():
        c, want, n_live = E.pair_gate_case(T)  # (asserts both roots and 100 % live cases)
        got = be.pair_gate(c["poses"], c["cand"], T, c["min_sep"])
        results.append((T, 2 * n_live, _flipped(c, got), got.tobytes() == want.tobytes()))
    _report("pair gate, host pointers", results)


def test_pair_gate_dev_at_threshold_edges(gpu):
    import torch
    lib, dev = _lib.load(), torch.device("cuda:0")
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    results = []
    for T in E.NAMED:
        c, want, n_live = E.pair_gate_case(T)
        d_p, d_c = torch.from_numpy(c["poses"]).to(dev), torch.from_numpy(c["cand"]).to(dev)
        d_f = torch.full((len(c["cand"]) ** 2,), 7, dtype=torch.uint8, device=dev)
        _lib.check(lib.nhip_lc_pair_gate_dev(d_p.data_ptr(), len(c["poses"]), d_c.data_ptr(), len(c["cand"]), T, c["min_sep"], d_f.data_ptr(), sp))
        _lib.check(lib.nhip_dev_status(sp, None))
        got = d_f.cpu().numpy().reshape(want.shape)
        results.append((T, 2 * n_live, _flipped(c, got), got.tobytes() == want.tobytes()))
    _report("pair gate, device pointers", results)
