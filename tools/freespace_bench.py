"""What the free-space check of match records costs (K15, nhip_freespace.hip): on configs[1]
(bench.Workload("weak", 1): 1,000 targets, 10,000 pairs, 16-bit cells, the headline's settings) the tables are built and the
list matched once, then the trace of the targets' free planes (nhip_freespace_trace_dev) and the check of the matcher's own
records (nhip_freespace_check_dev) are timed alone with hipEvents -- warm-up, then medians of 20 launches -- beside the
matcher step of the same session.  Writes profiles/freespace_bench.json.

  python tools/freespace_bench.py [--launches 20] [--warmup 3] [--out profiles/freespace_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, fn, launches, warmup):
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = np.array([a.elapsed_time(b) for a, b in ev])
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()),
            "spread_ms": float(ms.max() - ms.min()), "launches": launches}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "freespace_bench.json"))
    a = ap.parse_args()
    import torch
    import bench
    from nautilus_amd import _lib, freespace
    from tools.gate_bench import Match
    t0 = time.perf_counter()
    wl = bench.Workload("weak", 1)
    mt = Match(wl, (wl.src, wl.tgt, wl.th0), 16)
    m, lib = mt.m, mt.m.lib
    mt.run(None)
    torch.cuda.synchronize()
    spec = freespace.default_spec()
    d_free = torch.empty(freespace.planes_bytes(m.spec, m.n_targets), dtype=torch.uint8, device=m.d_grids.device)
    d_counts = torch.empty((m.n_pairs, 8), dtype=torch.int32, device=m.d_grids.device)

    def trace():
        _lib.check(lib.nhip_freespace_trace_dev(m.d_xy.data_ptr(), m.d_off.data_ptr(), m.n_scans, m.d_ids.data_ptr(), m.n_targets,
                                                C.byref(m.spec), m.d_grids.data_ptr(), d_free.data_ptr(), m.sp))

    def check():
        _lib.check(lib.nhip_freespace_check_dev(m.d_xy.data_ptr(), m.d_off.data_ptr(), m.n_scans, m.d_grids.data_ptr(), m.n_targets,
                                                C.byref(m.spec), m.d_src.data_ptr(), m.d_slot.data_ptr(), m.d_rot0.data_ptr(),
                                                m.d_delta.data_ptr(), None, m.n_pairs, C.byref(m.search), d_free.data_ptr(),
                                                m.d_out.data_ptr(), C.byref(spec), d_counts.data_ptr(), m.sp))

    res = {"note": "configs[1]: the matcher's own records (16-bit cells, NHIP_SEARCH_EXACT_SCORE), hipEvents around each launch; "
                   "trace = the free planes of every target, check = the eight counts of every pair; match = nhip_csm_match_dev "
                   "alone on the same tables in the same session",
           "n_targets": int(m.n_targets), "n_pairs": int(m.n_pairs), "hit_radius": spec.hit_radius, "end_margin": spec.end_margin,
           "planes_bytes": int(d_free.numel())}
    res["match"] = timed(torch, lambda: mt.run(None), a.launches, a.warmup)
    res["trace"] = timed(torch, trace, a.launches, a.warmup)
    res["check"] = timed(torch, check, a.launches, a.warmup)
    res["match_again"] = timed(torch, lambda: mt.run(None), a.launches, a.warmup)
    _lib.check(lib.nhip_dev_status(m.sp, None))
    c = d_counts.cpu().numpy().astype(np.int64)
    rec = m.d_out.cpu().numpy()
    score = rec.view(np.float32)[:, 3]
    share = freespace.violation_share(c)
    keep = freespace.keep(c)
    res["counts_sum"] = dict(zip(freespace.COUNT_FIELDS, (int(v) for v in c.sum(axis=0))))
    res["pairs_kept_at_default_gate"] = int(keep.sum())
    res["pairs_scoring_above_minus_5"] = int((score > -5.0).sum())
    res["pairs_above_minus_5_rejected_by_the_gate"] = int(((score > -5.0) & ~keep).sum())
    res["pairs_below_minus_5_kept_by_the_gate"] = int(((score <= -5.0) & keep).sum())
    res["share_percentiles_0_50_90_99_100"] = [float(np.percentile(share, p)) for p in (0, 50, 90, 99, 100)]
    res["seconds"] = time.perf_counter() - t0
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
