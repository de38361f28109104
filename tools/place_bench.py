"""What the place descriptors cost (K16, nhip_place.hip): on the scans of configs[1]
(bench.Workload("weak", 1): 1,000 dense 1081-beam scans) and on a 10,000-scan bag (configs[3]'s size), every scan described
(nhip_place_describe_dev) and every scan matched against all the others (nhip_place_match_dev, the defaults: 10 rings, 5 records,
separation 20), each timed alone with hipEvents -- warm-up, then medians with min and max of the launches.  The 1,000-scan
records are compared with the numpy host path (hostside.place_candidates).  Writes profiles/place_bench.json.

  python tools/place_bench.py [--launches 20] [--warmup 3] [--big 10000] [--out profiles/place_bench.json]
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
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()), "launches": launches}


def measure(torch, xy, off, launches, warmup, flags=0):
    from nautilus_amd import _lib, place
    lib, dev = _lib.load(), torch.device("cuda:0")
    n = len(off) - 1
    spec = place.spec(flags=flags)
    d_xy, d_off = torch.from_numpy(xy).to(dev), torch.from_numpy(off).to(dev)
    d_ids = torch.arange(n, dtype=torch.int32, device=dev)
    d_desc = torch.empty((n, spec.n_rings), dtype=torch.int64, device=dev)
    d_bits = torch.empty(n, dtype=torch.int32, device=dev)
    ws = place.workspace_bytes(spec, n)
    d_ws = torch.empty(ws // 2, dtype=torch.int16, device=dev)
    d_rec = torch.empty((n, spec.top_k, 4), dtype=torch.int32, device=dev)
    d_stats = torch.empty(8, dtype=torch.int64, device=dev)
    sp = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def describe():
        _lib.check(lib.nhip_place_describe_dev(d_xy.data_ptr(), d_off.data_ptr(), n, C.byref(spec), d_desc.data_ptr(), d_bits.data_ptr(), sp))

    def match():
        _lib.check(lib.nhip_place_match_dev(d_desc.data_ptr(), d_bits.data_ptr(), n, d_ids.data_ptr(), n, C.byref(spec), d_rec.data_ptr(),
                                            d_stats.data_ptr(), d_ws.data_ptr(), ws, sp))

    res = {"n_scans": n, "n_points": int(off[-1]), "n_rings": spec.n_rings, "top_k": spec.top_k, "min_separation": spec.min_separation,
           "flags": flags, "workspace_bytes": int(ws), "query_rows_per_chunk": int(ws // (2 * ((n + 63) // 64 * 64)))}
    res["describe"] = timed(torch, describe, launches, warmup)
    res["match"] = timed(torch, match, launches, warmup)
    res["describe_again"] = timed(torch, describe, launches, warmup)
    _lib.check(lib.nhip_dev_status(sp, None))
    stats = d_stats.cpu().numpy()
    res["stats"] = dict(zip(place.STATS_FIELDS, (int(v) for v in stats)))
    # lane-operations by count, not measured: per admissible pair 64 shifts x R rings x (2 xor + 2 popcount-accumulate)
    res["pair_shift_ring_words"] = int(stats[1]) * 64 * spec.n_rings
    res["match_pairs_per_s"] = float(stats[1]) / (res["match"]["median_ms"] * 1e-3)
    return res, d_rec.cpu().numpy(), stats, spec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--big", type=int, default=10000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "place_bench.json"))
    a = ap.parse_args()
    import torch
    import bench
    from nautilus_amd import csm, hostside, place, synth
    t0 = time.perf_counter()
    out = {"note": "hipEvents around each call, every scan a query against all scans; describe = nhip_place_describe_dev, match = "
                   "nhip_place_match_dev (distance and top-K kernels, all chunks); median with min and max of the launches"}
    wl = bench.Workload("weak", 1)
    res, rec, stats, spec = measure(torch, wl.xy, wl.off, a.launches, a.warmup)
    t1 = time.perf_counter()
    want_rec, want_stats = hostside.place_candidates(wl.xy, wl.off, np.arange(wl.n_scans), spec)
    res["records_equal_host_path"] = bool(rec.tobytes() == want_rec.tobytes() and stats.tobytes() == want_stats.tobytes())
    res["host_path_s"] = time.perf_counter() - t1
    out["configs1_1000_scans"] = res
    out["configs1_1000_scans_past_only"] = measure(torch, wl.xy, wl.off, a.launches, a.warmup, place.NHIP_PLACE_PAST_ONLY)[0]
    if a.big:
        bag = synth.SynthBag(a.big, dense=True)
        xy, off = csm.pack_scans(bag.scans)
        out["%d_scans" % a.big] = measure(torch, xy, off, max(a.launches // 4, 3), 1)[0]
        out["%d_scans_past_only" % a.big] = measure(torch, xy, off, max(a.launches // 4, 3), 1, place.NHIP_PLACE_PAST_ONLY)[0]
    out["seconds"] = time.perf_counter() - t0
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
