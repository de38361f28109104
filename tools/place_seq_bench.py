"""What the place sequences cost (K16b, nhip_place_seq.hip): on the two workloads of
tools/place_bench.py -- the scans of configs[1] (bench.Workload("weak", 1): 1,000 dense 1081-beam scans) and a 10,000-scan bag --
every scan matched against all the others by nhip_place_seq_match_dev at W = 0, 2 and 8 (step 1; 10 rings, 5 records, separation
20), beside nhip_place_match_dev on the same descriptors in the same process: each timed alone with hipEvents, warm-up, then
medians with min and max of the launches.  The 1,000-scan records are compared with the numpy host path
(hostside.place_sequence_candidates).  Writes profiles/place_seq_bench.json.

  python tools/place_seq_bench.py [--launches 20] [--warmup 3] [--big 10000] [--out profiles/place_seq_bench.json]
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

WINDOWS = (0, 2, 8)


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


def measure(torch, xy, off, launches, warmup, flags=0, compare=False):
    from nautilus_amd import _lib, hostside, place
    lib, dev = _lib.load(), torch.device("cuda:0")
    n = len(off) - 1
    spec = place.spec(flags=flags)
    d_xy, d_off = torch.from_numpy(xy).to(dev), torch.from_numpy(off).to(dev)
    d_ids = torch.arange(n, dtype=torch.int32, device=dev)
    d_desc, d_bits = place.describe_on_device(d_xy, d_off, n, spec)
    d_stats = torch.empty(8, dtype=torch.int64, device=dev)
    sp = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    res = {"n_scans": n, "n_rings": spec.n_rings, "top_k": spec.top_k, "min_separation": spec.min_separation, "flags": flags}

    ws1 = place.workspace_bytes(spec, n)
    d_ws1 = torch.empty(ws1 // 2, dtype=torch.int16, device=dev)
    d_rec1 = torch.empty((n, spec.top_k, 4), dtype=torch.int32, device=dev)

    def single():
        _lib.check(lib.nhip_place_match_dev(d_desc.data_ptr(), d_bits.data_ptr(), n, d_ids.data_ptr(), n, C.byref(spec), d_rec1.data_ptr(),
                                            d_stats.data_ptr(), d_ws1.data_ptr(), ws1, sp))

    res["place_match"] = timed(torch, single, launches, warmup)
    single_stats = d_stats.cpu().numpy().copy()
    d_rec = torch.empty((n, spec.top_k, 8), dtype=torch.int32, device=dev)
    for W in WINDOWS:
        seq = place.seq_spec(half_window=W)
        ws = place.seq_workspace_bytes(spec, seq, n, n)
        d_ws = torch.empty(ws // 2, dtype=torch.int16, device=dev)
        row = 2 * ((n + 63) // 64 * 64)

        def sequence():
            _lib.check(lib.nhip_place_seq_match_dev(d_desc.data_ptr(), d_bits.data_ptr(), n, d_ids.data_ptr(), n, C.byref(spec), C.byref(seq),
                                                    d_rec.data_ptr(), d_stats.data_ptr(), d_ws.data_ptr(), ws, sp))

        r = timed(torch, sequence, launches, warmup)
        _lib.check(lib.nhip_dev_status(sp, None))
        stats = d_stats.cpu().numpy()
        r["workspace_bytes"] = int(ws)
        r["query_scans_per_chunk"] = n if ws >= n * 2 * row else int((ws - 2 * W * row) // (2 * row))
        r["stats"] = dict(zip(place.SEQ_STATS_FIELDS, (int(v) for v in stats)))
        r["ratio_to_place_match"] = r["median_ms"] / res["place_match"]["median_ms"]
        # by count, not measured: the plane is n x n single distances (64 shifts x R rings each); a window is 2 (2W + 1) key reads a pair
        r["plane_pairs"], r["window_key_reads"] = n * n, int(stats[1]) * 2 * (2 * W + 1)
        if W == 0:
            rec = d_rec.cpu().numpy()
            r["fields_0_3_equal_place_match"] = bool(rec[:, :, :4].tobytes() == d_rec1.cpu().numpy().tobytes() and
                                                     stats[:6].tobytes() == single_stats[:6].tobytes())
        if compare and W:
            t1 = time.perf_counter()
            want_rec, want_stats = hostside.place_sequence_candidates(xy, off, np.arange(n), spec, seq)
            r["records_equal_host_path"] = bool(d_rec.cpu().numpy().tobytes() == want_rec.tobytes() and stats.tobytes() == want_stats.tobytes())
            r["host_path_s"] = time.perf_counter() - t1
        res["W%d" % W] = r
        del d_ws
    res["place_match_again"] = timed(torch, single, launches, warmup)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--big", type=int, default=10000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "place_seq_bench.json"))
    a = ap.parse_args()
    import torch
    import bench
    from nautilus_amd import csm, place, synth
    t0 = time.perf_counter()
    out = {"note": "hipEvents around each call, every scan a query against all scans; place_match = nhip_place_match_dev, W* = "
                   "nhip_place_seq_match_dev (plane, window and top-K kernels, all chunks) at that half window, step 1; median with min "
                   "and max of the launches"}
    wl = bench.Workload("weak", 1)
    out["configs1_1000_scans"] = measure(torch, wl.xy, wl.off, a.launches, a.warmup, compare=True)
    out["configs1_1000_scans_past_only"] = measure(torch, wl.xy, wl.off, a.launches, a.warmup, place.NHIP_PLACE_PAST_ONLY)
    if a.big:
        bag = synth.SynthBag(a.big, dense=True)
        xy, off = csm.pack_scans(bag.scans)
        out["%d_scans" % a.big] = measure(torch, xy, off, max(a.launches // 4, 3), 1)
        out["%d_scans_past_only" % a.big] = measure(torch, xy, off, max(a.launches // 4, 3), 1, place.NHIP_PLACE_PAST_ONLY)
    out["seconds"] = time.perf_counter() - t0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
