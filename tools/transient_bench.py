"""What the transient-returns filter (K19, nhip_transient_filter_dev) costs: SynthBag at --scans scans (2,000) at its TRUTH
poses with --movers walkers (2) on the robot's own loop, the defaults, the window of every pose +- 30 m.  The scans and the
planes (one nhip_occupancy_dev trace, not timed here) are on the device; each call of the filter alone is timed by a pair of
events on its stream around --batch calls back to back (filter_ms: per call; the two clears and the three kernels, nothing else), and the pair trace + filter in-stream as
transient.static_scans_on_device runs it on the host clock (static_scans_ms: enqueue, status check, downloads included).
Median and min-max of --calls calls after --warmup.  The yardstick is hostside.transient_filter, the numpy statement of the same
spec, once, in one process on the same machine's CPU, on the same input; its five outputs are compared with the device's.
Also reported: the bytes the call must move at least (every label cleared, written and read; every point read; every kept
point read again and written with its index; the plane gathers are left out -- neighbouring beams share their cells' lines)
over filter_ms.
Writes profiles/transient_bench.json.

  python tools/transient_bench.py [--scans 2000] [--movers 2] [--calls 30] [--warmup 5] [--batch 50] [--out profiles/transient_bench.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=2000)
    ap.add_argument("--movers", type=int, default=2)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=50, help="calls of the filter between one pair of events")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transient_bench.json"))
    a = ap.parse_args()
    import torch
    from nautilus_amd import _lib, csm, hostside, occupancy, synth, transient
    lib, dev = _lib.load(), torch.device("cuda:0")
    assert _lib.device_count() > 0, "transient_bench: no HIP device (a time is measured on the GPU or not at all)"
    bag = synth.SynthBag(a.scans)
    n = a.scans
    walkers = [((lambda k: (lambda i: tuple(bag.truth[(2 * i + 15 + 40 * k) % n, :2])))(k), 0.3) for k in range(a.movers)]
    scans, masks = synth.add_movers(bag.scans, bag.truth, walkers)
    xy, off = csm.pack_scans(scans)
    mover = np.concatenate(masks)
    poses = bag.truth
    occ = occupancy.window_spec(poses, 30.0)
    spec = transient.spec_from(occ)
    d_xy, d_off = torch.from_numpy(xy).to(dev), torch.from_numpy(off).to(dev)
    grid, hits, misses, occ_stats = occupancy.occupancy_grid_on_device(d_xy, d_off, n, poses, occ)
    d_hits, d_misses = torch.from_numpy(hits).to(dev), torch.from_numpy(misses).to(dev)
    d_aff = torch.from_numpy(transient.pose_affines(poses)).to(dev)
    out_t = transient._outputs(torch, dev, n, len(xy))
    sp = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def filter_ms():  # (a.batch calls back to back between the two events: one call is too short a window to time)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.batch):
            transient._enqueue(lib, d_xy, d_off, n, len(xy), d_aff, spec, d_hits, d_misses, out_t, sp)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.batch

    def static_ms():
        t0 = time.perf_counter()
        transient.static_scans_on_device(d_xy, d_off, n, poses, occ)
        return 1e3 * (time.perf_counter() - t0)

    for _ in range(a.warmup):
        filter_ms()
        static_ms()
    f_ms = np.array([filter_ms() for _ in range(a.calls)])
    _lib.check(lib.nhip_dev_status(sp, None))
    got = transient._download(out_t, len(xy))
    s_ms = np.array([static_ms() for _ in range(a.calls)])
    t0 = time.perf_counter()
    want = hostside.transient_filter(xy, off, poses, spec, hits, misses)
    host_s = time.perf_counter() - t0
    stat = lambda v: {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())}
    kept = int(got.offsets[-1])
    # the labels' clear and their write, a read of every point and label, a second read and a 12-byte write of every kept point
    least_bytes = int(len(xy) * (1 + 1 + 8 + 1) + kept * (8 + 12))
    flagged = got.labels == 1
    out = {
        "note": "nhip_transient_filter_dev on scans and planes already on the device: filter_ms per call, by a pair of events on the "
                "call's stream around `batch` calls back to back; static_scans_ms is transient.static_scans_on_device (occupancy trace + filter "
                "in-stream, allocation, status check and downloads included) on the host clock; the reference is "
                "hostside.transient_filter (numpy) once in one process on the same machine's CPU",
        "n_scans": n, "n_points": int(len(xy)), "movers": a.movers, "mover_returns": int(mover.sum()), "poses": "truth",
        "window_cells": [occ.width, occ.height], "support_radius": spec.support_radius, "min_through": spec.min_through,
        "transient_permille": spec.transient_permille, "stats": [int(v) for v in got.stats],
        "mover_share_flagged": float(flagged[mover].mean()) if mover.any() else None,
        "other_share_flagged": float(flagged[~mover].mean()),
        "calls": a.calls, "warmup": a.warmup, "batch": a.batch,
        "filter_ms": stat(f_ms), "static_scans_ms": stat(s_ms),
        "least_bytes": least_bytes, "least_bytes_gb_per_s": float(least_bytes / (1e6 * np.median(f_ms))),
        "hostside_s": host_s, "hostside_over_filter": float(1e3 * host_s / np.median(f_ms)),
        "outputs_equal_hostside": bool(all(g.tobytes() == w.tobytes() for g, w in zip(got, want))),
    }
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
