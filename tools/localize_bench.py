"""What localising scans in a finished map costs on the GPU, step by step: SynthBag(120), the map of its 60 even scans at their
TRUTH poses (HipBackend.occupancy_grid, the defaults: 1513 x 1500 cells), and --queries (1,000 and 10,000) queries: the bag's odd
scans in turn, each from a prior drawn up to 1 m and 10 degrees off its truth (seeded), on config #2's table and lattice.
localize.localize runs with a `timings` dict: the cells call, the window gathers, the table builds and the matches are each
timed on the host clock between two waits for the device (so the four add up to less than the call: uploads, downloads and
the host's bookkeeping are the rest, reported as wall_s).  Median and min-max of --runs runs after --warmup.
Also: ONE gather of every distinct origin of the list, timed by a pair of events on its stream (gather_all_ms), with the bytes
it must write, and hostside.map_windows on the same origins, once, on the same machine's CPU, its output compared.
Writes profiles/localize_bench.json.

  python tools/localize_bench.py [--queries 1000 10000] [--runs 5] [--warmup 1] [--out profiles/localize_bench.json]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, nargs="+", default=[1000, 10000])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-slots", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "localize_bench.json"))
    a = ap.parse_args()
    import torch
    from nautilus_amd import _lib, csm, hostside, localize, occupancy, posegraph, synth
    dev = torch.device("cuda:0")
    assert _lib.device_count() > 0, "localize_bench: no HIP device (a time is measured on the GPU or not at all)"
    bag = synth.SynthBag(120)
    even, odd = list(range(0, 120, 2)), list(range(1, 120, 2))
    mxy, moff = csm.pack_scans([bag.scans[i] for i in even])
    occ = occupancy.window_spec(bag.truth, 30.0)
    be = posegraph.HipBackend("cuda:0")
    grid = be.occupancy_grid(bag.truth[even], spec=occ, xy=mxy, offsets=moff)[0]
    gs = csm.grid_spec(30.0, 0.05, 2.0, 1e-10, 40, 16)
    mw = localize.spec(occ, gs)
    stat = lambda v: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
    out = {"note": "localize.localize on one MI355X, config #2's table (30 m / 0.05 m, 16-bit cells) and lattice (61 x 81 x 81): seconds "
                   "of the cells call, the window gathers, the table builds and the matches of ONE call, each on the host clock between "
                   "two waits for the device; wall_s is the whole call (uploads, downloads, host bookkeeping included); gather_all_ms is "
                   "one nhip_mapwin_gather_dev over every distinct origin, by a pair of events",
           "map_cells": [occ.width, occ.height], "map_cells_occupied": int((grid == 100).sum()), "runs": a.runs, "warmup": a.warmup,
           "max_slots": a.max_slots, "sizes": []}
    for n in a.queries:
        rng = np.random.default_rng(n)
        ids = [odd[k % len(odd)] for k in range(n)]
        d, r = rng.uniform(0.0, 2.0 * math.pi, n), rng.uniform(0.0, 1.0, n)
        priors = bag.truth[ids] + np.stack([r * np.cos(d), r * np.sin(d), np.radians(rng.uniform(-10.0, 10.0, n))], axis=1)
        qxy, qoff = csm.pack_scans([bag.scans[i] for i in ids])
        runs, walls, res = [], [], None
        for k in range(a.warmup + a.runs):
            t = {}
            t0 = time.perf_counter()
            res = localize.localize(qxy, qoff, priors, grid, mw, grid_spec=gs, max_slots=a.max_slots, timings=t)
            wall = time.perf_counter() - t0
            if k >= a.warmup:
                runs.append(t)
                walls.append(wall)
        e = res["poses"] - bag.truth[ids]
        uniq = np.unique(res["origins"], axis=0)
        # one gather of every distinct origin
        d_grid = torch.from_numpy(np.ascontiguousarray(grid)).to(dev)
        d_row_ptr, d_cols, d_stats = localize.map_cells_on_device(d_grid, mw)
        d_org = torch.from_numpy(uniq).to(dev)
        cap = len(uniq) * int(d_cols.numel())
        g_ms = []
        for k in range(a.warmup + a.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            d_wxy, d_woff, _ = localize.windows_on_device(d_row_ptr, d_cols, mw, d_org, len(uniq), cap, d_stats)
            e1.record()
            e1.synchronize()
            if k >= a.warmup:
                g_ms.append(e0.elapsed_time(e1))
        _lib.check(_lib.load().nhip_dev_status(None, None))
        woff = d_woff.cpu().numpy()
        t0 = time.perf_counter()
        hxy, hoff, _ = hostside.map_windows(grid, mw, uniq)
        host_s = time.perf_counter() - t0
        out["sizes"].append({
            "queries": n, "distinct_origins": int(len(uniq)), "source_points": int(len(qxy)),
            "points_per_window": [int(res["points_per_window"].min()), int(res["points_per_window"].max())],
            "cells_s": stat([t["cells"] for t in runs]), "gather_s": stat([t["gather"] for t in runs]),
            "build_s": stat([t["build"] for t in runs]), "match_s": stat([t["match"] for t in runs]), "wall_s": stat(walls),
            "gather_all_ms": stat(g_ms), "gather_all_points": int(woff[-1]),
            "gather_all_gb_per_s_written": float(8 * int(woff[-1]) / (1e6 * np.median(g_ms))),
            "hostside_map_windows_s": host_s,
            "gather_equals_hostside": bool(np.array_equal(woff, hoff) and d_wxy[:int(woff[-1])].cpu().numpy().tobytes() == hxy.tobytes()),
            "position_error_max_m": float(np.hypot(e[:, 0], e[:, 1]).max()),
            "heading_error_max_deg": float(np.degrees(np.abs(csm.angle_mod(e[:, 2]))).max()),
            "score_min": float(res["records"]["score"].min())})
        del d_wxy
        print(json.dumps(out["sizes"][-1]), flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
