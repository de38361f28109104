"""What global localisation costs on the GPU, step by step: SynthBag(400), the map of its 200 even scans at their TRUTH poses
(HipBackend.occupancy_grid, the defaults: 1843 x 1544 cells), and --queries (1,000 and 10,000) queries without priors: the bag's
odd scans in turn.  The four range-signature calls (nhip_rangesig_anchors_dev + nhip_rangesig_map_dev: map_ms;
nhip_rangesig_scans_dev: scans_ms; nhip_rangesig_match_dev: match_ms) are each timed by a pair of events on their stream;
candidates_s is rangesig.candidates on the host clock (uploads, the anchor count, downloads included) and wall_s the whole
relocalize.global_localize call, the K matches per query at config #2's table and lattice included.  Median and min-max of
--runs runs after --warmup.  Beside them hostside's time for the same work, once, on the same machine's CPU: range_signatures
on the same map, scan_signatures on all queries, signature_candidates on the first --host-queries queries (its time grows with
the queries: the per-query figure is what to compare), their outputs compared with the device's.
Writes profiles/relocalize_bench.json.

  python tools/relocalize_bench.py [--queries 1000 10000] [--runs 5] [--warmup 1] [--out profiles/relocalize_bench.json]
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
    ap.add_argument("--queries", type=int, nargs="+", default=[1000, 10000])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-queries", type=int, default=100)
    ap.add_argument("--whole-call-max", type=int, default=10000, help="no whole global_localize call above this many queries")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relocalize_bench.json"))
    a = ap.parse_args()
    import torch
    from nautilus_amd import _lib, csm, hostside, occupancy, posegraph, rangesig, relocalize, synth
    dev = torch.device("cuda:0")
    assert _lib.device_count() > 0, "relocalize_bench: no HIP device (a time is measured on the GPU or not at all)"
    bag = synth.SynthBag(400)
    even, odd = list(range(0, 400, 2)), list(range(1, 400, 2))
    mxy, moff = csm.pack_scans([bag.scans[i] for i in even])
    occ = occupancy.window_spec(bag.truth, 30.0)
    be = posegraph.HipBackend("cuda:0")
    grid = be.occupancy_grid(bag.truth[even], spec=occ, xy=mxy, offsets=moff)[0]
    spec = rangesig.spec(occ, flags=_lib.NHIP_RANGESIG_UNKNOWN_STOPS)
    stat = lambda v: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return r, e0.elapsed_time(e1)
    t0 = time.perf_counter()
    h_anchors, h_map, h_stats = hostside.range_signatures(grid, spec)
    host_map_s = time.perf_counter() - t0
    out = {"note": "global localisation on one MI355X: the range-signature calls by pairs of events (ms), rangesig.candidates and the "
                   "whole relocalize.global_localize call (config #2's table and lattice, K = 5 matches per query) on the host clock (s); "
                   "hostside_* is the numpy statement of the same work, once, on the same machine's CPU",
           "map_cells": [occ.width, occ.height], "map_cells_occupied": int((grid == 100).sum()), "anchors": int(len(h_anchors)),
           "lattice_nodes": int(h_stats[0]), "rays": int(h_stats[3:6].sum()), "runs": a.runs, "warmup": a.warmup,
           "hostside_range_signatures_s": host_map_s, "sizes": []}
    d_grid = torch.from_numpy(np.ascontiguousarray(grid)).to(dev)
    d_rays = torch.from_numpy(rangesig.tables(spec)[0]).to(dev)
    for n in a.queries:
        ids = [odd[k % len(odd)] for k in range(n)]
        qxy, qoff = csm.pack_scans([bag.scans[i] for i in ids])
        d_xy, d_off = torch.from_numpy(qxy).to(dev), torch.from_numpy(qoff).to(dev)
        ms = {"map": [], "scans": [], "match": []}
        cand_s, walls, res = [], [], None
        A = len(h_anchors)
        for k in range(a.warmup + a.runs):
            def map_calls():
                d_an, d_st, _ = rangesig.anchors_on_device(d_grid, spec, A)
                return d_an, d_st, rangesig.map_signatures_on_device(d_grid, spec, d_an, A, d_st, d_rays)
            (d_an, d_st, d_map), t_map = timed(map_calls)
            d_scan, t_scans = timed(lambda: rangesig.scan_signatures_on_device(d_xy, d_off, n, spec))
            # (the key workspace is allocated outside the pair of events)
            ws = rangesig.workspace_bytes(spec, A, n)
            d_ws = torch.empty(ws // 4, dtype=torch.int32, device=dev)
            d_rec = torch.empty((n, int(spec.top_k), 4), dtype=torch.int32, device=dev)
            sp = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            _, t_match = timed(lambda: _lib.check(_lib.load().nhip_rangesig_match_dev(
                d_scan.data_ptr(), n, d_map.data_ptr(), d_an.data_ptr(), A, C.byref(spec), d_rec.data_ptr(), d_st.data_ptr(), d_ws.data_ptr(),
                ws, sp)))
            _lib.check(_lib.load().nhip_dev_status(None, None))
            t0 = time.perf_counter()
            c = rangesig.candidates(d_grid, spec, qxy, qoff)
            t_cand = time.perf_counter() - t0
            wall = None
            if n <= a.whole_call_max:
                t0 = time.perf_counter()
                res = relocalize.global_localize(qxy, qoff, d_grid, occ, spec=spec)
                wall = time.perf_counter() - t0
            if k >= a.warmup:
                ms["map"].append(t_map), ms["scans"].append(t_scans), ms["match"].append(t_match), cand_s.append(t_cand)
                if wall is not None:
                    walls.append(wall)
        hq = min(a.host_queries, n)
        t0 = time.perf_counter()
        h_scan = hostside.scan_signatures(qxy, qoff, spec)
        host_scan_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        h_rec, _ = hostside.signature_candidates(h_scan[:hq], h_map, h_anchors, spec)
        host_match_s = time.perf_counter() - t0
        size = {"queries": n, "source_points": int(len(qxy)), "anchors": A, "key_workspace_bytes": int(ws),
                "map_ms": stat(ms["map"]), "scans_ms": stat(ms["scans"]), "match_ms": stat(ms["match"]),
                "match_sad_bytes_per_s": float(n) * A * 64 * 64 / (1e-3 * float(np.median(ms["match"]))),
                "candidates_s": stat(cand_s), "wall_s": stat(walls) if walls else None,
                "hostside_scan_signatures_s": host_scan_s, "hostside_signature_candidates_s": host_match_s,
                "hostside_signature_candidates_queries": hq, "hostside_signature_candidates_s_per_query": host_match_s / max(hq, 1),
                "device_equals_hostside": bool(np.array_equal(c["anchors"], h_anchors) and c["map_sig"].tobytes() == h_map.tobytes()
                                               and c["scan_sig"].tobytes() == h_scan.tobytes() and np.array_equal(c["records"][:hq], h_rec)
                                               and np.array_equal(d_rec.cpu().numpy(), c["records"]))}
        if res is not None:
            e = res["poses"] - bag.truth[ids]
            size.update(position_error_max_m=float(np.nanmax(np.hypot(e[:, 0], e[:, 1]))),
                        heading_error_max_deg=float(np.nanmax(np.degrees(np.abs(csm.angle_mod(e[:, 2]))))),
                        queries_without_pose=int((res["rank"] < 0).sum()),
                        winning_ranks=[int(v) for v in np.bincount(np.maximum(res["rank"], 0), minlength=int(spec.top_k))])
        out["sizes"].append(size)
        print(json.dumps(size), flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
