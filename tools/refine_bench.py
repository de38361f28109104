"""What the match refinement costs (K22, nhip_refine.hip): on configs[1] (bench.Workload("weak", 1): 1,000
targets, 10,000 pairs, 16-bit cells, the headline's settings) the tables are built and the list matched once; the start poses
come from the matcher's own records, the clouds and the bag's normals are on the device.  nhip_refine_icp_dev is timed by a pair
of hipEvents around `--calls` calls, the median of `--samples` samples after a warm-up, beside, from the same session,
  * the matcher's time for the list (nhip_csm_match_dev alone on the same tables);
  * the unfused composition the tree already offers: one correspondence search (nhip_corr_search_dev + compaction) plus one
    normal-equation launch (nhip_resid_lidar_normal_eq_dev) on the same 10,000 blocks at fixed poses (the bag's true ones),
    multiplied by the refinement's median iteration count + 1 -- what a caller pays today for the same evaluations, the host
    round trips between them not counted;
  * hostside.refine_matches on the CPU, on the first `--host-pairs` pairs (the record, not a leg of the comparison), which
    must equal the device's records byte for byte.
Reports the iterations min / median / max, the count per flag, and the refined against the lattice error on the list.  A split of
the kernel's time between staging, search and reduction is not taken.  Writes profiles/refine_bench.json.

  python tools/refine_bench.py [--calls 20] [--samples 10] [--host-pairs 64] [--out profiles/refine_bench.json]
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


def sampled(torch, fn, calls, samples, warmup=2):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(samples):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / calls)
    ms = np.array(ms)
    return {"median_ms_per_call": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()), "calls": calls,
            "samples": samples}


def errors(truth, t):
    dt = np.hypot(t[:, 0] - truth[:, 0], t[:, 1] - truth[:, 1])
    dr = t[:, 2] - truth[:, 2]
    dr = np.abs(dr - 2 * math.pi * np.rint(dr / (2 * math.pi)))
    return {"rms_m": float(np.sqrt(np.mean(dt ** 2))), "max_m": float(dt.max()), "rms_deg": float(np.degrees(np.sqrt(np.mean(dr ** 2)))),
            "max_deg": float(np.degrees(dr.max())), "pairs": int(len(dt))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--host-pairs", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_bench.json"))
    a = ap.parse_args()
    import torch
    import bench
    from nautilus_amd import _lib, csm, hostside, refine
    from nautilus_amd.correspondence import IcpBatch
    from tools.gate_bench import Match
    t0 = time.perf_counter()
    wl = bench.Workload("weak", 1)
    mt = Match(wl, (wl.src, wl.tgt, wl.th0), 16)
    m, lib = mt.m, mt.m.lib
    mt.run(None)
    torch.cuda.synchronize()
    dev = m.d_grids.device
    records = m.d_out.cpu().numpy().copy().view(csm.MATCH_DTYPE).reshape(-1)
    src = np.ascontiguousarray(m.src, dtype=np.int32)
    tgt = np.ascontiguousarray(np.asarray(m.ids)[np.asarray(m.slot)], dtype=np.int32)
    theta0 = np.ascontiguousarray(m.h_th0, dtype=np.float64)
    normals = np.concatenate(wl.bag.normals).astype(np.float32)
    pose0 = refine.start_poses(records, theta0, m.spec, m.search)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    d_nrm, d_src, d_tgt, d_pose0 = t(normals), t(src), t(tgt), t(pose0)
    spec = refine.default_spec()
    n = len(src)
    run = lambda: refine.icp_on_device(m.d_xy, d_nrm, m.d_off, m.n_scans, d_src, d_tgt, d_pose0, n, spec)
    refined = refine.records_from(run())
    _lib.check(lib.nhip_dev_status(m.sp, None))

    res = {"note": "configs[1]: start poses from the matcher's own records (16-bit cells, NHIP_SEARCH_EXACT_SCORE), the bag's normals; "
                   "a pair of hipEvents around `calls` calls, median over `samples` samples after 2 warm-up calls",
           "n_pairs": int(n), "n_targets": int(m.n_targets), "points_per_scan_median": float(np.median(np.diff(wl.off)))}
    res["match"] = sampled(torch, lambda: mt.run(None), a.calls, a.samples)
    res["refine_icp_dev"] = sampled(torch, run, a.calls, a.samples)
    res["match_again"] = sampled(torch, lambda: mt.run(None), a.calls, a.samples)
    res["refine_us_per_pair"] = 1e3 * res["refine_icp_dev"]["median_ms_per_call"] / n

    batch = IcpBatch(wl.xy, normals, wl.off, src, tgt, device=str(dev), outlier_threshold=0.25)
    batch.set_poses(wl.bag.truth)
    batch.search()

    def unfused():
        batch.search(sync=False)
        batch.normal_equations(_lib.NHIP_LIDAR_NORMAL)
    its = refined["iterations"]
    used = hostside.refine_keeps_pose(refined)
    res["unfused_search_plus_normal_eq"] = sampled(torch, unfused, max(a.calls // 4, 1), a.samples)
    res["iterations_min_median_max"] = [int(its.min()), float(np.median(its)), int(its.max())]
    res["unfused_times_evaluations_ms"] = res["unfused_search_plus_normal_eq"]["median_ms_per_call"] * (float(np.median(its)) + 1.0)
    res["flags"] = hostside.refine_flag_counts(refined)
    res["pairs_with_refined_pose"] = int(used.sum())
    truth = np.array([wl.bag.true_relative(s, t_) for s, t_ in zip(src, tgt)])
    ok = records["itheta"] >= 0
    lattice = np.stack([pose0[:, 2], pose0[:, 3], np.arctan2(pose0[:, 1], pose0[:, 0])], axis=1)
    res["error_lattice_all_matched"] = errors(truth[ok], lattice[ok])
    res["error_lattice_on_refined_pairs"] = errors(truth[used], lattice[used])
    res["error_refined_on_refined_pairs"] = errors(truth[used], refine.to_transform(refined[used]))
    near = used & (np.hypot(lattice[:, 0] - truth[:, 0], lattice[:, 1] - truth[:, 1]) < 0.2)
    res["error_lattice_where_lattice_within_0.2m"] = errors(truth[near], lattice[near])
    res["error_refined_where_lattice_within_0.2m"] = errors(truth[near], refine.to_transform(refined[near]))

    k = min(int(a.host_pairs), n)
    t1 = time.perf_counter()
    host = hostside.refine_matches(wl.xy, normals, wl.off, src[:k], tgt[:k], theta0[:k], records[:k], m.spec, m.search)
    res["hostside_refine_matches"] = {"pairs": k, "seconds": time.perf_counter() - t1,
                                      "equals_device_bytes": bool(host.tobytes() == refined[:k].tobytes())}
    res["phase_split"] = "not measured"
    res["seconds"] = time.perf_counter() - t0
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
