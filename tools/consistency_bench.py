"""What the loop-closure consistency costs (K17, nhip_consistency.hip): M = 1,000, 10,000 and 50,000
records of a drifted SynthBag(poses_only=True) loop with injected outliers, the matrix (nhip_consistency_adjacency_dev) and the set
(nhip_consistency_set_dev, steps in batches of 8) each timed alone with hipEvents -- warm-up, then medians with min and max of the
launches.  The 1,000-record result is compared with the numpy host path (hostside.consistent_set) for byte equality, and the host
path's seconds are recorded beside the device's.  Writes profiles/consistency_bench.json.

  python tools/consistency_bench.py [--launches 10] [--warmup 2] [--sizes 1000,10000,50000] [--out profiles/consistency_bench.json]
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


def loop_records(M, n_scans=4000, outliers=0.25, seed=3):
    """M prepared records: revisits (more than 20 scans apart, closer than 2 m) of a drifted loop with lattice noise, a share of
    them displaced by 1.5 .. 3 m."""
    from nautilus_amd import consistency, synth
    bag = synth.SynthBag(n_scans, poses_only=True)
    est = synth.odometry_from_truth(bag.truth, sigma_t=0.02, sigma_th_deg=0.3)
    est = est - est[0] + bag.truth[0]
    rng = np.random.default_rng(seed)
    idx = np.arange(n_scans)
    s, t = [], []
    for a in range(0, n_scans, 500):  # (rows in chunks: the distance matrix of 4,000 scans is 128 MB)
        d = np.linalg.norm(bag.truth[a:a + 500, None, :2] - bag.truth[None, :, :2], axis=2)
        sa, ta = np.nonzero((d < 2.0) & (idx[a:a + 500, None] - idx[None, :] > 20))
        s.append(sa + a), t.append(ta)
    s, t = np.concatenate(s), np.concatenate(t)
    pick = np.sort(rng.choice(len(s), M, replace=M > len(s)))
    src, tgt = s[pick], t[pick]
    c, sn = np.cos(bag.truth[tgt, 2]), np.sin(bag.truth[tgt, 2])
    dx, dy = bag.truth[src, 0] - bag.truth[tgt, 0], bag.truth[src, 1] - bag.truth[tgt, 1]
    rel = np.stack([c * dx + sn * dy, -sn * dx + c * dy, bag.truth[src, 2] - bag.truth[tgt, 2]], axis=1)
    rel[:, :2] += rng.uniform(-0.025, 0.025, (M, 2))
    rel[:, 2] += rng.uniform(-0.01, 0.01, M)
    bad = rng.random(M) < outliers
    r, a = rng.uniform(1.5, 3.0, M), rng.uniform(0, 2 * math.pi, M)
    rel[bad, 0] += (r * np.cos(a))[bad]
    rel[bad, 1] += (r * np.sin(a))[bad]
    return consistency.prepare(est, src, tgt, rel.astype(np.float32).astype(np.float64)), int(bad.sum())


def measure(torch, rec, launches, warmup):
    from nautilus_amd import _lib, consistency
    dev, M = torch.device("cuda:0"), len(rec)
    spec = consistency.default_spec()
    d_rec = torch.from_numpy(rec).to(dev)
    ws = torch.empty(consistency.workspace_bytes(M) // 8, dtype=torch.int64, device=dev)
    got = {}

    def adjacency():
        got["adj"] = consistency.adjacency_on_device(d_rec, M, spec, workspace=ws)

    def the_set():
        got["set"] = consistency.set_on_device(got["adj"][0], got["adj"][1], M, ws, spec)

    res = {"M": M, "words_per_row": consistency.words(M), "workspace_bytes": int(ws.numel() * 8), "pairs": M * (M - 1) // 2}
    res["adjacency"] = timed(torch, adjacency, launches, warmup)
    res["set"] = timed(torch, the_set, max(launches // 3, 2), 1)
    _lib.check(_lib.load().nhip_dev_status(None, None))
    stats = got["set"][2].cpu().numpy()
    res["stats"] = dict(zip(consistency.STATS_FIELDS, (int(v) for v in stats)))
    res["pair_tests_per_s"] = float(M) * M / (res["adjacency"]["median_ms"] * 1e-3)  # (both triangles are computed)
    res["set_us_per_step"] = 1e3 * res["set"]["median_ms"] / max(int(stats[3]), 1)
    res["set_over_adjacency"] = res["set"]["median_ms"] / res["adjacency"]["median_ms"]
    return res, got["adj"][0].cpu().numpy().view(np.uint64), got["adj"][1].cpu().numpy(), got["set"][0].cpu().numpy(), int(got["set"][1].cpu()[0]), stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="1000,10000,50000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consistency_bench.json"))
    a = ap.parse_args()
    import torch
    from nautilus_amd import hostside
    t0 = time.perf_counter()
    out = {"note": "hipEvents around each call; adjacency = nhip_consistency_adjacency_dev (memset, matrix and degree kernels), set = "
                   "nhip_consistency_set_dev (begin, then score + commit per step, batches of 8 with one read of the done word "
                   "between them; the call waits); median with min and max of the launches; the default spec"}
    for M in (int(v) for v in a.sizes.split(",")):
        rec, n_bad = loop_records(M)
        res, adj, deg, members, n, stats = measure(torch, rec, a.launches if M <= 10000 else max(a.launches // 3, 2), a.warmup)
        res["injected_outliers"] = n_bad
        if M <= 1000:
            t1 = time.perf_counter()
            h_members, h_n, h_stats, h_adj, h_deg = hostside.consistent_set(rec, adjacency=True)
            res["host_path_s"] = time.perf_counter() - t1
            res["equal_host_path"] = bool(adj.tobytes() == h_adj.tobytes() and deg.tobytes() == h_deg.tobytes() and n == h_n and
                                          members.tobytes() == h_members.tobytes() and stats.tobytes() == h_stats.tobytes())
            res["device_s"] = 1e-3 * (res["adjacency"]["median_ms"] + res["set"]["median_ms"])
        out["%d_records" % M] = res
    out["seconds"] = time.perf_counter() - t0
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    return 0 if out.get("1000_records", {}).get("equal_host_path", True) else 1


if __name__ == "__main__":
    sys.exit(main())
