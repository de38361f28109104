"""What the matcher's score gate (nhip_csm_match_gated_dev) saves: the matcher alone, ungated and gated at -5, timed with
hipEvents on configs[1] (bench.Workload("weak", 1), 10,000 pairs) and on a configs[3]-style list (sources up to 3.5 m from
their target, 100 per target), at the headline's settings (16-bit cells, NHIP_SEARCH_EXACT_SCORE) and with 8-bit cells.
The tables are built once per list and cell width; only the match is timed.  Then per list an instrumented run
(NHIP_BNB_INSTRUMENT=1 NHIP_BNB_STATS=1, a child process: the library reads the switches at its first call) counts the
pairs settled right after their bounds, the pairs rejected and the blocks refined, and the in-stream timers give the
matcher's kernels (bounds + seeds, candidates, exact score).  Writes profiles/gate_bench.json.

  python tools/gate_bench.py [--launches 20] [--warmup 3] [--c3-targets 30] [--out profiles/gate_bench.json]
  python tools/gate_bench.py --counts LIST CELL_BITS   (the instrumented child: prints one JSON line)
"""
import argparse
import ctypes as C
import json
import math
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
THRESHOLD = -5.0


def make_list(wl, name, c3_targets):
    if name == "configs[1]":
        return wl.src, wl.tgt, wl.th0
    t = np.linspace(0, wl.n_scans - 1, c3_targets + 2).astype(np.int32)[1:-1]
    return wl.bag.sample_pairs(per_target=100, targets=t, max_dist=3.5, min_sep=20, seed=4242)


class Match:
    """One list's tables built once (HipMatcher's buffers, pairs in the bench's launch order); run() launches the match."""

    def __init__(self, wl, lst, cell_bits):
        import torch
        import bench
        from nautilus_amd import sharding
        src, tgt, th0 = lst
        w = sharding.predicted_pair_cost(wl.bag.odom, src, tgt)
        plan = sharding.ShardPlan(src, tgt, th0, 1, w)
        self.torch = torch
        self.m = bench.HipMatcher(wl, plan.shard(0), torch.device("cuda", 0), cell_bits, weights=plan.shard_weights(0),
                                  exact_score=cell_bits == 16)
        self.m.step()  # tables, rotations
        torch.cuda.synchronize()

    def run(self, min_score):
        from nautilus_amd import _lib
        m = self.m
        args = (m.d_xy.data_ptr(), m.d_off.data_ptr(), m.n_scans, m.d_grids.data_ptr(), m.n_targets, C.byref(m.spec),
                m.d_src.data_ptr(), m.d_slot.data_ptr(), m.d_rot0.data_ptr(), m.d_delta.data_ptr(), None, m.n_pairs,
                C.byref(m.search), m.d_keys.data_ptr(), m.d_out.data_ptr(), m.d_sums.data_ptr(), m.d_ws_csm.data_ptr(),
                m.ws_csm, m.sp)
        if min_score is None:
            _lib.check(m.lib.nhip_csm_match_dev(*args))
        else:
            _lib.check(m.lib.nhip_csm_match_gated_dev(*args, float(min_score)))

    def time(self, min_score, launches, warmup):
        torch = self.torch
        for _ in range(warmup):
            self.run(min_score)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
        for a, b in ev:
            a.record()
            self.run(min_score)
            b.record()
        torch.cuda.synchronize()
        ms = np.array([a.elapsed_time(b) for a, b in ev])
        return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()),
                "spread_ms": float(ms.max() - ms.min()), "launches": launches}

    def records(self):
        rec, sums = self.m.records()
        return rec.cpu().numpy().copy(), sums.cpu().numpy().copy()

    def kernel_ms(self, min_score, launches):
        """per launch: the matcher's kernels by the library's in-stream timers"""
        from nautilus_amd import _lib
        lib = self.m.lib
        lib.nhip_timing_enable(1)
        lib.nhip_timing_reset()
        for _ in range(launches):
            self.run(min_score)
        self.torch.cuda.synchronize()
        out = {}
        for name, tid in (("whole_matcher", _lib.NHIP_TIMER_CSM), ("bounds_seeds", _lib.NHIP_TIMER_CSM_BOUNDS),
                          ("candidates", _lib.NHIP_TIMER_CSM_CAND), ("exact_score", _lib.NHIP_TIMER_EXACT_SCORE)):
            tot, n = C.c_double(0), C.c_int32(0)
            _lib.check(lib.nhip_timing_get(tid, C.byref(tot), C.byref(n)))
            out[name] = tot.value / max(n.value, 1) if n.value else None
        lib.nhip_timing_enable(0)
        return out


def counts(list_name, cell_bits, c3_targets):
    """(child process, NHIP_BNB_INSTRUMENT=1 NHIP_BNB_STATS=1) work counters of one ungated and one gated launch"""
    import bench
    from nautilus_amd import csm, _lib
    wl = bench.Workload("weak", 1)
    mt = Match(wl, make_list(wl, list_name, c3_targets), cell_bits)
    n = mt.m.n_pairs
    out = {"n_pairs": n}
    for key, ms in (("ungated", None), ("gated", THRESHOLD)):
        # (the per-pair counters accumulate over launches: this launch's are the difference)
        before = np.zeros(n, np.uint64)
        _lib.check(mt.m.lib.nhip_bnb_stats_per_pair(_lib.ptr(before), n))
        csm.bnb_stats_levels()  # (reset)
        mt.run(ms)
        mt.torch.cuda.synchronize()
        per = np.zeros(n, np.uint64)
        _lib.check(mt.m.lib.nhip_bnb_stats_per_pair(_lib.ptr(per), n))
        per = (per - before).astype(np.float64)
        lv = csm.bnb_stats_levels()
        rec, _ = mt.records()
        out[key] = {"pairs_settled_after_bounds": int(lv["pairs_settled_by_gate"]),
                    "pairs_rejected": int(np.count_nonzero(rec[:, 0] < 0)),
                    "candidate_blocks_refined_per_pair": lv["candidates_refined"] / n,
                    "blocks_evaluated_per_pair": (lv["blocks_whole"] + lv["sub_blocks"] / 4.0) / n,
                    "sub_blocks_evaluated_per_pair_mean": float(per.mean()),
                    "sub_blocks_evaluated_per_pair_p99": float(np.percentile(per, 99)),
                    "kernel_ms_instrumented_build": mt.kernel_ms(ms, 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--c3-targets", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gate_bench.json"))
    ap.add_argument("--counts", nargs=2, metavar=("LIST", "CELL_BITS"))
    a = ap.parse_args()
    if a.counts:
        print(json.dumps(counts(a.counts[0], int(a.counts[1]), a.c3_targets)))
        return 0
    import bench
    t0 = time.perf_counter()
    wl = bench.Workload("weak", 1)
    res = {"threshold": THRESHOLD, "note": "the matcher alone (nhip_csm_match_dev / nhip_csm_match_gated_dev on tables built "
           "once), hipEvents around each launch; 16-bit cells with NHIP_SEARCH_EXACT_SCORE (the headline's settings), 8-bit "
           "cells without; counts and kernel times from an instrumented build (NHIP_BNB_INSTRUMENT=1 NHIP_BNB_STATS=1)",
           "lists": {}}
    for name in ("configs[1]", "configs[3]-style"):
        lst = make_list(wl, name, a.c3_targets)
        entry = {"n_pairs": int(len(lst[0]))}
        for cb in (16, 8):
            mt = Match(wl, lst, cb)
            mt.run(None)
            rec, _ = mt.records()
            ung = mt.time(None, a.launches, a.warmup)
            gat = mt.time(THRESHOLD, a.launches, a.warmup)
            ung2 = mt.time(None, a.launches, a.warmup)  # (again: run-to-run spread of the same launch)
            below = int(np.count_nonzero(rec.view(np.float32)[:, 3] < THRESHOLD))
            entry["u%d" % cb] = {"ungated": ung, "gated": gat, "ungated_again": ung2, "pairs_below_threshold": below,
                                 "kernel_ms_ungated": mt.kernel_ms(None, 5), "kernel_ms_gated": mt.kernel_ms(THRESHOLD, 5)}
            mt.m.free_grids()
            del mt
            # the instrumented counts, in a child process (the library reads the switches at its first call)
            env = dict(os.environ, NHIP_TUNABLES="1", NHIP_BNB_INSTRUMENT="1", NHIP_BNB_STATS="1")
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--counts", name, str(cb), "--c3-targets",
                                str(a.c3_targets)], env=env, capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                entry["u%d" % cb]["counts_error"] = (p.stderr or "")[-2000:]
                print(json.dumps(res), file=sys.stderr)
                raise SystemExit("instrumented child failed (%d): %s" % (p.returncode, p.stderr[-2000:]))
            entry["u%d" % cb]["counts"] = json.loads(p.stdout.strip().splitlines()[-1])
            print(name, cb, json.dumps(entry["u%d" % cb]), flush=True)
        res["lists"][name] = entry
    res["seconds"] = time.perf_counter() - t0
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
