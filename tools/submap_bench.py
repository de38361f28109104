"""What submap tables cost (nhip_submaps_gather_dev, nhip_submap.hip, in front of the table build): the 1000 dense 1081-point
scans and 10,000 pairs of BASELINE configs[1] (bench.Workload("weak", 1)), every scan a target, its submap the scans
t - k .. t + k under the odometry, k in {0, 3, 5}.  Device events around runs of launches, median of --samples after --warmup,
with min - max.  Per k: the gather, the table rebuild over the gathered cloud, the matcher on those tables; beside them the
plain rebuild of the same targets and the matcher on the plain tables, measured in the same run.  The gather's bytes (points
read + points written, 8 bytes each) against the 8 TB/s of HBM.  Writes profiles/submap_bench.json.

  python tools/submap_bench.py [--samples 10] [--warmup 2] [--out profiles/submap_bench.json]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12


class Bench:
    def __init__(self, wl, cell_bits=16):
        import torch
        from nautilus_amd import _lib, csm
        self.torch, self._lib, self.lib, self.wl = torch, _lib, _lib.load(), wl
        self.dev = torch.device("cuda", 0)
        self.t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self.spec = csm.grid_spec(30.0, 0.05, 2.0, 1e-10, 40, cell_bits=cell_bits, no_image=True)  # the benchmark's slots
        self.n = wl.n_scans
        self.d_xy, self.d_off = self.t(wl.xy), self.t(wl.off)
        self.d_ids = torch.arange(self.n, dtype=torch.int32, device=self.dev)
        self.ws_bytes = self.lib.nhip_grid_workspace_bytes(C.byref(self.spec), self.n)
        self.sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        # the matcher's side: the benchmark's 10,000 pairs, slot = target
        self.search = csm.search_spec(61, 81, 81, math.radians(1.0), short_scans=True)
        self.n_pairs = wl.n_pairs
        rot0 = np.empty((self.n_pairs, 2))
        _lib.check(self.lib.nhip_csm_rot0(_lib.ptr(np.ascontiguousarray(wl.th0, dtype=np.float64)), None, self.n_pairs, _lib.ptr(rot0)))
        self.d_src, self.d_slot, self.d_rot0 = self.t(wl.src.astype(np.int32)), self.t(wl.tgt.astype(np.int32)), self.t(rot0)
        self.d_delta = self.t(csm.delta_table(self.search))
        self.d_keys = torch.empty(self.n_pairs, dtype=torch.int64, device=self.dev)
        self.d_out = torch.empty((self.n_pairs, 4), dtype=torch.int32, device=self.dev)
        self.ws_csm = self.lib.nhip_csm_workspace_bytes(self.n_pairs)
        self.d_ws_csm = torch.empty(self.ws_csm, dtype=torch.uint8, device=self.dev)

    def tables(self):
        torch = self.torch
        g = torch.empty(self.lib.nhip_grids_bytes(C.byref(self.spec), self.n), dtype=torch.uint8, device=self.dev)
        g[-256:].zero_()
        return g, torch.empty(self.ws_bytes, dtype=torch.uint8, device=self.dev)

    def build(self, d_xy, d_off, tables, rebuild):
        fn = self.lib.nhip_grid_rebuild_dev if rebuild else self.lib.nhip_grid_build_dev
        self._lib.check(fn(d_xy.data_ptr(), d_off.data_ptr(), self.n, self.d_ids.data_ptr(), self.n, C.byref(self.spec),
                           tables[0].data_ptr(), tables[1].data_ptr(), self.ws_bytes, self.sp))

    def match(self, tables):
        self._lib.check(self.lib.nhip_csm_match_dev(self.d_xy.data_ptr(), self.d_off.data_ptr(), self.n, tables[0].data_ptr(), self.n,
                                                    C.byref(self.spec), self.d_src.data_ptr(), self.d_slot.data_ptr(),
                                                    self.d_rot0.data_ptr(), self.d_delta.data_ptr(), None, self.n_pairs,
                                                    C.byref(self.search), self.d_keys.data_ptr(), self.d_out.data_ptr(), None,
                                                    self.d_ws_csm.data_ptr(), self.ws_csm, self.sp))

    def submaps(self, k):
        """The member arrays of radius k on the device, and buffers for the merged cloud."""
        from nautilus_amd import csm, hostside
        torch = self.torch
        targets = np.arange(self.n)
        scan, moff = hostside.submap_members(self.n, targets, k)
        aff = csm.submap_member_affines(self.wl.bag.odom, np.repeat(targets, np.diff(moff)), scan)
        total = int(np.diff(self.wl.off)[scan].sum())
        return {"scan": self.t(scan), "aff": self.t(aff), "moff": self.t(moff), "total": total, "members": len(scan),
                "xy": torch.empty((total, 2), dtype=torch.float32, device=self.dev),
                "off": torch.empty(self.n + 1, dtype=torch.int32, device=self.dev)}

    def gather(self, s):
        self._lib.check(self.lib.nhip_submaps_gather_dev(self.d_xy.data_ptr(), self.d_off.data_ptr(), self.n, s["scan"].data_ptr(),
                                                         s["aff"].data_ptr(), s["moff"].data_ptr(), self.n, s["xy"].data_ptr(),
                                                         s["total"], s["off"].data_ptr(), self.sp))

    def time(self, fn, samples, warmup, reps):
        """ms per call: `reps` calls between two events (a gather is tens of microseconds), median over the samples."""
        torch = self.torch
        for _ in range(warmup):
            fn()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(samples)]
        for a, b in ev:
            a.record()
            for _ in range(reps):
                fn()
            b.record()
        torch.cuda.synchronize()
        self._lib.check(self.lib.nhip_dev_status(self.sp, None))
        ms = np.array([a.elapsed_time(b) for a, b in ev]) / reps
        return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()), "samples": samples,
                "calls_per_sample": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "submap_bench.json"))
    a = ap.parse_args()
    import bench
    wl = bench.Workload("weak", 1)
    b = Bench(wl)
    res = {"note": "1000 dense 1081-point scans, every scan a target, 10,000 pairs (bench.Workload('weak', 1)); 16-bit cells, "
                   "slots without the image; device events, ms per call",
           "n_targets": b.n, "n_pairs": b.n_pairs}
    plain = b.tables()
    b.build(b.d_xy, b.d_off, plain, False)
    res["plain"] = {"points": int(wl.off[-1]),
                    "table_rebuild": b.time(lambda: b.build(b.d_xy, b.d_off, plain, True), a.samples, a.warmup, 4),
                    "match": b.time(lambda: b.match(plain), a.samples, a.warmup, 1)}
    res["submaps"] = {}
    for k in (0, 3, 5):
        s = b.submaps(k)
        b.gather(s)
        tables = b.tables()
        b.build(s["xy"], s["off"], tables, False)
        r = {"members": s["members"], "points": s["total"], "points_per_target": s["total"] / b.n,
             "gather": b.time(lambda: b.gather(s), a.samples, a.warmup, 20),
             "table_rebuild": b.time(lambda: b.build(s["xy"], s["off"], tables, True), a.samples, a.warmup, 4),
             "match": b.time(lambda: b.match(tables), a.samples, a.warmup, 1)}
        r["gather_bytes"] = 16 * s["total"]  # a float2 read and a float2 written per point (the member tables are noise)
        r["gather_bytes_per_s"] = r["gather_bytes"] / (r["gather"]["median_ms"] * 1e-3)
        r["gather_share_of_8_TB_per_s"] = r["gather_bytes_per_s"] / HBM_BYTES_PER_S
        r["table_rebuild_over_plain"] = r["table_rebuild"]["median_ms"] / res["plain"]["table_rebuild"]["median_ms"]
        r["points_over_plain"] = s["total"] / res["plain"]["points"]
        r["match_over_plain"] = r["match"]["median_ms"] / res["plain"]["match"]["median_ms"]
        res["submaps"]["k=%d" % k] = r
        del tables, s
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
