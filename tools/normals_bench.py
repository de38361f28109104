"""What the scan normals cost (nhip_normals_estimate_dev, nhip_normals.hip): the 1000 dense 1081-point scans of BASELINE
configs[1] (bench.Workload("weak", 1)) and 10,000 scans of 1081 points (the same 1000, ten times over: casting 10,000 costs
12 s, and a scan's cost does not depend on its neighbours in the batch), timed with device events, median of --launches after
--warmup, with the spread.  Beside the time: points per second, and the distance tests the launch performs -- every point
against every point of its scan, once more for a point whose radius grew.  Writes profiles/normals_bench.json.

  python tools/normals_bench.py [--launches 10] [--warmup 2] [--out profiles/normals_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Estimate:
    def __init__(self, xy, off):
        import torch
        from nautilus_amd import _lib, normals
        self.torch, self._lib, self.lib = torch, _lib, _lib.load()
        dev = torch.device("cuda", 0)
        self.spec = normals.default_spec()
        self.n, self.n_points = len(off) - 1, len(xy)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.d_xy, self.d_off = t(xy), t(off)
        self.d_nrm = torch.zeros(2 * len(xy), dtype=torch.float32, device=dev)
        self.d_info = torch.zeros(4 * len(xy), dtype=torch.int32, device=dev)
        self.sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def estimate(self, info=False):
        self._lib.check(self.lib.nhip_normals_estimate_dev(self.d_xy.data_ptr(), self.d_off.data_ptr(), self.n, C.byref(self.spec),
                                                           self.d_nrm.data_ptr(), self.d_info.data_ptr() if info else None, self.sp))

    def distance_tests(self, off):
        """Of one launch: n tests per point of a scan of n points, n more for a point whose list was rebuilt at a grown radius."""
        self.estimate(info=True)
        self._lib.check(self.lib.nhip_dev_status(self.sp, None))
        info = self.d_info.cpu().numpy().reshape(-1, 4)
        per_point = np.repeat(np.diff(off).astype(np.int64), np.diff(off))
        rebuilt = (info[:, 1] > 0) & (info[:, 0] >= 2)
        return int(per_point.sum() + per_point[rebuilt].sum()), int(rebuilt.sum()), float((info[:, 3] >> 16).mean())

    def time(self, fn, launches, warmup):
        torch = self.torch
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


def workloads():
    import bench
    wl = bench.Workload("weak", 1)
    xy10 = np.tile(wl.xy, (10, 1))
    off10 = (np.arange(10 * wl.n_scans + 1, dtype=np.int64) * 1081).astype(np.int32)
    assert np.all(np.diff(wl.off) == 1081)
    return {"configs[1]: 1000 scans x 1081": (wl.xy, wl.off), "10,000 scans x 1081": (xy10, off10)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normals_bench.json"))
    a = ap.parse_args()
    res = {"note": "nhip_normals_estimate_dev (default spec, no info), device events around each launch", "sizes": {}}
    for name, (xy, off) in workloads().items():
        es = Estimate(xy, off)
        tests, rebuilt, samples = es.distance_tests(off)
        r = {"n_scans": es.n, "n_points": es.n_points, "distance_tests": tests, "points_rebuilt": rebuilt,
             "samples_per_point": samples, "estimate": es.time(es.estimate, a.launches, a.warmup)}
        r["points_per_s"] = es.n_points / (r["estimate"]["median_ms"] * 1e-3)
        r["distance_tests_per_s"] = tests / (r["estimate"]["median_ms"] * 1e-3)
        res["sizes"][name] = r
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
