"""What the scan-feature extraction costs (nhip_features_extract_dev + nhip_features_pack_dev, nhip_feat.hip): the 1000 dense
1081-point scans of BASELINE configs[1] (bench.Workload("weak", 1)) and 10,000 scans of 1081 points (the same 1000, ten
times over: the kernel's time does not depend on which scans they are, and casting 10,000 costs 12 s), timed with device
events, median of --launches after --warmup, with the spread; the extraction also with both caps at 1 (scores + two rounds of
selection instead of 21: the rounds' share by difference).  Then one child process under
`rocprofv3 --kernel-trace --stats` (a run of its own) gives the kernels' own times.  Writes profiles/features_bench.json.

  python tools/features_bench.py [--launches 20] [--warmup 3] [--out profiles/features_bench.json] [--no-trace]
  python tools/features_bench.py --child        (what runs under rocprofv3: 5 launches per size, no timing)
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Extract:
    def __init__(self, xy, off, normals):
        import torch
        from nautilus_amd import _lib, features
        self.torch, self._lib, self.lib = torch, _lib, _lib.load()
        dev = torch.device("cuda", 0)
        self.spec = features.default_spec()
        self.n = len(off) - 1
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.d_xy, self.d_off, self.d_nrm = t(xy), t(off), t(normals)
        e = lambda k, dt: torch.empty(k, dtype=dt, device=dev)
        self.d_pi, self.d_pc = e(self.n * self.spec.max_planar, torch.int32), e(self.n, torch.int32)
        self.d_ei, self.d_ec = e(self.n * self.spec.max_edge, torch.int32), e(self.n, torch.int32)
        self.out = [(e(2 * self.n * c, torch.float32), e(2 * self.n * c, torch.float32), e(self.n + 1, torch.int32))
                    for c in (self.spec.max_planar, self.spec.max_edge)]
        self.sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def extract(self, spec=None):
        self._lib.check(self.lib.nhip_features_extract_dev(self.d_xy.data_ptr(), self.d_off.data_ptr(), self.n,
                                                           C.byref(self.spec if spec is None else spec),
                                                           self.d_pi.data_ptr(), self.d_pc.data_ptr(), self.d_ei.data_ptr(),
                                                           self.d_ec.data_ptr(), None, self.sp))

    def extract_caps_1(self):
        """Both caps 1: the scores and two rounds of selection instead of 21 -- what the rounds of phase 2 cost, by difference."""
        from nautilus_amd import features
        self.extract(features.feature_spec(max_planar=1, max_edge=1))

    def pack(self):
        for (d_idx, d_cnt, cap), (xo, no, oo) in zip(((self.d_pi, self.d_pc, self.spec.max_planar), (self.d_ei, self.d_ec, self.spec.max_edge)),
                                                     self.out):
            self._lib.check(self.lib.nhip_features_pack_dev(self.d_xy.data_ptr(), self.d_nrm.data_ptr(), self.d_off.data_ptr(), self.n,
                                                            d_idx.data_ptr(), d_cnt.data_ptr(), cap, xo.data_ptr(), no.data_ptr(),
                                                            oo.data_ptr(), self.sp))

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
    nrm = np.concatenate(wl.bag.normals).astype(np.float32)
    xy10 = np.tile(wl.xy, (10, 1))
    off10 = (np.arange(10 * wl.n_scans + 1, dtype=np.int64) * 1081).astype(np.int32)
    return {"configs[1]: 1000 scans x 1081": (wl.xy, wl.off, nrm), "10,000 scans x 1081": (xy10, off10, np.tile(nrm, (10, 1)))}


def kernel_stats():
    """The child under rocprofv3 --kernel-trace --stats: {kernel and grid size: calls, median / min / max us} of the feat_* kernels."""
    tmp = tempfile.mkdtemp(prefix="features_bench_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable,
               os.path.abspath(__file__), "--child"]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        if p.returncode != 0:
            return {"error": "rocprofv3 exited %d: %s" % (p.returncode, p.stderr.decode("utf-8", "replace")[-400:])}
        rows = []
        for f in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            rows += [r for r in csv.DictReader(open(f)) if "feat_" in r["Kernel_Name"]]
        out = {}
        for r in rows:  # per dispatch: the two sizes apart, by grid size
            name = [k for k in ("feat_extract_kernel", "feat_offsets_kernel", "feat_pack_kernel") if k in r["Kernel_Name"]][0]
            key = "%s grid %s" % (name, r.get("Grid_Size_X", r.get("Grid_Size", "?")))
            out.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        return {k: {"calls": len(v), "median_us": float(np.median(v)), "min_us": float(min(v)), "max_us": float(max(v))}
                for k, v in sorted(out.items())}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "features_bench.json"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    import torch
    res = {"note": "nhip_features_extract_dev (default spec, no scores) and the two nhip_features_pack_dev calls (planar, edge; with "
                   "normals), device events around each launch; kernel times from a separate run under rocprofv3 --kernel-trace --stats",
           "table_build_of_the_same_1000_scans_ms": 0.55, "sizes": {}}
    for name, (xy, off, nrm) in workloads().items():
        ex = Extract(xy, off, nrm)
        if a.child:
            for _ in range(5):
                ex.extract()
                ex.pack()
            torch.cuda.synchronize()
            continue
        r = {"n_scans": ex.n, "extract_caps_1": ex.time(ex.extract_caps_1, a.launches, a.warmup),
             "extract": ex.time(ex.extract, a.launches, a.warmup), "pack": ex.time(ex.pack, a.launches, a.warmup)}
        r["planar_per_scan"] = float(ex.d_pc.float().mean().item())
        r["edge_per_scan"] = float(ex.d_ec.float().mean().item())
        res["sizes"][name] = r
    if a.child:
        return
    if not a.no_trace:
        res["kernels"] = kernel_stats()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
