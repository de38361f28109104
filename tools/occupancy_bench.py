"""What the occupancy grid (K14, nhip_occupancy_dev) costs: SynthBag at --scans scans (2,000) at its TRUTH poses, the defaults,
the window of every pose +- 30 m.  The scans are uploaded once; each call is timed on the host (enqueue, the status check that
drains the stream, and the downloads of grid, planes and stats are in call_ms) and split into trace (clears included) and
classification by the in-stream timers (NHIP_TIMER_OCC_*: hipEvents on the call's stream).  Median of --calls calls after
--warmup.  There is no earlier device path to compare with: the yardstick is tests/occupancy_reference.py, the numpy statement
of the same spec, in one process on the same machine -- timed on the first --ref-scans scans (120), and its outputs on ALL
scans compared with the device's.  Also reported: ray steps per second, and the flush's atomics per second and added bytes per
second (one int32 add per distinct cell of a scan) over the WHOLE trace interval, which also holds the clears and the ray
steps -- a lower bound of the flush's own rate.  Writes profiles/occupancy_bench.json.

--step-atomics-lib PATH: also time the TIMING-ONLY build of the trace kernel that adds every ray step straight to `misses`
with a global atomic (`make -C nautilus_amd/csrc step-atomics` builds it beside the library; it counts steps, not scans, so
its planes are not the spec's and nothing is compared), in a child process that loads that library, and record the ratio.

  python tools/occupancy_bench.py [--scans 2000] [--calls 20] [--warmup 3] [--ref-scans 120] [--step-atomics-lib PATH]
                                  [--out profiles/occupancy_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=2000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ref-scans", type=int, default=120)
    ap.add_argument("--step-atomics-lib", default=None, help="the library built by `make step-atomics` (timing only)")
    ap.add_argument("--trace-only", action="store_true", help="print the trace timer's JSON and stop (what the child process runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "occupancy_bench.json"))
    a = ap.parse_args()
    import torch
    from nautilus_amd import _lib, csm, occupancy, synth
    from tests import occupancy_reference as R
    lib, dev = _lib.load(), torch.device("cuda:0")
    bag = synth.SynthBag(a.scans)
    xy, off = csm.pack_scans(bag.scans)
    poses = bag.truth
    spec = occupancy.window_spec(poses, 30.0)
    d_xy, d_off = torch.from_numpy(xy).to(dev), torch.from_numpy(off).to(dev)
    ids = (_lib.NHIP_TIMER_OCC_TRACE, _lib.NHIP_TIMER_OCC_CLASSIFY)

    def call():
        lib.nhip_timing_reset()
        t0 = time.perf_counter()
        out = occupancy.occupancy_grid_on_device(d_xy, d_off, len(off) - 1, poses, spec)
        wall = 1e3 * (time.perf_counter() - t0)
        ms = []
        for i in ids:
            v, n = C.c_double(0), C.c_int32(0)
            _lib.check(lib.nhip_timing_get(i, C.byref(v), C.byref(n)))
            ms.append(v.value)
        return wall, ms, out

    for _ in range(a.warmup):
        call()
    _lib.check(lib.nhip_timing_enable(1))
    runs = [call() for _ in range(a.calls)]
    _lib.check(lib.nhip_timing_enable(0))
    lib.nhip_timing_reset()
    wall = np.array([r[0] for r in runs])
    parts = np.array([r[1] for r in runs])
    grid, hits, misses, stats = runs[-1][2]
    med = np.median(parts, axis=0)
    stat = lambda v: {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())}
    if a.trace_only:
        print(json.dumps({"trace_ms": stat(parts[:, 0]), "misses_sum": int(misses.sum())}))
        return
    aff = R.pose_affines(poses)
    steps = 0
    for i in range(len(off) - 1):
        b = R.beams(xy[off[i]:off[i + 1]], aff[i], spec)
        steps += int(np.abs(b[1]).max(axis=1).sum()) if b is not None and len(b[1]) else 0
    k = min(a.ref_scans, a.scans)
    t0 = time.perf_counter()
    R.occupancy(xy[:off[k]], off[:k + 1], poses[:k], spec)
    ref_s = time.perf_counter() - t0
    want = R.occupancy(xy, off, poses, spec)
    atomics = int(hits.sum()) + int(misses.sum())
    out = {
        "note": "nhip_occupancy_dev on scans already on the device (the upload of the affines, the allocation and the downloads of "
                "grid, planes and stats included in call_ms); phases by hipEvents on the call's stream; the reference is "
                "tests/occupancy_reference.py (numpy) in one process on the same machine's CPU",
        "n_scans": a.scans, "n_points": int(len(xy)), "poses": "truth", "window_cells": [spec.width, spec.height],
        "max_ray_cells": spec.max_ray_cells, "stats": [int(v) for v in stats],
        "calls": a.calls, "warmup": a.warmup,
        "call_ms": stat(wall), "trace_ms": stat(parts[:, 0]), "classify_ms": stat(parts[:, 1]),
        "ray_steps": steps, "ray_steps_per_s": float(steps / (1e-3 * med[0])) if med[0] > 0 else None,
        "flush_atomics": atomics,
        "flush_atomics_per_s_lower_bound": float(atomics / (1e-3 * med[0])) if med[0] > 0 else None,
        "flush_added_gb_per_s_lower_bound": float(4 * atomics / (1e6 * med[0])) if med[0] > 0 else None,
        "guide_float_atomics_gb_per_s": 1300.0,
        "atomics_note": "the chip-wide 1.3 TB/s was measured for FLOAT atomic adds of 256 contiguous bytes per wave instruction; a "
                        "rate for int32 adds is unmeasured, and the sweep's adds are as sparse as a scan's free cells in a row",
        "classify_bytes": int(9 * spec.width * spec.height),
        "classify_gb_per_s": float(9 * spec.width * spec.height / (1e6 * med[1])) if med[1] > 0 else None,
        "reference_scans": k, "reference_s": ref_s,
        "outputs_equal_reference": bool(all(np.array_equal(g, w) for g, w in zip((grid, hits, misses, stats), want))),
    }
    if a.step_atomics_lib:
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--trace-only", "--scans", str(a.scans), "--calls", str(a.calls),
                                "--warmup", str(a.warmup)], env=dict(os.environ, NHIP_LIB=os.path.abspath(a.step_atomics_lib)),
                               capture_output=True, text=True, timeout=600)
        if child.returncode != 0:
            raise RuntimeError("the step-atomics child failed:\n" + child.stderr[-2000:])
        other = json.loads(child.stdout.strip().splitlines()[-1])
        out["step_atomics"] = {
            "note": "TIMING ONLY, never shipped: the trace kernel with one global atomicAdd on `misses` per ray step instead of the LDS "
                    "bitmap and its sweep (hits unchanged); it counts steps, not scans, so only its time is reported",
            "trace_ms": other["trace_ms"], "global_atomics_on_misses": other["misses_sum"],
            "ratio_to_bitmap": float(other["trace_ms"]["median"] / med[0]) if med[0] > 0 else None}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
