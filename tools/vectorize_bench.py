"""What the map vectorisation (K13, nhip_vectorize_dev) costs: SynthBag at --scans scans (2,000) at its TRUTH poses (the
loop's solve of 2,000 scans takes minutes; the step's cost depends on the cloud, not on where the poses came from), the
defaults, the window of every pose +- 30 m.  The scans are uploaded once; each call is timed on the host (it ends with the
stream drained) and split into raster + cell list, votes and rounds by the in-stream timers (NHIP_TIMER_VEC_*: hipEvents on
the call's stream).  Median of --calls calls after --warmup.  There is no earlier device path to compare with: the yardstick
is tests/vectorize_reference.py, the numpy statement of the same spec, on the same input in one process on the same machine; its records
are compared with the device's.  Also reported: the bytes the votes kernel must read (cells x rows x 8 B) over its time.
Writes profiles/vectorize_bench.json.

  python tools/vectorize_bench.py [--scans 2000] [--calls 20] [--warmup 3] [--check-every 8] [--out profiles/vectorize_bench.json]
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
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--check-every", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vectorize_bench.json"))
    a = ap.parse_args()
    import torch
    from nautilus_amd import _lib, csm, synth, vectorize
    from tests import vectorize_reference as R
    lib, dev = _lib.load(), torch.device("cuda:0")
    bag = synth.SynthBag(a.scans)
    xy, off = csm.pack_scans(bag.scans)
    poses = bag.truth
    spec = vectorize.window_spec(poses, 30.0)
    d_xy, d_off = torch.from_numpy(xy).to(dev), torch.from_numpy(off).to(dev)
    ids = (_lib.NHIP_TIMER_VEC_RASTER, _lib.NHIP_TIMER_VEC_VOTES, _lib.NHIP_TIMER_VEC_ROUNDS)

    def call():
        lib.nhip_timing_reset()
        t0 = time.perf_counter()
        lines, rec, stats = vectorize.vectorize_on_device(d_xy, d_off, len(off) - 1, poses, spec, check_every=a.check_every)
        wall = 1e3 * (time.perf_counter() - t0)
        ms = []
        for i in ids:
            v, n = C.c_double(0), C.c_int32(0)
            _lib.check(lib.nhip_timing_get(i, C.byref(v), C.byref(n)))
            ms.append(v.value)
        return wall, ms, lines, rec, stats

    for _ in range(a.warmup):
        call()
    _lib.check(lib.nhip_timing_enable(1))
    runs = [call() for _ in range(a.calls)]
    _lib.check(lib.nhip_timing_enable(0))
    lib.nhip_timing_reset()
    wall = np.array([r[0] for r in runs])
    parts = np.array([r[1] for r in runs])
    _, _, lines, rec, stats = runs[-1]
    t0 = time.perf_counter()
    want = R.vectorize(xy, off, poses, spec)
    ref_s = time.perf_counter() - t0
    med = np.median(parts, axis=0)
    vote_bytes = int(stats[0]) * spec.n_theta * 8
    out = {
        "note": "nhip_vectorize_dev on scans already on the device (workspace allocation, the upload of the affines and the "
                "downloads of records and stats included in call_ms); phases by hipEvents on the call's stream; the reference is "
                "tests/vectorize_reference.py (numpy) on the same input in one process on the same machine's CPU",
        "n_scans": a.scans, "n_points": int(len(xy)), "poses": "truth",
        "window_cells": [spec.width, spec.height], "n_theta": spec.n_theta, "n_rho": int(stats[6]), "check_every": a.check_every,
        "cells": int(stats[0]), "segments": int(stats[1]), "rounds": int(stats[2]), "flag": int(stats[3]),
        "cells_emitted": int(stats[4]), "cells_retired": int(stats[5]),
        "calls": a.calls, "warmup": a.warmup,
        "call_ms": {"median": float(np.median(wall)), "min": float(wall.min()), "max": float(wall.max())},
        "raster_and_cells_ms": {"median": float(med[0]), "min": float(parts[:, 0].min()), "max": float(parts[:, 0].max())},
        "votes_ms": {"median": float(med[1]), "min": float(parts[:, 1].min()), "max": float(parts[:, 1].max())},
        "rounds_ms": {"median": float(med[2]), "min": float(parts[:, 2].min()), "max": float(parts[:, 2].max())},
        "rounds_us_per_round": float(1e3 * med[2] / max(int(stats[2]) + 1, 1)),
        "votes_bytes_read": vote_bytes,
        "votes_gb_per_s": float(vote_bytes / (1e6 * med[1])) if med[1] > 0 else None,
        "reference_s": ref_s,
        "records_equal_reference": bool(rec.tolist() == want["records"].tolist() and stats.tolist() == want["stats"].tolist()),
        "lines_equal_reference": bool(np.array_equal(lines.view(np.uint32), want["lines"].view(np.uint32))),
    }
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
