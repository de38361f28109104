"""Times the strip kernel that performs every add (csm_correlate16_kernel, or csm_correlate_kernel with --cell-bits 8) on
the bench workload, with the skip map and dense, for the libraries given -- by default every one under build/variants/
(tools/c16_variants.sh) --, one child process per library and round (NHIP_LIB), interleaved over `rounds`, each under its
own time limit; the first child that fails ends the run.
  python tools/c16_time.py [--cell-bits 16] [--scans 300] [--rounds 3] [LIB.so ...]        -> JSON lines on stdout"""
import argparse
import glob
import json
import os
os.environ.setdefault("NHIP_TUNABLES", "1")  # (the library reads its switches only then)
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(scans, steps, cell_bits):
    sys.path.insert(0, ROOT)
    import ctypes as C
    import torch
    import bench
    from nautilus_amd import _lib, sharding
    lib = _lib.load()
    wl = bench.Workload("weak", 1, scans=scans)
    plan = sharding.ShardPlan(wl.src, wl.tgt, wl.th0, 1)
    dev = torch.device("cuda", 0)
    out = {}
    for dense in ("0", "1"):
        os.environ["NHIP_CSM_DENSE"] = dense
        m = bench.HipMatcher(wl, plan.shard(0), dev, cell_bits, exhaustive=True)
        m.step()
        torch.cuda.synchronize()
        lib.nhip_timing_reset()
        lib.nhip_timing_enable(1)
        for _ in range(steps):
            m.step()
        torch.cuda.synchronize()
        lib.nhip_timing_enable(0)
        ms, n = C.c_double(0), C.c_int32(0)
        lib.nhip_timing_get(0, C.byref(ms), C.byref(n))
        out["dense" if dense == "1" else "skip"] = ms.value / max(n.value, 1)
        out["sum_check"] = int(m.d_sums[:m.n_pairs].sum().item())
        m.free_grids()
    out["pairs"] = wl.n_pairs
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=300)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--cell-bits", type=int, choices=(8, 16), default=16)
    ap.add_argument("--timeout", type=int, default=240, help="seconds a child may take")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("libs", nargs="*", help="libraries to time (default: build/variants/lib_*.so)")
    a = ap.parse_args()
    if a.child:
        child(a.scans, a.steps, a.cell_bits)
        sys.exit(0)
    libs = [os.path.abspath(lp) for lp in a.libs] or sorted(glob.glob(os.path.join(ROOT, "build", "variants", "lib_*.so")))
    for r in range(a.rounds):
        for lp in libs:
            env = dict(os.environ, NHIP_LIB=lp)
            p = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child",
                                "--scans", str(a.scans), "--steps", str(a.steps), "--cell-bits", str(a.cell_bits)],
                               env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            line = p.stdout.decode().strip().splitlines()[-1] if p.stdout.strip() else p.stderr.decode()[-400:]
            print(json.dumps({"lib": lp if a.libs else os.path.basename(lp), "cell_bits": a.cell_bits, "round": r, "exit": p.returncode,
                              "result": line}), flush=True)
            if p.returncode != 0:  # (a fault, an abort or the time limit: nothing more is started on that GPU)
                sys.exit(p.returncode)
