"""What the robust-loss rows cost (K18, nhip_loss.hip): nhip_resid_odometry_robust_normal_eq_dev at
1,000 and 100,000 factors, every loss kind, with and without the weights output, in both forms of its row store (every lane its
own 224-byte row, or the workgroup's span staged in LDS and stored as whole lines: NHIP_LOSS_STORE, read per launch in a process
with NHIP_TUNABLES=1), beside nhip_resid_odometry_normal_eq_dev on the same factors in the same process.  hipEvents around
windows of --reps back-to-back launches, the variants alternating window by window after a warm-up of each; per-launch medians
with min and max over the windows.  The two forms' outputs are compared for byte equality at every size and kind, and NONE's
with the plain kernel's.  Writes profiles/loss_bench.json.

  python tools/loss_bench.py [--windows 15] [--reps 200] [--warmup 3] [--sizes 1000,100000] [--out profiles/loss_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

os.environ.setdefault("NHIP_TUNABLES", "1")  # (the library reads its switches only then)

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TW, RW, SCALE = 10.0, 10.0, 1.0  # the loop closures' weights, --lc-loss-scale's default
SHIPPED = "staged"                # nhip_loss.hip's STAGED_BY_DEFAULT, restated: the form a process without the switch runs


def factors(n, seed=5):
    """n closure-like factors over a 4,000-pose track: most close to a few centimetres, one in five is displaced by metres."""
    rng = np.random.default_rng(seed)
    n_poses = 4000
    poses = np.concatenate([np.cumsum(rng.normal(0, 0.3, (n_poses, 2)), axis=0), rng.uniform(-np.pi, np.pi, (n_poses, 1))], axis=1)
    pi, pj = rng.integers(0, n_poses, n).astype(np.int32), rng.integers(0, n_poses, n).astype(np.int32)
    t = poses[pj, :2] - poses[pi, :2] + rng.normal(0, 0.03, (n, 2))
    r = poses[pj, 2] - poses[pi, 2] + rng.normal(0, 0.01, n)
    bad = rng.random(n) < 0.2
    t[bad] += rng.uniform(-3, 3, (int(bad.sum()), 2))
    return poses, pi, pj, t.astype(np.float32), r.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="1000,100000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_bench.json"))
    a = ap.parse_args()
    import torch
    from nautilus_amd import _lib
    from nautilus_amd.loss import KINDS, Loss
    lib = _lib.load()
    if _lib.device_count() == 0:
        raise SystemExit("loss_bench: no HIP device")
    dev = torch.device("cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    t0 = time.perf_counter()
    out = {"note": "microseconds per launch: hipEvents around windows of `reps` back-to-back launches, variants alternating window by "
                   "window, median with min and max over the windows; weights %g / %g, scale %g; shipped = the library's default "
                   "store form" % (TW, RW, SCALE), "reps": a.reps, "windows": a.windows, "shipped_store": SHIPPED}
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    for n in (int(v) for v in a.sizes.split(",")):
        poses, pi, pj, t, r = factors(n)
        d_p, d_i, d_j, d_t, d_r = up(poses), up(pi), up(pj), up(t), up(r)
        d_out = torch.empty((n, 28), dtype=torch.float64, device=dev)
        d_w = torch.empty((n, 4), dtype=torch.float64, device=dev)

        def plain():
            _lib.check(lib.nhip_resid_odometry_normal_eq_dev(d_t.data_ptr(), d_r.data_ptr(), d_i.data_ptr(), d_j.data_ptr(), n, TW, RW,
                                                             d_p.data_ptr(), len(poses), d_out.data_ptr(), stream))

        def robust(spec, store, weights):
            def call():
                if store is None:
                    os.environ.pop("NHIP_LOSS_STORE", None)
                else:
                    os.environ["NHIP_LOSS_STORE"] = store
                _lib.check(lib.nhip_resid_odometry_robust_normal_eq_dev(
                    d_t.data_ptr(), d_r.data_ptr(), d_i.data_ptr(), d_j.data_ptr(), n, TW, RW, C.byref(spec), d_p.data_ptr(), len(poses),
                    d_out.data_ptr(), d_w.data_ptr() if weights else None, stream))
            return call

        size = {"factors": n, "row_bytes": 224 * n, "weights_bytes": 32 * n}
        for kind in KINDS:
            spec = Loss(kind, SCALE).spec()
            variants = {"plain": plain}
            for store in ("direct", "staged"):
                for weights in (True, False):
                    variants["%s%s" % (store, "_weights" if weights else "")] = robust(spec, store, weights)
            variants["shipped"] = robust(spec, None, False)
            # the same bytes from both forms, and from the shipped default; NONE's are the plain kernel's
            got = {}
            for name, store in (("direct", "direct"), ("staged", "staged"), ("shipped", None)):
                d_out.fill_(-1.0), d_w.fill_(-1.0)
                robust(spec, store, True)()
                got[name] = (d_out.cpu().numpy().tobytes(), d_w.cpu().numpy().tobytes())
            d_out.fill_(-1.0)
            plain()
            plain_bytes = d_out.cpu().numpy().tobytes()
            res = {"forms_equal": got["direct"] == got["staged"] == got["shipped"],
                   "downweighted_share": float((np.frombuffer(got["direct"][1]).reshape(n, 4)[:, 2] < 0.5).mean())}
            if kind == "none":
                res["equal_plain"] = got["direct"][0] == plain_bytes
            for fn in variants.values():
                for _ in range(a.warmup * a.reps):
                    fn()
            torch.cuda.synchronize()
            us = {name: [] for name in variants}
            for _ in range(a.windows):
                for name, fn in variants.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.reps):
                        fn()
                    e1.record()
                    e1.synchronize()
                    us[name].append(1e3 * e0.elapsed_time(e1) / a.reps)
            for name, v in us.items():
                v = np.array(v)
                res[name] = {"median_us": float(np.median(v)), "min_us": float(v.min()), "max_us": float(v.max())}
            for name in ("direct", "staged", "direct_weights", "staged_weights"):
                res[name]["over_plain"] = res[name]["median_us"] / res["plain"]["median_us"]
            res["staged_over_direct"] = res["staged"]["median_us"] / res["direct"]["median_us"]
            res["staged_over_direct_weights"] = res["staged_weights"]["median_us"] / res["direct_weights"]["median_us"]
            size[kind] = res
        _lib.check(lib.nhip_dev_status(stream, None))
        out["%d_factors" % n] = size
    os.environ.pop("NHIP_LOSS_STORE", None)
    out["seconds"] = time.perf_counter() - t0
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    ok = all(out[k][kind]["forms_equal"] and out[k][kind].get("equal_plain", True) for k in out if k.endswith("_factors") for kind in KINDS)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
