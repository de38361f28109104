"""What the relative-pose factors cost and what they buy (K23, nhip_relpose.hip).

Kernels (default): nhip_resid_relpose_normal_eq_dev at 1,000 and 100,000 factors, every loss kind, in both forms of its row store
(NHIP_RELPOSE_STORE, read per launch in a process with NHIP_TUNABLES=1), beside nhip_resid_odometry_robust_normal_eq_dev on
factors over the same poses in the same process.  hipEvents around windows of --reps back-to-back launches, the variants
alternating window by window after a warm-up of each; per-launch medians with min and max over the windows.  The two forms'
outputs are compared for byte equality at every size and kind.

Loops (--loops cpu,hip): the loop tests' 32-scan bag (tests/loss_loop.KW) with --lc-refine icp at three drifts, its closures as
the world-frame factor, as relative-pose factors at the weights' information, and at the refinement's H: err_lc_m and
t_lc_solve_s, on the CPU backend and / or on the device (both linear solvers).

  python tools/relpose_bench.py [--windows 15] [--reps 200] [--warmup 3] [--sizes 1000,100000] [--loops cpu,hip] [--no-kernels]
                                [--out profiles/relpose_bench.json]
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

TW, RW, SCALE = 10.0, 10.0, 1.0  # the world-frame closures' weights, --lc-loss-scale's default
SHIPPED = "staged"                # nhip_relpose.hip's STAGED_BY_DEFAULT, restated
ROOM_INFO = np.array([420.0, -35.0, 610.0, 230.0, 95.0, 16000.0])  # the size of a room pair's H
DRIFTS = (0.3, 5.0, 20.0)


def factors(n, seed=5):
    """n closure-like factors over a 4,000-pose track, as relative-pose factors and as world-frame ones: most close to a few
    centimetres, one in five is displaced by metres."""
    rng = np.random.default_rng(seed)
    n_poses = 4000
    poses = np.concatenate([np.cumsum(rng.normal(0, 0.3, (n_poses, 2)), axis=0), rng.uniform(-np.pi, np.pi, (n_poses, 1))], axis=1)
    pi = rng.integers(0, n_poses, n).astype(np.int32)
    pj = ((pi + rng.integers(1, n_poses, n)) % n_poses).astype(np.int32)  # (never the same pose)
    t = poses[pj, :2] - poses[pi, :2] + rng.normal(0, 0.03, (n, 2))
    r = poses[pj, 2] - poses[pi, 2] + rng.normal(0, 0.01, n)
    bad = rng.random(n) < 0.2
    t[bad] += rng.uniform(-3, 3, (int(bad.sum()), 2))
    ca, sa = np.cos(poses[pi, 2]), np.sin(poses[pi, 2])
    z = np.stack([ca * t[:, 0] + sa * t[:, 1], -sa * t[:, 0] + ca * t[:, 1], np.cos(r), np.sin(r)], axis=1)
    info = ROOM_INFO[None, :] * rng.uniform(0.3, 3.0, (n, 1))
    return poses, pi, pj, t.astype(np.float32), r.astype(np.float32), np.ascontiguousarray(z), np.ascontiguousarray(info)


def kernels(a, out):
    import torch
    from nautilus_amd import _lib
    from nautilus_amd.loss import KINDS, Loss
    lib = _lib.load()
    if _lib.device_count() == 0:
        raise SystemExit("relpose_bench: no HIP device")
    dev = torch.device("cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    out.update({"note": "microseconds per launch: hipEvents around windows of `reps` back-to-back launches, variants alternating window "
                        "by window, median with min and max over the windows; odometry = nhip_resid_odometry_robust_normal_eq_dev "
                        "(weights %g / %g) on factors over the same poses; scale %g" % (TW, RW, SCALE),
                "reps": a.reps, "windows": a.windows, "shipped_store": SHIPPED})
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    ok = True
    for n in (int(v) for v in a.sizes.split(",")):
        poses, pi, pj, t, r, z, info = factors(n)
        d_p, d_i, d_j, d_t, d_r, d_z, d_l = up(poses), up(pi), up(pj), up(t), up(r), up(z), up(info)
        d_out = torch.empty((n, 28), dtype=torch.float64, device=dev)
        d_w = torch.empty((n, 4), dtype=torch.float64, device=dev)

        def odometry(spec):
            def call():
                _lib.check(lib.nhip_resid_odometry_robust_normal_eq_dev(
                    d_t.data_ptr(), d_r.data_ptr(), d_i.data_ptr(), d_j.data_ptr(), n, TW, RW, C.byref(spec), d_p.data_ptr(), len(poses),
                    d_out.data_ptr(), None, stream))
            return call

        def relpose(spec, store, weights):
            def call():
                if store is None:
                    os.environ.pop("NHIP_RELPOSE_STORE", None)
                else:
                    os.environ["NHIP_RELPOSE_STORE"] = store
                _lib.check(lib.nhip_resid_relpose_normal_eq_dev(
                    d_z.data_ptr(), d_l.data_ptr(), d_i.data_ptr(), d_j.data_ptr(), n, C.byref(spec), d_p.data_ptr(), len(poses),
                    d_out.data_ptr(), d_w.data_ptr() if weights else None, None, stream))
            return call

        size = {"factors": n, "row_bytes": 224 * n, "weights_bytes": 32 * n}
        for kind in KINDS:
            spec = Loss(kind, SCALE).spec()
            variants = {"odometry": odometry(spec), "direct": relpose(spec, "direct", False), "staged": relpose(spec, "staged", False),
                        "staged_weights": relpose(spec, "staged", True), "shipped": relpose(spec, None, False)}
            got = {}
            for name, store in (("direct", "direct"), ("staged", "staged"), ("shipped", None)):
                d_out.fill_(-1.0), d_w.fill_(-1.0)
                relpose(spec, store, True)()
                got[name] = (d_out.cpu().numpy().tobytes(), d_w.cpu().numpy().tobytes())
            res = {"forms_equal": got["direct"] == got["staged"] == got["shipped"],
                   "downweighted_share": float((np.frombuffer(got["direct"][1]).reshape(n, 4)[:, 2] < 0.5).mean())}
            ok = ok and res["forms_equal"]
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
            for name in ("direct", "staged", "staged_weights", "shipped"):
                res[name]["over_odometry"] = res[name]["median_us"] / res["odometry"]["median_us"]
            res["staged_over_direct"] = res["staged"]["median_us"] / res["direct"]["median_us"]
            size[kind] = res
        _lib.check(lib.nhip_dev_status(stream, None))
        out["%d_factors" % n] = size
    os.environ.pop("NHIP_RELPOSE_STORE", None)
    return ok


def loops(which, out):
    """The loop table: per backend and linear solver, per drift, {world, relative_weights, relative_h}: [lc_accepted, err_lc_m,
    t_lc_solve_s]."""
    import examples.slam_loop as loop
    from nautilus_amd import hostside, posegraph
    from tests import loss_loop as LL
    configs = []
    if "cpu" in which:
        from oracle.cpu_backend import OracleBackend
        configs.append(("cpu_host", OracleBackend, "host"))
    if "hip" in which:
        configs += [("hip_host", posegraph.HipBackend, "host"), ("hip_device", posegraph.HipBackend, "device")]
    information = hostside.relpose_information
    weights_only = lambda refined, n=None, **kw: information(None, n=len(refined) if refined is not None else n, **kw)
    table = {}
    for name, make, solver in configs:
        for drift in DRIFTS:
            row = {}
            for factor, fn in (("world", None), ("relative_weights", weights_only), ("relative_h", information)):
                hostside.relpose_information = fn or information
                try:
                    r = loop.run(backend=make(), drift_th_deg=drift, lc_refine="icp", linear_solver=solver,
                                 lc_factor=None if factor == "world" else "relative", **LL.KW)
                finally:
                    hostside.relpose_information = information
                row[factor] = {"lc_accepted": r["lc_accepted"], "err_lc_m": r["err_lc_m"], "t_lc_solve_s": r["t_lc_solve_s"],
                               "lc_info_from_icp": r.get("lc_info_from_icp"), "lc_info_eig": [r.get("lc_info_eig_min"), r.get("lc_info_eig_max")]}
            table.setdefault(name, {})["drift_%g_deg" % drift] = row
            print(name, drift, json.dumps(row), flush=True)
    out["loops"] = table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="1000,100000")
    ap.add_argument("--loops", default="", help="comma list of cpu, hip: also take the loop table on those backends")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relpose_bench.json"))
    a = ap.parse_args()
    t0 = time.perf_counter()
    out, ok = {}, True
    if os.path.exists(a.out):  # (the kernels and the loops may be taken in separate runs: the file keeps both)
        with open(a.out) as f:
            out = json.load(f)
    if not a.no_kernels:
        ok = kernels(a, out)
    if a.loops:
        loops(a.loops.split(","), out)
    out["seconds"] = time.perf_counter() - t0
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
