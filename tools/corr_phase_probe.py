"""corr_search_kernel's time on bench.bench_icp's workload (9,945 blocks of 1081-point scans): the product library and every
build/variants/libcorr_*.so present (other builds of the same library, selected through NHIP_LIB), one subprocess each (GPU
box).  `one` is a single leg: it prints corr_search_ms and normal_eq_ms of the library NHIP_LIB names."""
import glob, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if len(sys.argv) > 1 and sys.argv[1] == "one":
    sys.path.insert(0, ROOT)
    import bench
    from nautilus_amd import synth, csm
    bag = synth.SynthBag(1000, dense=True)
    xy, off = csm.pack_scans(bag.scans)
    r = bench.bench_icp(bag, xy, off, False)
    print("corr_search_ms %.4f normal_eq_ms %.4f" % (r["corr_search_ms"], r["normal_eq_ms"]))
    sys.exit(0)
for lib in [None] + sorted(glob.glob(os.path.join(ROOT, "build", "variants", "libcorr_*.so"))):
    env = dict(os.environ)
    if lib:
        env["NHIP_LIB"] = lib
    p = subprocess.run([sys.executable, __file__, "one"], env=env, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
    print(os.path.basename(lib) if lib else "product", p.stdout.decode().strip().splitlines()[-1:], flush=True)
