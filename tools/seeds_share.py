"""The seeds of the bounds kernel on the bench's 10,000 pairs (instrumented build): their share of the first kernel's workgroup
time, their wave clocks by part, and the counts a seed pass without strip bounds rests on -- with NHIP_BNB_SEED_BOUNDS=1
(every seed takes its sub-block bounds: the path before round 19, which alone can count the bounds that are 0) and as shipped.

    python tools/seeds_share.py [CELL_BITS]        (16)"""
import os, sys
os.environ["NHIP_TUNABLES"] = "1"; os.environ["NHIP_BNB_INSTRUMENT"] = "1"; os.environ["NHIP_BNB_STATS"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, bench
from nautilus_amd import csm, sharding
bits = int(sys.argv[1]) if len(sys.argv) > 1 else 16
wl = bench.Workload("weak", 1)
plan = sharding.ShardPlan(wl.src, wl.tgt, wl.th0, 1, None)
m = bench.HipMatcher(wl, plan.shard(0), torch.device("cuda:0"), bits)
for name, env in (("seed bounds always (NHIP_BNB_SEED_BOUNDS=1)", {"NHIP_BNB_SEED_BOUNDS": "1"}), ("as shipped", {})):
    os.environ.update(env)
    m.step(); torch.cuda.synchronize(); csm.bnb_stats_levels(); csm.bnb_stats_seeds()
    m.step(); torch.cuda.synchronize()
    launch, lv, sd = csm.last_launch(), csm.bnb_stats_levels(), csm.bnb_stats_seeds()
    for k in env:
        os.environ.pop(k)
    print("==", name, "| %d-bit cells | form %s, seed_bounds %s" % (bits, launch["form"], launch["seed_bounds"]))
    print({k: lv[k] for k in ("clk_bounds", "clk_seeds", "blocks_whole", "sub_blocks", "candidates_refined", "pose_evals16")})
    print(sd)
    print("seeds / (bounds + seeds) of the first kernel's workgroup time: %.3f" % (lv["clk_seeds"] / float(lv["clk_seeds"] + lv["clk_bounds"])))
    parts = [sd["clk_seed_origins"], sd["clk_seed_sub_bounds"], sd["clk_seed_exact"]]
    print("seed passes' wave clocks by part: origins %.3f, sub-block bounds %.3f, exact sums %.3f of %d; per pass %.0f"
          % tuple([p / float(max(sum(parts), 1)) for p in parts] + [sum(parts), sum(parts) / float(max(sd["seed_passes"], 1))]))
