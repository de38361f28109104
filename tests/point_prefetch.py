"""The point loops of the branch-and-bound matcher's kernels that keep loads in flight across turns -- coarse_rotation
(nhip_bnb_bounds.h: BOUNDS_SLOTS chunks of 64 points per turn, every form's bounds) and the seeds' cache_origins
(nhip_bnb_origin.h: ORIGIN_SLOTS chunks per turn; the candidates' kernels walk the same chunks through a ring) -- the scan
lengths at their seams, and the child process that runs them in every form.  tests/test_point_prefetch_cpu.py checks the
lists (and that the slot counts are the headers'); tests/test_point_prefetch_gpu.py starts the child and compares.

A turn works `slots` chunks: the first body always, the later ones only where the scan reaches them, and every slot's next load
is clamped to the scan's last point.  What can go wrong is a scan that ends in a given body of a given turn, or exactly on one.

    python -m tests.point_prefetch CELL_BITS OUT.npz     (in a process started with NHIP_TUNABLES=1)"""
import json
import math
import os
import sys

import numpy as np

CHUNK = 64
BOUNDS_SLOTS, ORIGIN_SLOTS = 2, 3  # PD of coarse_rotation, D of cache_origins
BY_ROTATION_MAX = 1088            # the longest scan the by-rotation form admits (17 chunks); longer ones take the general kernel
TURNS = 3


def seam_lengths(slots):
    """One length on each side of every multiple of 64 * slots, and the multiple, up to three turns."""
    out = []
    for t in range(1, TURNS + 1):
        m = CHUNK * slots * t
        out += [m - 1, m, m + 1]
    return out


LENGTHS = sorted(set(
    [1, 63, 64, 65, 127, 128, 129]                          # one chunk, two chunks, either side
    + seam_lengths(BOUNDS_SLOTS) + seam_lengths(ORIGIN_SLOTS)
    + [100, 160, 300]                                      # ends inside a later body of a turn (see ends_in)
    + [1081, 1087, 1088]                                   # a full scan; the last lengths of the by-rotation form
    + [1089, 1151, 1152, 1153]))                           # the general kernel: its bounds run the same loop (turn 9 of 128)


def ends_in(n, slots):
    """(turn, body, full): the turn and the body (slot) of it that holds the scan's last point; full: the point is the body's
    last lane."""
    last = (n - 1) // CHUNK
    return last // slots, last % slots, n % CHUNK == 0


SRC_SCAN, TGT_SCAN = 3, 9   # two scans of the small bag that see the same walls
RANGE_M, RES = 30.0, 0.15   # a 400-cell table
N_THETA, NXY, THETA_STEP = 3, 17, math.radians(1.0)

SPLIT_ONE = {"NHIP_BNB_KERNELS": "1", "NHIP_BNB_SPLIT": "1"}
HAND_OVER = {"NHIP_BNB_KERNELS": "2", "NHIP_BNB_HEAVY_MIN": "1", "NHIP_BNB_KEEP_RANKS": "0"}
# name -> (environment, form id nhip_csm_last_launch reports)
FORMS = {
    "fused": ({"NHIP_BNB_KERNELS": "1"}, 0),
    "hand_over": (HAND_OVER, 0),
    "split": (SPLIT_ONE, 1),
    "split_rounds": ({"NHIP_BNB_KERNELS": "1", "NHIP_BNB_SPLIT": "1", "NHIP_BNB_SPLIT_BATCH": "2", "NHIP_BNB_SPLIT_MIN": "1",
                      "NHIP_BNB_SPLIT_MAX": "5"}, 3),
}
INSTR = {"NHIP_BNB_INSTRUMENT": "1", "NHIP_BNB_STATS": "1"}
EVERY_ADD = {"every_add": {}, "every_add_rows": {"NHIP_CSM_SMALL": "0"}, "every_add_dense": {"NHIP_CSM_DENSE": "1"}}


def scans_of(bag):
    """The bag's scans, then one scan per length: the first n beams of SRC_SCAN (repeated from the start where n is longer)."""
    return list(bag.scans) + [np.resize(bag.scans[SRC_SCAN], (n, 2)).astype(np.float32) for n in LENGTHS]


def run(cell_bits, out_path):
    from nautilus_amd import csm, synth
    assert os.environ.get("NHIP_TUNABLES") == "1", "the forms are chosen through switches a process reads only then"
    bag = synth.SynthBag(48)
    scans = scans_of(bag)
    st = csm.ScanTable(*csm.pack_scans(scans))
    spec = csm.grid_spec(RANGE_M, RES, 2.0, 1e-10, 40, cell_bits, skip_map=cell_bits == 16)
    grids = csm.LikelihoodGrids(st, np.array([TGT_SCAN], np.int32), spec)
    n = len(LENGTHS)
    src = np.arange(len(bag.scans), len(bag.scans) + n, dtype=np.int32)
    slot, th0 = np.zeros(n, np.int32), np.zeros(n)
    arrays, meta = {}, {}

    def once(name, search, env):
        os.environ.update(env)
        try:
            csm.bnb_stats_levels()  # (reset)
            rec, sums = csm.match_pairs(st, grids, src, slot, th0, search)
            launch = csm.last_launch()
            stats = {k: int(v) for k, v in csm.bnb_stats_levels().items()} if "NHIP_BNB_STATS" in env else None
        finally:
            for k in env:
                os.environ.pop(k, None)
        arrays["rec_" + name] = np.frombuffer(rec.tobytes(), np.uint8)
        arrays["sum_" + name] = sums
        meta[name] = {"launch": launch, "stats": stats}

    bnb = csm.search_spec(N_THETA, NXY, NXY, THETA_STEP)
    for name, (env, _) in FORMS.items():
        once(name, bnb, env)
        once(name + "_instr", bnb, dict(env, **INSTR))
    ex = csm.search_spec(N_THETA, NXY, NXY, THETA_STEP, exhaustive=True)
    for name, env in EVERY_ADD.items():
        once(name, ex, env)
    np.savez(out_path, meta=np.array(json.dumps(meta)), **arrays)


if __name__ == "__main__":
    run(int(sys.argv[1]), sys.argv[2])
