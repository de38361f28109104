"""The gather of csm_bnb_kernel's bounds (nhip_bnb_bounds.h coarse_rotation): the scans at the seams of its passes, in both
forms of the pooled table, and the child process that runs them in every form.  tests/test_gather_rows_cpu.py checks the
lists; tests/test_gather_rows_gpu.py starts the child and compares.

A rotation's points become a list of RUNS -- consecutive points that share a pooled entry, cut at 64 -- and a gather pass takes
64 entries, one per lane: the 11 rows of 16 bytes of the lane's entry, row by row, the row after the one being added already
in flight (in both forms of the table; two rows ahead were measured in round 19 and bought nothing: profiles/r19_seeds.txt),
weighted by the run length.
A lane may gather a total run length of LANE_WEIGHT = 64 between two reductions; a pass that would exceed it reduces first.
The bounds themselves stay inside the kernel.  What they decide is visible: on `plateau` every bound equals every sum, so every
block stays alive exactly while no bound comes out too low, and the instrumented build's counts are
tests/lattice_edge.py's saturated prediction; and the records are those of the kernels that perform every add.

  lds      tests/lattice_edge.py's geometry (240 cells, the pooled table in LDS), `plateau`, 17 x 17 x 3: coincident points --
           run lengths 0 (an empty scan), 1, 63, 64, 65, 128, 129 -- and `early`: a run of 64, 63 runs of 1 in 63 other
           entries, a run of 64: entry 64 is lane 0's second, and 64 + 64 forces the reduction before its pass
  global   tests/rotation_round_trips.py's smallest table that bnb_plan leaves in global memory, 17 x 17 x 9, the same run
           lengths on a wall point of the target scan, and `early` along it

    python -m tests.gather_rows CELL_BITS OUT.npz     (in a process started with NHIP_TUNABLES=1)"""
import json
import os
import sys

import numpy as np

from tests import lattice_edge as L
from tests import rotation_round_trips as RT
from tests import saturated_cases as S
from tests.point_prefetch import EVERY_ADD, FORMS, INSTR

RUN_MAX, LANE_WEIGHT, ENTRIES = 64, 64, 64   # nhip_bnb_bounds.h: a run's longest, a lane's weight between reductions, a pass
RUNS = (0, 1, 63, 64, 65, 128, 129)
NXY, LDS_THETA = 17, 3
A_CELL, B_CELL = (80, 80), (80, 160)         # the two long runs of `early` (cells of the plateau's top level)


def singles():
    """63 cells of the plateau, 8 apart: 63 pooled entries, none A's or B's."""
    return [(72 + 8 * (i % 9), 96 + 8 * (i // 9)) for i in range(63)]


def early_lds():
    return np.concatenate([S.cluster(A_CELL, 64)] + [S.cluster(c, 1) for c in singles()] + [S.cluster(B_CELL, 64)]).astype(np.float32)


def lds_scans():
    """[(name, points)]"""
    return [("run%d" % n, S.cluster((L.CENTRE, L.CENTRE), n).astype(np.float32).reshape(-1, 2)) for n in RUNS] + [("early", early_lds())]


def global_scans(tgt):
    a, b = np.asarray(tgt[100], np.float32), np.asarray(tgt[300], np.float32)
    step = np.float32(0.2)  # (more than the 8 cells of a pooled entry: 8 * 60 / 2753.5 = 0.174 m)
    line = np.stack([a + np.array([step * (i + 1), 0], np.float32) for i in range(63)])
    early = np.concatenate([np.tile(a, (64, 1)), line, np.tile(b, (64, 1))]).astype(np.float32)
    return [("run%d" % n, np.tile(a, (n, 1)).astype(np.float32).reshape(-1, 2)) for n in RUNS] + [("early", early)]


def run_lengths(entries):
    """The run list of a rotation whose points have pooled entries `entries` (any hashable, in point order)."""
    out = []
    for i, e in enumerate(entries):
        if i and e == entries[i - 1] and out[-1] < RUN_MAX:
            out[-1] += 1
        else:
            out.append(1)
    return out


def lds_entries(points):
    """Pooled entry (row, column) of each point's window origin at the centre rotation (tests/lattice_edge.py lookup_origin)."""
    out = []
    for p in points:
        row, col = L.lookup_origin(p, 0, 1, NXY // 2, NXY // 2)
        out.append(((row + L.PAD) >> 3, (col + L.PAD) >> 3))
    return out


def reductions_before_pass(runs):
    """Per gather pass of 64 entries: whether some lane's weight since the last reduction would pass LANE_WEIGHT with it."""
    weight, out = [0] * ENTRIES, []
    for p in range(0, len(runs), ENTRIES):
        chunk = runs[p:p + ENTRIES]
        over = any(weight[i] + c > LANE_WEIGHT for i, c in enumerate(chunk))
        if over:
            weight = [0] * ENTRIES
        for i, c in enumerate(chunk):
            weight[i] += c
        out.append(over)
    return out


def run(bits, out_path):
    from nautilus_amd import csm, synth
    assert os.environ.get("NHIP_TUNABLES") == "1", "the forms are chosen through switches a process reads only then"
    arrays, meta = {}, {}
    tgt = synth.SynthBag(48).scans[RT.TGT_SCAN].astype(np.float32)
    todo = [("lds", L.target("plateau"), lds_scans(), L.spec_of(csm, bits), LDS_THETA, L.THETA_STEP),
            ("global", tgt, global_scans(tgt), RT.spec_of(csm, RT.GLOBAL_SIDE, RT.MAX_SHIFT, bits), RT.N_THETA, RT.THETA_STEP)]
    for group, target, scans, spec, n_theta, step in todo:
        st = csm.ScanTable(*csm.pack_scans([target] + [p for _, p in scans]))
        grids = csm.LikelihoodGrids(st, np.array([0], np.int32), spec)
        n = len(scans)
        src, slot, th0 = np.arange(1, n + 1, dtype=np.int32), np.zeros(n, np.int32), np.zeros(n)
        meta[group] = {"side": int(grids.layout.side), "pool_words": int(grids.layout.pool_bytes // 16), "n_pairs": n}

        def once(search, env, src=src, slot=slot, th0=th0):
            os.environ.update(env)
            try:
                csm.bnb_stats_levels()  # (reset)
                rec, sums = csm.match_pairs(st, grids, src, slot, th0, search)
                launch = csm.last_launch()
                stats = {k: int(v) for k, v in csm.bnb_stats_levels().items() if k in L.COUNTED} if "NHIP_BNB_STATS" in env else None
            finally:
                for k in env:
                    os.environ.pop(k, None)
            return np.frombuffer(rec.tobytes(), np.uint8), sums, launch, stats

        bnb = csm.search_spec(n_theta, NXY, NXY, step)
        for name, (env, _) in FORMS.items():
            for v, e in ((name, env), (name + "_instr", dict(env, **INSTR))):
                arrays["rec_%s_%s" % (group, v)], arrays["sum_%s_%s" % (group, v)], meta[group][v], _ = once(bnb, e)
            if group == "lds":  # the saturated pairs alone, one at a time, counted
                meta[group][name + "_counts"] = [once(bnb, dict(env, **INSTR), src[i:i + 1], slot[i:i + 1], th0[i:i + 1])[3] for i in range(n)]
        ex = csm.search_spec(n_theta, NXY, NXY, step, exhaustive=True)
        for name, env in EVERY_ADD.items():
            arrays["rec_%s_%s" % (group, name)], arrays["sum_%s_%s" % (group, name)], _, _ = once(ex, env)
        grids.close()
        st.close()
    np.savez(out_path, meta=np.array(json.dumps(meta)), **arrays)


if __name__ == "__main__":
    run(int(sys.argv[1]), sys.argv[2])
