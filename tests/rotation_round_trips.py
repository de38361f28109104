"""The paths of csm_bnb_kernel's bounds phase that keep a round trip off a wave's way (nhip_bnb.hip, nhip_bnb_bounds.h,
nhip_bnb_origin.h; profiles/r15_bounds_round_trips_isa.txt), the inputs at their seams, and the child process that runs
them in every form.  tests/test_rotation_round_trips_cpu.py checks the lists; tests/test_rotation_round_trips_gpu.py starts
the child and compares.

  rotations   A wave takes (cos, sin) of ALL its rotations k = wave, wave + WAVES, ... at once, one per lane, before the
              loop (rotation_terms_of_wave); the lanes past its last rotation read that rotation's entry again.  N_THETAS
              gives waves with no rotation, with one, with two or more, and a last rotation on either side of a full round.
              A search has an odd number of rotations (nhip_csm_match refuses an even one, and the drop-in call deals odd
              parts): 8 and 16 -- every wave exactly one, exactly two -- cannot reach the kernel.  They stay in the list, and
              the child records that the library refuses them; 7 / 9 and 15 / 17 are the counts on either side.
  points      The two slots of coarse_rotation's point prefetch outlive the rotation: the last turn loads chunks 0 and 1
              again (clamped for scans shorter than 128 points).  LENGTHS: one chunk, two, either side, a full scan, the
              longest the by-rotation form admits, and an empty scan, which loads nothing.
  staging     The pooled table goes to LDS in rounds of four loads per thread, 4 * THREADS 16-byte words a round, from a
              clamped index with the writes predicated.  What matters is where pool_bytes / 16 modulo ROUND falls against
              the four guards (0, 512, 1024, 1536).  The table's size is a product -- pool_rows * pool_pitch / 16 =
              (t + 12) * ceil((t + 16) / 16), t = ceil((side + 2 pad) / 8) -- so most residues do not occur: of 0-1, 511-513,
              1535-1537 and 2046-2047 only 513 does for a table that fits LDS.  POOL_SIDES takes, on either side of the seams
              at 0, 512 and 1536, the nearest residue that any side gives (nearest_residues; the CPU test holds the list
              against csm.grid_layout and against every other side), and GLOBAL_SIDE is the smallest side whose pooled table
              bnb_plan leaves in global memory (csm_bnb_kernel<*, false, *, *>, whose gather reads one row ahead too).
  rows        A list entry's 11 rows are read one row ahead.  EDGE_SHIFT (max_shift = 8: 32 cells of border) and the points of
              edge_scan put window origins on the last stored row, whose rows y .. y + 10 reach the zero rows below the
              pooled image, and on the lowest row the clamp admits (pooled row 1; 2 * hy + 1 stored rows lie above it).

    python -m tests.rotation_round_trips CELL_BITS OUT.npz     (in a process started with NHIP_TUNABLES=1)"""
import json
import math
import os
import sys

import numpy as np

from tests.point_prefetch import EVERY_ADD, FORMS, INSTR

CHUNK = 64
PD, WAVES = 2, 8                   # PD of coarse_rotation; BNB_WAVES = SPLIT_WAVES of csm_bnb_kernel
THREADS = CHUNK * WAVES
ROUND = 4 * THREADS                # 16-byte words of the pooled table staged per round of the workgroup
N_THETAS = (1, 7, 8, 9, 15, 16, 17, 61)
LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 1081, 1088)
N_THETA = 9                        # of the groups that vary something else: wave 0 has two rotations, the others one
NXY, THETA_STEP = 17, math.radians(1.0)
SRC_SCAN, TGT_SCAN = 3, 9          # two scans of the small bag that see the same walls
RANGE_M, MAX_SHIFT, EDGE_SHIFT = 30.0, 40, 8
BASE_SIDE = 400
# side: pool_bytes / 16 modulo ROUND (see the top of the file)
POOL_SIDES = {2176: 16, 392: 510, 1288: 513, 936: 1530, 944: 1540, 2168: 2044}
GLOBAL_SIDE = 2753
SEAMS = (0, 512, 1536, ROUND)      # the guards of loads 0, 1 and 3 of a round, and the round's end
LDS_MAX, ORG_LDS, QCAP, LDS_TAIL_BYTES = 160 * 1024, 8 * 17 * 64 * 4, 1024, 64  # nhip_bnb_host.hip, nhip_bnb_params.h


def wave_rotations(n_theta):
    """Rotations of each wave of the workgroup."""
    return [len(range(w, n_theta, WAVES)) for w in range(WAVES)]


def res_of(side):
    """A cell size that gives exactly `side` cells: floor(2 range / res) with the quotient half a cell inside."""
    return 2.0 * RANGE_M / (side + 0.5)


def pooled_words(side, pad):
    """pool_bytes / 16 as make_layout (nhip_layout.hip) sizes the pooled table."""
    t = (side + 2 * pad + 7) // 8
    return (t + 12) * (((t + 16 + 15) & ~15) // 16)


def pad_of(max_shift):
    return ((2 * max_shift + 16) + 3) & ~3


def pool_in_lds(words, n_theta=N_THETA):
    """bnb_plan's rule (nhip_bnb_host.hip): the fused form's LDS with the pooled table staged is within LDS_MAX."""
    return max(16 * words, ORG_LDS) + n_theta * 128 * 4 + QCAP * 8 + LDS_TAIL_BYTES <= LDS_MAX


def nearest_residues(sides=range(8, 4096)):
    """{(seam, side of it): residue}: for each seam the nearest residue below it and the nearest at or above it that the
    pooled table of any side (LDS-resident at N_THETA rotations, MAX_SHIFT) gives.  None where no side gives one."""
    have = sorted({pooled_words(s, pad_of(MAX_SHIFT)) % ROUND for s in sides if pool_in_lds(pooled_words(s, pad_of(MAX_SHIFT)))})
    out = {}
    for seam in SEAMS:
        below = [r for r in have if r < seam]
        above = [r for r in have if seam <= r < ROUND]
        out[(seam, "below")] = below[-1] if below else None
        out[(seam, "above")] = above[0] if above else None
    return out


def edge_scan(scan):
    """The first 300 beams of `scan`, then rows of points just inside and well beyond the table on all four sides and in
    its corners: their window origins clamp to the first and the last rows and columns the lattice admits."""
    t = np.linspace(-RANGE_M - 4.0, RANGE_M + 4.0, 50, dtype=np.float32)
    parts = [np.asarray(scan[:300], np.float32)]
    for d in (RANGE_M - 0.31, RANGE_M + 3.0):
        for sgn in (-1.0, 1.0):
            parts.append(np.stack([t, np.full_like(t, sgn * d)], axis=1))
            parts.append(np.stack([np.full_like(t, sgn * d), t], axis=1))
    return np.concatenate(parts).astype(np.float32)


def origin_rows(pts, side, max_shift, h=NXY // 2):
    """Pooled row of the window origin of each point at the search's centre rotation (theta0 = 0: the identity) -- the
    clamp of window_origin (nhip_bnb_origin.h) on the y coordinate, restated."""
    pad, half, res = pad_of(max_shift), side // 2, res_of(side)
    iy = np.floor(np.asarray(pts, np.float64)[:, 1] / res).astype(np.int64)
    iy = np.minimum(np.maximum(iy, -h - 1 - half), side + h - half)
    return (iy + half - h + pad) >> 3


def spec_of(csm, side, max_shift, cell_bits):
    return csm.grid_spec(RANGE_M, res_of(side), 2.0, 1e-10, max_shift, cell_bits, skip_map=cell_bits == 16)


def groups(bag):
    """[(name, side, max_shift, scans, n_theta)]: one list of pairs (every scan against TGT_SCAN's table) per group."""
    src, tgt = bag.scans[SRC_SCAN], bag.scans[TGT_SCAN]
    short = [np.resize(src, (129, 2)).astype(np.float32), src.astype(np.float32), tgt.astype(np.float32)]  # (the target scores on any table)
    out = [("rot%d" % n, BASE_SIDE, MAX_SHIFT, short, n) for n in N_THETAS]
    lengths = [np.resize(src, (n, 2)).astype(np.float32) for n in LENGTHS]
    out.append(("lengths", BASE_SIDE, MAX_SHIFT, lengths, N_THETA))
    out.append(("rows", BASE_SIDE, EDGE_SHIFT, [edge_scan(src), edge_scan(tgt)] + lengths[5:9], N_THETA))
    out += [("pool%d" % s, s, MAX_SHIFT, short, N_THETA) for s in list(POOL_SIDES) + [GLOBAL_SIDE]]
    return out, tgt.astype(np.float32)


def run(cell_bits, out_path):
    from nautilus_amd import csm, synth
    assert os.environ.get("NHIP_TUNABLES") == "1", "the forms are chosen through switches a process reads only then"
    todo, tgt = groups(synth.SynthBag(48))
    arrays, meta = {}, {}
    for group, side, max_shift, scans, n_theta in todo:
        if n_theta % 2 == 0:  # (refused: what the library says goes to the parent)
            st = csm.ScanTable(*csm.pack_scans([tgt] + scans))
            grids = csm.LikelihoodGrids(st, np.array([0], np.int32), spec_of(csm, side, max_shift, cell_bits))
            try:
                csm.match_pairs(st, grids, np.array([1], np.int32), np.zeros(1, np.int32), np.zeros(1),
                                csm.search_spec(n_theta, NXY, NXY, THETA_STEP))
                meta[group] = {"refused": None}
            except Exception as e:  # (NhipError)
                meta[group] = {"refused": str(e)}
            grids.close()
            st.close()
            continue
        st = csm.ScanTable(*csm.pack_scans([tgt] + scans))
        spec = spec_of(csm, side, max_shift, cell_bits)
        grids = csm.LikelihoodGrids(st, np.array([0], np.int32), spec)
        n = len(scans)
        src, slot, th0 = np.arange(1, n + 1, dtype=np.int32), np.zeros(n, np.int32), np.zeros(n)
        meta[group] = {"side": int(grids.layout.side), "pool_words": int(grids.layout.pool_bytes // 16), "n_pairs": n}

        def once(name, search, env):
            os.environ.update(env)
            try:
                csm.bnb_stats_levels()  # (reset)
                rec, sums = csm.match_pairs(st, grids, src, slot, th0, search)
                launch = csm.last_launch()
            finally:
                for k in env:
                    os.environ.pop(k, None)
            arrays["rec_%s_%s" % (group, name)] = np.frombuffer(rec.tobytes(), np.uint8)
            arrays["sum_%s_%s" % (group, name)] = sums
            meta[group][name] = launch

        bnb = csm.search_spec(n_theta, NXY, NXY, THETA_STEP)
        for name, (env, _) in FORMS.items():
            once(name, bnb, env)
            once(name + "_instr", bnb, dict(env, **INSTR))
        ex = csm.search_spec(n_theta, NXY, NXY, THETA_STEP, exhaustive=True)
        for name, env in EVERY_ADD.items():
            once(name, ex, env)
        grids.close()
        st.close()
    np.savez(out_path, meta=np.array(json.dumps(meta)), **arrays)


if __name__ == "__main__":
    run(int(sys.argv[1]), sys.argv[2])
