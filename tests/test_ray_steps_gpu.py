"""The steps of the grid ray at which the float estimate of nhip_ray.h is one off (tests/ray_steps.py: LOW one too low, HIGH
one too high), walked by the four kernels that use it and compared for EQUALITY with the references, which divide python
integers: K14's occ_trace_kernel (rdiv), K15's fs_check_kernel (rdiv_straight) and fs_trace_kernel (rdiv), K21's
rs_map_kernel (rdiv).  tests/test_ray_steps_cpu.py proves on the CPU that each comparison made here fails when a correction
is missing.  Every test is a call of the existing entry points."""
import numpy as np
import pytest

from nautilus_amd import _lib, csm
from tests import freespace_reference as FR
from tests import rangesig_reference as RR
from tests import ray_steps as S
from tests.test_freespace_gpu import Rig
from tests.test_occupancy_gpu import check as occupancy_check
from tests.test_rangesig_gpu import device_map, product_spec

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- K14
def test_occupancy_low_steps(gpu):
    """every LOW beam whole inside the window: a scan per beam, all beams in one scan, the short ones on a lattice of origins"""
    for name, packed, spec, walked in S.occupancy_low_cases():
        occupancy_check(*packed, spec, name)


@pytest.mark.parametrize("i", range(len(S.HIGH)))
def test_occupancy_high_steps(gpu, i):
    """max_ray_cells 4096 and a window of 3 .. 8 rows, up to 16384 wide, on the row of each off step of HIGH beam i: the box has
    8193 rows, more than a hundred bands, and k is narrowed to the band at (2 ra - 1) n in the millions.  The origin of two
    scans lies outside the window, that of the third inside it."""
    for name, packed, spec, walked in S.occupancy_high_cases(i):
        grid, hits, misses, stats = occupancy_check(*packed, spec, name)
        assert stats[:5].tolist() == [3, 0, 1 + 2 * len(S.HIGH), 0, 0] and misses.any()


# ---------------------------------------------------------------- K15
@pytest.mark.parametrize("case", S.check_cases(), ids=lambda c: c["name"])
def test_check_counts_the_right_cell_of_an_off_step(gpu, case):
    """fs_check_kernel (rdiv_straight) on the 1200-cell grid: per off step a pair whose target has its one hit on the step's
    right cell and a pair whose hit lies on the cell the uncorrected estimate names; chunk groups of one, two and four with
    the step in their first and in their last chunk (asserted on the CPU)."""
    rig = Rig(case["scans"], [0, 1, 2, 3], S.check_grid_spec())
    for fs in case["fs"]:
        want = S.check_counts(case, fs)
        got, info, rc = rig.counts(case["src"], case["tgt"], case["theta0"], case["poses"], case["lattice"], fs, case["origin"])
        assert rc == _lib.NHIP_OK, info
        assert got.dtype == np.int32 and np.array_equal(got, want), (case["name"], fs, np.argwhere(got != want)[:4])


def test_trace_low_steps(gpu):
    """fs_trace_kernel (rdiv) with LOW beams as a target's beams, at grid sides 120 and 1200: the free planes.  No HIGH beam
    fits a grid (half its side would have to reach 2457 cells, a slot of some 50 MB), so the trace's `q--` is NOT walked
    here: that branch is covered through K14 alone, whose kernel holds the same loop over the same rdiv."""
    for side, reach, targets in S.trace_targets():
        rig = Rig(targets, list(range(len(targets))), csm.grid_spec(reach, FR.RES, 2.0, 1e-10, 8, 16))
        for slot, pts in enumerate(targets):
            want = FR.free_plane(pts, side, FR.RES)
            got = rig.plane(slot)
            assert got.shape == want.shape and np.array_equal(got, want), (side, slot)


# ---------------------------------------------------------------- K21
@pytest.mark.parametrize("index", range(S.N_MAP_CASES))
def test_map_walk_over_off_steps(gpu, index):
    """rs_map_kernel with a crafted ray table of LOW or HIGH beams and one anchor: a wall on the off step's right cell (the
    walk ends there), or on the cell the uncorrected estimate names (the walk passes): signatures and the three end counters"""
    import torch
    name, grid, spec, rays, walls = S.map_cases()[index]
    want_a, want_sig, want_stats = RR.anchors_and_signatures(grid, spec, rays)
    a, sig, stats, st = device_map(torch, grid, product_spec(spec), rays)
    assert st[0] == _lib.NHIP_OK, st
    assert len(a) == 1 and np.array_equal(a, want_a)
    assert sig.tobytes() == want_sig.tobytes(), (name, np.argwhere(sig != want_sig)[:5])
    assert stats.tolist() == want_stats.tolist() and stats[3:6].sum() == 64
