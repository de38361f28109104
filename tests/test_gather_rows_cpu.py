"""The inputs of tests/test_gather_rows_gpu.py hold what they claim (tests/gather_rows.py), by numpy alone: the scans' run lists
are the listed run lengths, `early` forces the reduction before its second pass, the global table is not staged in LDS, and
the order in which the gather keeps rows in flight adds every row once."""
import os

import numpy as np

from tests import gather_rows as M
from tests import lattice_edge as L
from tests import rotation_round_trips as RT
from tests import saturated_cases as S

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nautilus_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_constants_are_the_sources():
    bounds = _src("nhip_bnb_bounds.h")
    assert "constexpr uint32_t LANE_WEIGHT = %du;" % M.LANE_WEIGHT in bounds
    assert "if (y + 1 < NB) load_row(y + 1, n0, n1, n2, n3);" in bounds  # (one row ahead, both forms of the pool)
    assert M.NXY == RT.NXY and M.RUN_MAX == 64 and M.ENTRIES == 64


def test_rows_ahead_add_every_row_once():
    """The register rotation of the gather, restated: row y + 1 (the shipped form) or rows y + 1 and y + 2 (measured in round
    19, not shipped) in flight while row y is added."""
    NB = 11
    for ahead in (1, 2):
        held, added, loads = {}, [], []
        for y in range(ahead):
            held[y] = "row%d" % y
            loads.append(y)
        for y in range(NB):
            w = held.pop(y)
            if y + ahead < NB:
                held[y + ahead] = "row%d" % (y + ahead)
                loads.append(y + ahead)
            assert len(held) <= ahead
            added.append(w)
        assert added == ["row%d" % y for y in range(NB)] and loads == list(range(NB)) and not held


def test_lds_scans_have_the_listed_runs():
    lo, hi = S.plateau_square()
    h = M.NXY // 2
    for name, pts in M.lds_scans():
        runs = M.run_lengths(M.lds_entries(pts))
        if name == "early":
            assert runs == [64] + [1] * 63 + [64] and len(pts) == 191
            assert M.reductions_before_pass(runs) == [False, True]   # entry 64 is lane 0's second: 64 + 64 > LANE_WEIGHT
            assert len(set(M.lds_entries(pts))) == 65
        else:
            n = int(name[3:])
            assert len(pts) == n and runs == [64] * (n // 64) + ([n % 64] if n % 64 else []), name
            assert not any(M.reductions_before_pass(runs))
        # every lookup of every pose at the top level of `plateau` (a cell of margin for the other rotations)
        for p in pts:
            row, col = L.lookup_origin(p, 0, 1, h, h)
            assert lo + 1 <= row and row + M.NXY <= hi - 1 and lo + 1 <= col and col + M.NXY <= hi - 1, (name, row, col)
    assert [n for n, _ in M.lds_scans()] == ["run%d" % n for n in M.RUNS] + ["early"] and M.RUNS == (0, 1, 63, 64, 65, 128, 129)


def test_global_scans_and_table():
    words = RT.pooled_words(RT.GLOBAL_SIDE, RT.pad_of(RT.MAX_SHIFT))
    assert not RT.pool_in_lds(words) and RT.pool_in_lds(RT.pooled_words(RT.GLOBAL_SIDE - 8, RT.pad_of(RT.MAX_SHIFT)))
    tgt = np.zeros((400, 2), np.float32) + np.float32(1.5)
    scans = dict(M.global_scans(tgt))
    assert [len(scans["run%d" % n]) for n in M.RUNS] == list(M.RUNS) and len(scans["early"]) == 191
    res = RT.res_of(RT.GLOBAL_SIDE)
    assert 0.2 > 8 * res  # (the line's points lie in 63 different pooled entries)
    assert L.spec_of and RT.N_THETA == 9
