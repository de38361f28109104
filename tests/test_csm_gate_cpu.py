"""CPU checks of the score gate's floor (nhip_csm_gate_floor, include/nautilus_hip.h).

The floor is where a gated branch-and-bound search starts its best: it must never be above a sum the caller could keep,
or a record would be lost.  Kept means: the quantised score plus half a step (the most the exact score can lie above it)
reaches min_score.  The floor must not be loose either: within 2N + 1 of the smallest such sum."""
import ctypes as C
import math

import numpy as np
import pytest

from nautilus_amd import _lib, csm

N_POINTS = (1, 7, 1081, 32768)


def _floor(spec, min_score, n):
    out = C.c_int32(-7)
    _lib.check(_lib.load().nhip_csm_gate_floor(C.byref(spec), float(min_score), int(n), C.byref(out)))
    return out.value


@pytest.mark.parametrize("cell_bits", [16, 8])
def test_floor_is_conservative_and_tight(cell_bits):
    lib = _lib.load()
    spec = csm.grid_spec(cell_bits=cell_bits)
    Lf = math.log(1e-10)
    levels = 65535 if cell_bits == 16 else 255
    step = -Lf / levels
    thresholds = [Lf, Lf + 0.3 * step, Lf + step, Lf + 1.7 * step, -20.0, -8.0, -5.0, -5.0 + 1e-9, -1.234567, -step, 0.0]
    thresholds += list(np.random.default_rng(3).uniform(Lf, 0.0, 12))
    for n in N_POINTS:
        for m in thresholds:
            f = _floor(spec, m, n)
            assert 0 <= f <= levels * n + n, (n, m, f)
            # the smallest sum a caller could keep: quantised score + half a step >= min_score (searched by brute force
            # around the boundary the formula predicts)
            guess = int(math.ceil(n * ((m - Lf) / step - 0.5)))
            lo, hi = max(0, guess - 2 * n - 4), guess + 2 * n + 4
            kept = [s for s in range(lo, hi + 1) if lib.nhip_score_from_sum(C.byref(spec), s, n) + step / 2 >= m]
            s_min = kept[0] if kept else hi
            assert s_min > lo or lo == 0, "search window too narrow"
            assert f <= s_min, (cell_bits, n, m, f, s_min)
            # every sum below the floor is rejected, near the floor
            for s in range(max(0, f - 3), f):
                assert lib.nhip_score_from_sum(C.byref(spec), s, n) + step / 2 < m, (n, m, s, f)
            assert s_min - f <= 2 * n + 1, (cell_bits, n, m, f, s_min)


def test_floor_arguments():
    lib = _lib.load()
    spec = csm.grid_spec(cell_bits=16)
    out = C.c_int32(-7)
    assert lib.nhip_csm_gate_floor(C.byref(spec), float("nan"), 1081, C.byref(out)) == _lib.NHIP_ERR_ARG
    assert out.value == -7, "nothing is written on an error"
    assert lib.nhip_csm_gate_floor(C.byref(spec), -5.0, -1, C.byref(out)) == _lib.NHIP_ERR_ARG
    for n in N_POINTS + (0,):
        assert _floor(spec, -math.inf, n) == 0
        assert _floor(spec, math.log(1e-10), n) == 0  # (nothing is below the floor score)
    assert _floor(spec, -5.0, 0) == 0  # an empty scan: its record (the floor score) is gated by its score
    # a threshold above every score: the floor is above every sum a scan can reach
    assert _floor(spec, 1.0, 32768) > 65535 * 32768
    assert _floor(spec, -5.0, 1081) == int(math.floor(1081 * ((-5.0 - math.log(1e-10)) / (-math.log(1e-10) / 65535) - 1)))


def test_python_helpers():
    spec = csm.grid_spec(cell_bits=8)
    assert csm.gate_floor(spec, -5.0, 1081) == _floor(spec, -5.0, 1081) > 0
    recs = np.zeros(3, dtype=csm.MATCH_DTYPE)
    recs[1] = (-1, -1, -1, -np.inf)
    assert list(csm.rejected(recs)) == [False, True, False]
