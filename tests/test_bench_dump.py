"""bench.py --dump-outputs: the last timed step's records as .npy files a second build's run can be compared with, value
for value (float32 / float64 only, at most 64 MB in all, a fixed seeded sample of the pairs above that); --steps sets the
number of timed steps and must be at least one."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from nautilus_amd.csm import MATCH_DTYPE  # noqa: E402


def _table(n, seed=4):
    rng = np.random.default_rng(seed)
    rec = np.zeros(n, dtype=MATCH_DTYPE)
    rec["itheta"], rec["ix"], rec["iy"] = rng.integers(0, 61, n), rng.integers(0, 81, n), rng.integers(0, 81, n)
    rec["score"] = rng.uniform(-23.0, 0.0, n).astype(np.float32)
    return rec, rec.view(np.int32).reshape(-1, 4)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_writes_every_record_in_float(tmp_path):
    rec, table = _table(1000)
    bench.dump_outputs(str(tmp_path / "out"), table)
    got = _load(tmp_path / "out")
    assert set(got) == {"best_pose_index", "score", "pair_index"}
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert np.array_equal(got["best_pose_index"], np.stack([rec["itheta"], rec["ix"], rec["iy"]], 1).astype(np.float64))
    assert np.array_equal(got["score"], rec["score"]) and got["score"].dtype == np.float32
    assert np.array_equal(got["pair_index"], np.arange(1000))


def test_dump_samples_the_same_pairs_under_the_size_cap(tmp_path):
    rec, table = _table(5000)
    cap = 40000
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), table, max_bytes=cap)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= cap
    idx = a["pair_index"].astype(np.int64)
    assert 0 < len(idx) < 5000 and np.all(np.diff(idx) > 0)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["score"], rec["score"][idx])
    assert np.array_equal(a["best_pose_index"][:, 1], rec["ix"][idx])


def test_steps_and_dump_flags_parse():
    a = bench.parse(["--steps", "7", "--warmup", "2", "--dump-outputs", "d"])
    assert a.steps == 7 and a.warmup == 2 and a.dump_outputs == "d"
    assert bench.parse([]).dump_outputs is None
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])
