"""Global localisation without a GPU: hostside.global_localize on the CPU oracle's matcher, on the mapped lap of the synthetic
world -- the measurement the GPU test's bounds come from -- and the bookkeeping of the (scan, proposal) entries."""
import json
import os
import subprocess
import sys

import numpy as np

from nautilus_amd import _lib, csm, hostside, rangesig
from tests import relocalize_cases as cases


def test_global_localize_on_the_cpu_oracle():
    """The 23 odd scans 1, 19, ..., 397 of SynthBag(400) in the map of its even scans (tests/relocalize_cases.py), NO priors, the
    defaults of the spec with NHIP_RANGESIG_UNKNOWN_STOPS, config #2's table and lattice, the CPU oracle's matcher: 115 (scan,
    proposal) entries.  Measured here: every query has five proposals, the truth is within 1 m and 15 degrees of one of them
    for all 23 (no query is left out, here or in the GPU test), the winning ranks are 0 .. 4, and the winning poses lie within
    0.0598 m and 0.2799 degrees of the truth -- the figures tests/relocalize_cases.py keeps for the GPU test.  Conditions: three
    cells and one step of the lattice, as for localize with priors (tests/test_localize_cpu.py)."""
    from oracle.cpu_backend import OracleBackend
    bag, grid, occ = cases.mapped_lap()
    q = cases.QUERIES
    qxy, qoff = csm.pack_scans([bag.scans[i] for i in q])
    spec = rangesig.spec(occ, flags=_lib.NHIP_RANGESIG_UNKNOWN_STOPS)
    r = hostside.global_localize(OracleBackend(), qxy, qoff, grid, occ, spec=spec)
    assert r["poses"].shape == (len(q), 3) and r["proposals"].shape == (len(q), 5, 3) and r["records"].shape == (len(q), 5)
    assert (r["candidates"][:, :, 0] >= 0).all() and r["stats"][6] == 0 and r["stats"][7] == 5 * len(q)
    assert cases.near_truth(r["proposals"], bag.truth[q]).any(axis=1).all()
    pos, ang = cases.errors(r["poses"], bag.truth[q])
    print("ranks %s; position error max %.4f m, heading error max %.4f deg" % (r["rank"].tolist(), pos.max(), ang.max()))
    assert (r["rank"] >= 0).all() and pos.max() <= 0.15 and ang.max() <= 1.0
    assert pos.max() <= cases.ORACLE_POSITION_ERROR_M and ang.max() <= cases.ORACLE_HEADING_ERROR_DEG
    # the winner is the entry with the highest score, ties to the lower rank; the default spec of the call sets the flag
    score = r["records"]["score"]
    assert np.array_equal(r["rank"], score.argmax(axis=1))


def test_entries_ranks_and_queries_without_a_record():
    """the second half alone, on a matcher that is a table: unfilled records make no entry, a rejected entry cannot win, ties go
    to the lower rank, a query none of whose entries matched has no pose"""
    spec = rangesig.spec(width=40, height=40, cell_x0=-5, cell_y0=7)
    anchors = np.array([[5, 5, 0, 0], [15, 5, 1, 0], [25, 35, 2, 3]], np.int32)
    cand = np.full((4, 3, 4), -1, np.int32)
    cand[0, :3] = [[0, 0, 10, 64], [1, 5, 11, 64], [2, 63, 12, 64]]
    cand[1, :2] = [[2, 1, 3, 30], [0, 2, 4, 30]]
    cand[3, :1] = [[1, 0, 0, 9]]
    xy = np.arange(2 * 10, dtype=np.float32).reshape(10, 2)
    off = np.array([0, 1, 3, 6, 10], np.int32)
    seen = {}

    def table(xy2, off2, priors, grid, occ_spec, **kw):
        seen.update(xy=xy2, off=off2, priors=priors, kw=kw)
        rec = np.zeros(len(priors), csm.MATCH_DTYPE)
        rec["itheta"], rec["score"] = [3, 4, 5, -1, 6, -1], [-2.0, -1.0, -1.0, 0.0, -3.0, 0.0]  # (entry 3 and 5: rejected)
        poses = np.arange(3 * len(priors), dtype=np.float64).reshape(-1, 3)
        poses[rec["itheta"] < 0] = np.nan
        return {"records": rec, "poses": poses}
    r = hostside.global_localize_finish(table, xy, off, cand, anchors, spec, np.zeros(8, np.int64), None, spec, dict(cell_bits=16))
    assert seen["off"].tolist() == [0, 1, 2, 3, 5, 7, 11] and np.array_equal(seen["xy"][3:5], xy[1:3]) and seen["kw"] == dict(cell_bits=16)
    assert np.array_equal(seen["priors"], r["proposals"][cand[:, :, 0] >= 0])
    assert seen["priors"][0].tolist() == [(-5 + 5 + 0.5) * 0.05, (7 + 5 + 0.5) * 0.05, 0.0]
    assert r["rank"].tolist() == [1, 1, -1, -1]  # query 0: entries 1 and 2 tie, the lower rank; query 1: entry 3 is rejected
    assert r["poses"][0].tolist() == [3.0, 4.0, 5.0] and r["poses"][1].tolist() == [12.0, 13.0, 14.0] and np.isnan(r["poses"][2:]).all()
    assert r["records"]["itheta"].tolist() == [[3, 4, 5], [-1, 6, -1], [-1, -1, -1], [-1, -1, -1]]


def test_example_without_priors_on_the_oracle(tmp_path):
    """examples/localize.py --no-prior --backend oracle on a small bag, through the map files: errors of the order of the run
    with priors (tests/test_localize_cpu.py holds that one to 0.15 m and 1 degree), the winning ranks in the JSON line"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    stem = str(tmp_path / "map")
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "localize.py"), "--backend", "oracle", "--scans", "24", "--map-scans",
                          "16", "--map-poses", "truth", "--map", stem, "--no-prior"], capture_output=True, text=True, cwd=root, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["no_prior"] is True and res["queries"] == 8 and res["rejected"] == 0 and len(res["ranks"]) == 8
    assert all(0 <= k < 5 for k in res["ranks"])
    assert res["position_error_max_m"] <= 0.15 and res["heading_error_max_deg"] <= 1.0
