"""The scan matcher on saturated tables and at the largest admitted sums (tests/saturated_cases.py states the inputs and the
closed forms, tests/test_saturated_cases_cpu.py shows that they hold what they claim).

Every matcher kernel adds 8-bit cell values in packed 16-bit fields, each with a hand-derived limit that is tight only when
every cell read is 255 -- which tables built from range scans never offer.  Here they do: clusters of coincident points on a
plateau of top-level cells, at the lengths either side of every limit (64, 256 | 257 | 258, 320, 1088 | 1089, 2048 | 2049,
4096 | 4097) in all four alignment classes, with the unique maximum placed in the first and in the last packed field of a
plane, and the longest scans whose sums an int32 holds (32,768 points at 16 bits, 8,421,504 at 8 bits) -- one point more is
refused.  Records, sums and whole score volumes against the oracle AND against closed forms that use neither the oracle nor a
kernel (n coincident points sum to n times one cell), in every form of the branch-and-bound matcher (the hooks and form ids
of tests/test_bnb_level2_runs_gpu.py, the general instantiation NHIP_BNB_QUEUE=1), the kernels that perform every add
(strips with and without skip map, dense; the kernel whose lanes are poses) and the default plan; the instrumented build
counts the rotation passes that took the run list | the field check; the score gate at the top score; the exact-score pass
where every row window is all ones.

Every form matches 87 sources x 4 targets = 348 pairs on lattice L and 350 on S (the corner sources once more about their own
search centre), per cell width; the forms with a form id take them in lists of at most 128 pairs, below the 192 from which on
the matcher chooses the split form by itself.  Three sources exist because a one-line change of a limit passed without them:
stagger194 (SWAR_START_MAX + 3), lanes258 (LANE_WEIGHT + 1); co258 and co4096 catch cache_origins' 258 and SEG_CHUNKS 36."""
import ctypes as C
import math
import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from nautilus_amd import _lib, csm
from oracle import oracle as O
from tests import exact_score_cases as E
from tests import level2_runs as M
from tests import saturated_cases as S
from tests import test_bnb_level2_runs_gpu as RUNS

pytestmark = pytest.mark.gpu

EVERY_ADD = {"NHIP_CSM_EXHAUSTIVE": "1"}
# id -> (environment, form id nhip_csm_last_launch reports | None: not the branch-and-bound matcher)
PLANS = {"default": ({}, None), "queue": ({"NHIP_BNB_QUEUE": "1"}, 0)}
for _i, (_env, _form) in enumerate(RUNS.FORMS):
    PLANS["bnb%d" % _i] = (_env, _form)
    PLANS["bnb%d-per-cell" % _i] = (dict(_env, **RUNS.OFF), _form)
for _small in ({}, {"NHIP_CSM_SMALL": "0"}):
    for _dense in ({}, {"NHIP_CSM_DENSE": "1"}):
        PLANS["-".join(["every-add"] + ["strips"] * bool(_small) + ["dense"] * bool(_dense))] = (dict(EVERY_ADD, **_small, **_dense), None)
assert len(PLANS) == 14


def _threaded(fn, jobs):
    with ThreadPoolExecutor(8) as pool:  # (the oracle's calls release the interpreter lock)
        return list(pool.map(fn, jobs))


class _World:
    """The sources and the four targets of one cell width on the device, the tables (16 bits: with a skip map too), the oracle's."""

    def __init__(self, bits):
        self.bits, self.levels = bits, S.levels(bits)
        self.src = dict(S.sources())
        if bits == 16:
            self.src["long16"] = S.long_source(16)
        self.names = list(self.src)
        self.scan_of = {n: i for i, n in enumerate(self.names)}
        self.slot_of = {t: i for i, t in enumerate(S.TARGETS)}
        self.target_pts = [S.target(t, bits) for t in S.TARGETS]
        self.st = csm.ScanTable.from_list([self.src[n].points for n in self.names] + self.target_pts)
        self.ids = np.arange(len(self.names), len(self.names) + len(S.TARGETS), dtype=np.int32)
        self.spec = csm.grid_spec(S.RANGE, S.RES, S.SIGMA, S.FLOOR_P, S.MAX_SHIFT, bits)
        self.ospec = O.grid_spec(S.RANGE, S.RES, S.SIGMA, S.FLOOR_P, bits)
        self.grids = csm.LikelihoodGrids(self.st, self.ids, self.spec)
        self.tables = [self.grids]
        if bits == 16:  # (8-bit grids always carry a skip map; 16-bit ones only when asked: both strip variants)
            self.with_map = csm.LikelihoodGrids(self.st, self.ids, csm.grid_spec(S.RANGE, S.RES, S.SIGMA, S.FLOOR_P, S.MAX_SHIFT, 16, skip_map=True))
            self.tables.append(self.with_map)
        assert self.grids.layout.pad == S.PAD and self.grids.layout.side == S.SIDE
        self.images = O.grid_build_batch(self.st.xy, self.st.offsets, self.ids, self.ospec)
        for g in self.tables:
            for slot in range(len(S.TARGETS)):
                assert np.array_equal(g.interior(slot), self.images[slot]), "a table differs from the oracle's"
        self._want = {}

    def close(self):
        for g in self.tables:
            g.close()
        self.st.close()

    def arrays(self, pairs):
        src = np.array([self.scan_of[s] for s, _, _ in pairs], np.int32)
        slot = np.array([self.slot_of[t] for _, t, _ in pairs], np.int32)
        org = np.array([o for _, _, o in pairs], np.int32).reshape(-1, 2)
        return src, slot, np.zeros(len(pairs)), org

    def match(self, pairs, lattice, env=(), grids=None, min_score=None, **flags):
        src, slot, th0, org = self.arrays(pairs)
        os.environ.update(env)
        try:
            got, sums = csm.match_pairs(self.st, grids or self.grids, src, slot, th0, csm.search_spec(*S.LATTICES[lattice], **flags),
                                        pair_origin=org, min_score=min_score)
            launch = csm.last_launch()
        finally:
            for k in env:
                os.environ.pop(k, None)
        return got, sums, launch

    def oracle(self, pairs, lattice):
        key = (lattice, tuple(pairs))
        if key not in self._want:
            src, slot, th0, org = self.arrays(pairs)
            self._want[key] = O.csm_match_batch(self.st.xy, self.st.offsets, self.images, self.ospec, src, slot, th0,
                                                O.search_spec(*S.LATTICES[lattice]), pair_origin=org)
            self._want[key].setflags(write=False)
        return self._want[key]


@pytest.fixture(scope="module")
def world8(gpu):
    w = _World(8)
    yield w
    w.close()


@pytest.fixture(scope="module")
def world16(gpu):
    w = _World(16)
    yield w
    w.close()


@pytest.fixture(params=[8, 16], ids=["8bit", "16bit"])
def world(request):
    return request.getfixturevalue("world%d" % request.param)


def _check_records(w, pairs, lattice, got, sums, what):
    """Records and sums: the oracle's, and the closed forms where there is one."""
    want = w.oracle(pairs, lattice)
    n = np.array([w.src[s].n for s, _, _ in pairs])
    for f in ("itheta", "ix", "iy"):
        assert np.array_equal(got[f], want[f]), (what, f, [(p, g, v) for p, g, v in zip(pairs, got[f], want[f]) if g != v][:5])
    assert np.array_equal(sums, want["sum"]), (what, [(p, g, v) for p, g, v in zip(pairs, sums, want["sum"]) if g != v][:5])
    assert np.array_equal(got["score"], want["score"].astype(np.float32)), what
    assert np.array_equal(got["score"], np.array([S.score_of(s, k, w.bits) for s, k in zip(sums, n)], np.float32)), what
    Lf = math.log(S.FLOOR_P)
    n_closed = 0
    for i, (s, t, org) in enumerate(pairs):
        rec = (int(got["itheta"][i]), int(got["ix"][i]), int(got["iy"][i]))
        if t == "plateau":  # every pose ties at n * levels: the tie-break's choice
            assert rec == (0, 0, 0) and int(sums[i]) == w.src[s].n * w.levels > 0, (what, s, rec, sums[i])
            # (three rounded double operations of magnitude |Lf|, and one for margin)
            assert abs(float(got["score"][i])) <= 4 * 2.0 ** -53 * abs(Lf), (what, s, got["score"][i])
            n_closed += 1
        if s in S.CORNER_POSE and (t, org) == S.corner_pose(s, lattice)[:2]:  # the one top-level translation
            assert rec == S.corner_pose(s, lattice)[2] and int(sums[i]) == w.src[s].n * w.levels, (what, s, rec, sums[i])
            n_closed += 1
    return n_closed


@pytest.mark.parametrize("plan", sorted(PLANS))
@pytest.mark.parametrize("lattice", ["L", "S"])
def test_records_every_source_target_and_form(world, lattice, plan):
    w = world
    env, form = PLANS[plan]
    n_pairs = 0
    for group, names in S.groups().items():
        pairs = S.pairs(names, lattice)
        for g in (w.tables if "NHIP_CSM_EXHAUSTIVE" in env else w.tables[:1]):
            # (the hooks' form ids are those of lists below the matcher's 192 pairs, from which on it shares pairs among
            #  workgroups by itself: such plans take a list in parts; the default plan takes it whole)
            part = len(pairs) if form is None else 128
            parts = [w.match(pairs[i:i + part], lattice, env, g) for i in range(0, len(pairs), part)]
            got, sums = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
            what = (w.bits, lattice, plan, group, g is not w.grids)
            assert _check_records(w, pairs, lattice, got, sums, what) >= len(names)
            for i, (_, _, launch) in enumerate(parts):
                if form is None:
                    break
                assert launch["form_id"] == form and launch["n_pairs"] == len(pairs[i * part:(i + 1) * part]), (what, launch)
                assert launch["l2_runs"] == ("NHIP_BNB_L2_RUNS" not in env) and not launch["instrumented"], (what, launch)
                assert launch["short_scans"] == (group == "short" and plan != "queue"), (what, launch)
        n_pairs += len(pairs)
    assert n_pairs == len(S.sources()) * len(S.TARGETS) + 2 * (lattice == "S")
    print("%d-bit, lattice %s, plan %s: %d pairs" % (w.bits, lattice, plan, n_pairs))


@pytest.mark.parametrize("cls", range(4))
def test_score_volumes_are_the_closed_forms(world, cls):
    """csm.score_volume of every single-cluster source of one alignment class, with the skip map, dense and (16 bits) without a
    map: every entry is n times the cell of the table as the device holds it, and the oracle's."""
    w = world
    srcs = [w.src["co%d@%d" % (n, cls)] for n in S.COUNTS]
    osearch = O.search_spec(*S.LATTICES["L"])
    oracle_half = _threaded(lambda s: O.csm_scores(s.points, w.images[w.slot_of["half"]], w.ospec, 0.0, osearch), srcs)
    variants = [(g, dense) for g in w.tables for dense in (False, True)]
    for g, dense in variants:
        search = csm.search_spec(*S.LATTICES["L"], dense=dense)
        for t in ("half", "plateau", "corner"):
            image = g.interior(w.slot_of[t])
            for i, s in enumerate(srcs):
                vol = csm.score_volume(w.st, g, w.scan_of[s.name], w.slot_of[t], 0.0, search)
                assert np.array_equal(vol, S.closed_volume(image, s.n, s.cell, "L")), (w.bits, s.name, t, dense, g is not w.grids)
                if t == "half":
                    assert np.array_equal(vol, oracle_half[i]), (w.bits, s.name, dense)
                if t == "plateau":
                    assert vol.shape == (7, 25, 25) and np.all(vol == s.n * w.levels), (w.bits, s.name, dense)
    assert len(variants) == (4 if w.bits == 16 else 2)


def _passes(w, pair, env):
    """Rotation passes by strip path of one instrumented launch of one pair on lattice L."""
    csm.bnb_stats_levels()  # (reset)
    got, sums, launch = w.match([pair], "L", dict(env, **RUNS.INSTR))
    assert launch["instrumented"]
    lv = csm.bnb_stats_levels()
    return got, sums, {k: int(lv[v]) for k, v in RUNS.KIND.items()}


@pytest.mark.parametrize("n", [257, 258])
def test_group_limit_takes_the_stated_path(world, n):
    """257 points in one group of 8 lanes fill its fields to 65,535 and stay on the merged lists; 258 fall back on the field
    check.  The counters of the instrumented build say which list the rotation passes took -- summed over the targets: a case
    that only ever ran the fall-back would prove nothing."""
    w = world
    for cls in range(4):
        s = w.src["co%d@%d" % (n, cls)]
        what = {M.status(row, col) for row, col in S.rotations(s.points, "L")}
        assert what == {"runs" if n == 257 else "field"}
        what = what.pop()
        for env in (RUNS.SPLIT_ONE, RUNS.HAND_OVER):
            total = dict.fromkeys(RUNS.KIND, 0)
            for t in S.TARGETS:
                pair = (s.name, t, (0, 0))
                got, sums, counts = _passes(w, pair, env)
                _check_records(w, [pair], "L", got, sums, (w.bits, s.name, t, "instrumented"))
                for k, v in counts.items():
                    total[k] += v
                _, _, off = _passes(w, pair, dict(env, **RUNS.OFF))
                assert not any(off.values()), (s.name, t, off)
            print(w.bits, s.name, what, sorted(env)[-1], total)
            assert total[what] >= 1, (s.name, env, total, "no rotation pass reached the kernels that keep the lists")
            assert all(v == 0 for k, v in total.items() if k != what), (s.name, env, total)


def _floor_value(spec, n, want, near, half_unit):
    """The smallest min_score whose gate floor on n points is `want`: bisection between near -+ half_unit (half a unit of the
    sum either side of the boundary) down to two neighbouring floats.  None if the floor steps over `want`."""
    lo, hi = near - half_unit, near + half_unit
    assert csm.gate_floor(spec, lo, n) < want <= csm.gate_floor(spec, hi, n)
    while np.nextafter(lo, math.inf) < hi:
        mid = 0.5 * (lo + hi)
        if csm.gate_floor(spec, mid, n) < want:
            lo = mid
        else:
            hi = mid
    return float(hi) if csm.gate_floor(spec, hi, n) == want else None


def test_gate_at_the_top_score(world):
    _gate_at_the_top_score(world, "co1088@0")


def test_gate_at_the_top_score_longest_scan(world16):
    _gate_at_the_top_score(world16, "long16")


def _gate_at_the_top_score(w, name):
    """The gate keeps a record whose score is >= min_score and prunes below floor(n ((min_score - Lf) / step - 1)).  On the
    plateau the top score is the largest a scan can have.  At min_score = that score the record is the ungated one, bit for bit;
    one float above it is rejected.  The floors n * levels and n * levels + 1 -- the largest the arithmetic can be asked for,
    2,147,450,880 at 32,768 points -- both have floats that give them: they need min_score >= step, far above every score
    (the top score is 0 but for rounding), so both reject (a floor equal to the top sum never keeps a record: the floor lies one step BELOW the threshold by design)."""
    s = w.src[name]
    pair = [(name, "plateau", (0, 0))]
    top = s.n * w.levels
    Lf = math.log(S.FLOOR_P)
    step = -Lf / w.levels
    for env in ({}, EVERY_ADD):
        plain, plain_sums, _ = w.match(pair, "L", env)
        assert int(plain_sums[0]) == top
        edge = float(plain["score"][0])  # the record's float, exactly representable as a double
        kept, kept_sums, _ = w.match(pair, "L", env, min_score=edge)
        assert kept.tobytes() == plain.tobytes() and np.array_equal(kept_sums, plain_sums), env
        assert csm.gate_floor(w.spec, edge, s.n) <= top - s.n
        above = float(np.nextafter(edge, math.inf))
        gone, gone_sums, _ = w.match(pair, "L", env, min_score=above)
        assert csm.rejected(gone)[0] and gone_sums[0] == -1 and gone["score"][0] == -math.inf, env
        for want in (top, top + 1):
            v = _floor_value(w.spec, s.n, want, Lf + step * (want / s.n + 1.0), 0.5 * step / s.n)
            assert v is not None, "no float gives the floor %d" % want
            assert v > 0.5 * step > abs(edge)
            gone, gone_sums, _ = w.match(pair, "L", env, min_score=float(v))
            assert csm.rejected(gone)[0] and gone_sums[0] == -1, (env, want)


def test_exact_score_where_every_row_window_is_all_ones(world):
    w = world
    s = w.src["co1088@0"]
    pair = [(s.name, "plateau", (0, 0))]
    got, sums, _ = w.match(pair, "L", exact_score=True)
    assert (int(got["itheta"][0]), int(got["ix"][0]), int(got["iy"][0])) == (0, 0, 0) and int(sums[0]) == s.n * w.levels
    ref = O.pose_score_exact(s.points, w.target_pts[w.slot_of["plateau"]], O.grid_spec(S.RANGE, S.RES, S.SIGMA, S.FLOOR_P, 16), 0.0,
                             O.search_spec(*S.LATTICES["L"]), 0, 0, 0)
    assert ref == 0.0  # V = K^2 at every lookup: log 1
    lo, hi = E.interval(ref, s.n)
    assert lo <= got["score"][0] <= hi, (got["score"][0], lo, hi)


# ---- the longest admitted scans -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("lattice", ["L", "S"])
def test_longest_16_bit_scan_every_form(world16, lattice):
    w = world16
    pairs = S.pairs(["long16"], lattice)[:len(S.TARGETS)]
    top = S.max_pts(16) * 65535
    assert top == 2147450880 < 2 ** 31
    for plan, (env, form) in sorted(PLANS.items()):
        for g in (w.tables if "NHIP_CSM_EXHAUSTIVE" in env else w.tables[:1]):
            t0 = time.perf_counter()
            got, sums, launch = w.match(pairs, lattice, env, g)
            print("long16 lattice %s plan %s%s: %.3f s" % (lattice, plan, " (skip map)" if g is not w.grids else "", time.perf_counter() - t0))
            assert _check_records(w, pairs, lattice, got, sums, (lattice, plan)) == 1
            assert sums.dtype == np.int32 and sums[w.slot_of["plateau"]] == top and np.all(sums >= 0)
            if form is not None:
                assert launch["form_id"] == form and not launch["short_scans"], (plan, launch)


def _refused(st, grids, search):
    """nhip_csm_match on pair (scan 0, slot 0) with sentinel-filled outputs: (return code, message, outputs untouched)."""
    out = np.zeros(1, dtype=csm.MATCH_DTYPE)
    out[:] = (7, 7, 7, 7.0)
    sums = np.full(1, 7, np.int32)
    zero, th0 = np.zeros(1, np.int32), np.zeros(1)
    rc = _lib.load().nhip_csm_match(st._h, grids._h, _lib.ptr(zero), _lib.ptr(zero), _lib.ptr(th0), None, 1, C.byref(search),
                                    _lib.ptr(out), _lib.ptr(sums))
    msg = _lib.load().nhip_last_error().decode("utf-8", "replace")
    return rc, msg, bool(np.all(out["itheta"] == 7) and np.all(out["score"] == 7.0) and np.all(sums == 7))


def test_one_point_more_is_refused(world):
    w = world
    n = S.max_pts(w.bits) + 1
    long_pts = S.cluster((S.CENTRE, S.CENTRE), n)
    st = csm.ScanTable.from_list([long_pts, w.target_pts[0]])
    grids = csm.LikelihoodGrids(st, np.array([1], np.int32), w.spec)
    try:
        for lattice in ("T", "S"):
            for flags in ({}, {"exhaustive": True}):
                rc, msg, untouched = _refused(st, grids, csm.search_spec(*S.LATTICES[lattice], **flags))
                assert rc == _lib.NHIP_ERR_ARG and "int32 sums" in msg and str(n) in msg and untouched, (rc, msg)
    finally:
        grids.close()
        st.close()
    # the drop-in call refuses such a pc_a the same way
    matcher = csm.CorrelativeScanMatcher(S.RANGE, 0.6, 0.3, S.RES, S.SIGMA, w.bits)
    with pytest.raises(_lib.NhipError, match="int32 sums") as err:
        matcher.GetTransformation(long_pts, w.target_pts[0], 0.0, 0.0, math.radians(2.0))
    assert err.value.code == _lib.NHIP_ERR_ARG and str(n) in str(err.value)
    if w.bits == 16:
        assert n == 32769


LONG8_PLANS = ["default", "every-add", "every-add-strips"]


def test_longest_8_bit_scan(world8):
    """8,421,504 coincident points on the 1 x 3 x 3 lattice: sums up to 2,147,483,520."""
    w = world8
    s = S.long_source(8)
    top = s.n * 255
    assert top == 2147483520 < 2 ** 31
    st = csm.ScanTable.from_list([s.points] + w.target_pts)
    ids = np.arange(1, 1 + len(S.TARGETS), dtype=np.int32)
    grids = csm.LikelihoodGrids(st, ids, w.spec)
    try:
        src, slot, th0 = np.zeros(len(S.TARGETS), np.int32), np.arange(len(S.TARGETS), dtype=np.int32), np.zeros(len(S.TARGETS))
        want = O.csm_match_batch(st.xy, st.offsets, w.images, w.ospec, src, slot, th0, O.search_spec(*S.LATTICES["T"]))
        closed = [S.first_maximum(S.closed_volume(w.images[k], s.n, s.cell, "T")) for k in range(len(S.TARGETS))]
        assert closed[w.slot_of["plateau"]] == ((0, 0, 0), top)
        for plan in LONG8_PLANS:
            env = PLANS[plan][0]
            os.environ.update(env)
            try:
                t0 = time.perf_counter()
                got, sums = csm.match_pairs(st, grids, src, slot, th0, csm.search_spec(*S.LATTICES["T"]))
                print("long8 plan %s: %.3f s for %d pairs" % (plan, time.perf_counter() - t0, len(src)))
            finally:
                for k in env:
                    os.environ.pop(k, None)
            for f in ("itheta", "ix", "iy"):
                assert np.array_equal(got[f], want[f]), (plan, f, got[f], want[f])
            assert np.array_equal(sums, want["sum"]) and sums.dtype == np.int32 and np.all(sums >= 0), (plan, sums, want["sum"])
            assert [((int(r["itheta"]), int(r["ix"]), int(r["iy"])), int(v)) for r, v in zip(got, sums)] == closed, plan
            assert np.array_equal(got["score"], want["score"].astype(np.float32)), plan
            assert np.array_equal(got["score"], S.score_of(sums, s.n, 8)), plan
    finally:
        grids.close()
        st.close()
