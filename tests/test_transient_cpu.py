"""Transient returns without a device: hostside.transient_filter against the numpy statement of the spec
(tests/transient_reference.py) bit for bit on every case the GPU tests run too, the spec's accepted ranges at both edges of
every field, the properties of the packing, synth.add_movers, and the quality of the rule on a synthetic bag with one walker."""
import ctypes as C
import math

import numpy as np
import pytest

from nautilus_amd import _lib, csm, hostside, synth, transient
from tests import occupancy_reference as OR
from tests import transient_reference as R

CASES = R.shared_cases()


def product_spec(spec):
    return transient.spec(**{f: getattr(spec, f) for f in R.FIELDS})


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hostside_equals_reference(case):
    name, xy, off, poses, spec, hits, misses = case
    h0, m0 = hits.copy(), misses.copy()
    want = R.transient_filter(xy, off, poses, spec, hits, misses)
    R.same(hostside.transient_filter(xy, off, poses, spec, hits, misses), want, name)
    R.same(hostside.transient_filter(xy, off, poses, product_spec(spec), hits, misses), want, name + " (ctypes spec)")
    R.packing_properties(xy, off, want, name)
    assert np.array_equal(hits, h0) and np.array_equal(misses, m0)
    assert want[4][:4].sum() == len(xy) and want[4][4] == len(off) - 1


def test_threshold_edges_by_hand():
    """equality on either comparison counts as transient; one below min_through and one above on the ratio do not"""
    case, want = R.case_thresholds()
    assert R.transient_filter(*case[1:])[3].tolist() == want
    for case, want in R.case_thresholds_one_above():
        assert R.transient_filter(*case[1:])[3].tolist() == want
    name, xy, off, poses, spec, hits, misses = R.case_permille(0)
    assert R.transient_filter(xy, off, poses, spec, hits, misses)[3].tolist() == [1, 0, 0, 0, 0, 1]  # (m = 0 < min_through: static)
    name, xy, off, poses, spec, hits, misses = R.case_permille(1000)
    assert R.transient_filter(xy, off, poses, spec, hits, misses)[3].tolist() == [1, 1, 0, 0, 1, 1]


def test_neighbourhood_is_clipped_to_the_window():
    """3 x 3 window, radius 4: every cell's S is the sum of the whole plane; radius 0: its own cell"""
    name, xy, off, poses, spec, hits, misses = R.case_window_edges(4, width=3, height=3, x0=-1, y0=-1)
    labels = R.transient_filter(xy, off, poses, spec, hits, misses)[3]
    S = int(hits.sum())
    inside = [(x, y) for y in range(-2, 3) for x in range(-2, 3)]
    for k, (x, y) in enumerate(inside):
        if -1 <= x <= 1 and -1 <= y <= 1:
            m = int(misses[y + 1, x + 1])
            assert labels[k] == int(m >= 1 and 1000 * S <= 500 * (S + m)), (x, y)
        else:
            assert labels[k] == R.UNOBSERVED, (x, y)


def test_bad_offsets_are_empty_scans():
    for name, xy, off, poses, spec, hits, misses, bad, first in R.bad_offset_cases():
        want = R.transient_filter(xy, off, poses, spec, hits, misses)
        R.same(hostside.transient_filter(xy, off, poses, spec, hits, misses), want, name)
        R.packing_properties(xy, off, want, name)
        assert want[4][5] == len(bad) and want[4][4] == len(off) - 1
        for s in bad:
            assert want[1][s] == want[1][s + 1]
        covered = np.zeros(len(xy), bool)
        for s in range(len(off) - 1):
            if s not in bad:
                covered[off[s]:off[s + 1]] = True
        assert (want[3][~covered] == R.INVALID).all() and (want[3][covered] != R.INVALID).all()
        # the good scans alone give the same clouds
        good = [s for s in range(len(off) - 1) if s not in bad]
        alone = R.transient_filter(np.concatenate([xy[off[s]:off[s + 1]] for s in good]),
                                   np.concatenate([[0], np.cumsum([off[s + 1] - off[s] for s in good])]), poses[good], spec, hits, misses)
        assert alone[0].tobytes() == want[0].tobytes()


# ---------------------------------------------------------------- the spec's accepted ranges
EDGES = [("width", 1, 16384, "window"), ("height", 1, 16384, "window"), ("support_radius", 0, 4, "support_radius"),
         ("min_through", 1, 1 << 30, "min_through"), ("transient_permille", 0, 1000, "transient_permille"), ("flags", 0, 0, "flags"),
         ("reserved", 0, 0, "reserved")]


def spec_verdict(s):
    """(accepted, message) of the library's check, with or without a device: the call is made with no buffers, so an accepted
    spec ends at the missing device or at the null pointers, never at a launch"""
    lib = _lib.load()
    rc = lib.nhip_transient_filter_dev(None, None, 0, 0, None, C.byref(s), None, None, None, None, None, None, None, None)
    msg = lib.nhip_last_error().decode()
    if rc == _lib.NHIP_ERR_NODEV or (rc == _lib.NHIP_ERR_ARG and "null pointer" in msg):
        return True, msg
    assert rc == _lib.NHIP_ERR_ARG, (rc, msg)
    return False, msg


@pytest.mark.parametrize("field,lo,hi,word", EDGES, ids=[e[0] for e in EDGES])
def test_spec_edges(field, lo, hi, word):
    for v, ok in ((lo, True), (hi, True), (lo - 1, False), (hi + 1, False)):
        s = transient.spec(width=8, height=8, **{field: v}) if field not in ("width", "height") else transient.spec(**{"width": 8, "height": 8, field: v})
        accepted, msg = spec_verdict(s)
        assert accepted == ok, (field, v, msg)
        if not ok:
            assert word in msg and len(msg) > 10, (field, v, msg)
            with pytest.raises(ValueError, match=field):
                hostside.transient_spec_check(s)
        else:
            hostside.transient_spec_check(s)


def test_spec_res_and_defaults():
    d = transient.default_spec()
    assert (d.res, d.support_radius, d.min_through, d.transient_permille, d.flags, d.reserved) == (0.05, 1, 2, 500, 0, 0)
    assert (d.cell_x0, d.cell_y0, d.width, d.height) == (0, 0, 0, 0) and C.sizeof(_lib.TransientSpec) == 48
    for res, ok in ((5e-324, True), (1.7976931348623157e308, True), (0.0, False), (-0.05, False), (math.inf, False), (math.nan, False)):
        s = transient.spec(width=8, height=8, res=res)
        accepted, msg = spec_verdict(s)
        assert accepted == ok, (res, msg)
        if not ok:
            assert "res" in msg
            with pytest.raises(ValueError, match="res"):
                hostside.transient_spec_check(s)
    lib = _lib.load()
    assert lib.nhip_transient_filter_dev(None, None, -1, 0, None, C.byref(transient.spec(width=8, height=8)), *([None] * 8)) == _lib.NHIP_ERR_ARG
    assert b"n_scans" in lib.nhip_last_error()
    assert lib.nhip_transient_filter_dev(None, None, 0, -1, None, C.byref(transient.spec(width=8, height=8)), *([None] * 8)) == _lib.NHIP_ERR_ARG
    assert b"n_points" in lib.nhip_last_error()
    assert lib.nhip_transient_spec_default(None) == _lib.NHIP_ERR_ARG
    with pytest.raises(TypeError):
        transient.spec(no_such_field=1)
    o = OR.make_spec(res=0.1, cell_x0=-7, cell_y0=3, width=11, height=13)
    t = transient.spec_from(o, min_through=5)
    assert (t.res, t.cell_x0, t.cell_y0, t.width, t.height, t.min_through, t.support_radius) == (0.1, -7, 3, 11, 13, 5, 1)


# ---------------------------------------------------------------- movers and quality
def test_add_movers():
    bag = synth.SynthBag(6)
    centre = np.array([bag.truth[0, 0] + 1.0, bag.truth[0, 1] + 2.0])
    scans, masks = synth.add_movers(bag.scans, bag.truth, [(np.tile(centre, (6, 1)), 0.3), (lambda i: (1e3, 1e3), 0.5)])
    again, _ = synth.add_movers(bag.scans, bag.truth, [(lambda i: tuple(centre), 0.3)])
    for i in range(6):
        assert scans[i].dtype == np.float32 and scans[i].shape == bag.scans[i].shape and scans[i].tobytes() == again[i].tobytes()
        m = masks[i]
        assert np.array_equal(scans[i][~m], bag.scans[i][~m]) and m.sum() > 5
        c, s = math.cos(bag.truth[i, 2]), math.sin(bag.truth[i, 2])
        wx = c * scans[i][m, 0] - s * scans[i][m, 1] + bag.truth[i, 0]
        wy = s * scans[i][m, 0] + c * scans[i][m, 1] + bag.truth[i, 1]
        assert np.allclose(np.hypot(wx - centre[0], wy - centre[1]), 0.3, atol=1e-4)  # on the disc
        assert (np.hypot(*scans[i][m].T) < np.hypot(*bag.scans[i][m].T)).all()      # nearer than the wall behind
    assert all(np.array_equal(a, b) for a, b in zip(bag.scans, synth.SynthBag(6).scans))  # (the input is not modified)


def test_quality_on_synthetic_bag_with_one_walker():
    """SynthBag(120) at its truth poses, one disc of radius 0.3 m that walks 0.15 m per scan past the start of the trajectory,
    the window of every pose +- 30 m, default specs; the rule is judged on the reference alone.  Measured here: 1,767 of the
    122,687 returns come off the walker; the default rule flags 99.55 % of them and 0.26 % of the wall returns; with
    support_radius = 0 (the return's own cell only) it flags 11.0 % of the wall returns -- grazing beams that end one cell
    further along a wall pass through the wall's own cells, which is why the hit support comes from the neighbourhood."""
    bag = synth.SynthBag(120)
    i = np.arange(120)
    centres = np.stack([bag.truth[0, 0] + 0.15 * i, bag.truth[0, 1] + 2.0 + 0.02 * i], axis=1)
    scans, masks = synth.add_movers(bag.scans, bag.truth, [(centres, 0.3)])
    xy, off = csm.pack_scans(scans)
    mover = np.concatenate(masks)
    x0, y0, w, h = hostside.map_window(bag.truth, 30.0, 0.05)
    occ = OR.make_spec(cell_x0=x0, cell_y0=y0, width=w, height=h)
    grid, hits, misses, occ_stats = OR.occupancy(xy, off, bag.truth, occ)
    labels = R.transient_filter(xy, off, bag.truth, R.spec_from(occ), hits, misses)[3]
    wall_share, mover_share = (labels[~mover] == R.TRANSIENT).mean(), (labels[mover] == R.TRANSIENT).mean()
    naive = R.transient_filter(xy, off, bag.truth, R.spec_from(occ, support_radius=0), hits, misses)[3]
    naive_wall_share = (naive[~mover] == R.TRANSIENT).mean()
    print("returns %d, off the walker %d; flagged: wall %.2f %%, walker %.2f %%; support_radius 0: wall %.2f %%"
          % (len(xy), mover.sum(), 100 * wall_share, 100 * mover_share, 100 * naive_wall_share))
    assert mover.sum() > 1000
    assert wall_share <= 0.01             # a filter that eats more than one wall return in a hundred is not usable
    assert mover_share >= 0.9955 - 0.02    # the measured value minus two percentage points
    assert naive_wall_share > 0.05         # the reason for the neighbourhood
