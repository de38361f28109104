"""The HITL path without a GPU: the new entry points refuse bad arguments before they ask for a device, the spec's defaults
are the reference's, the selection inputs of tests/hitl_reference.py contain every category they claim (checked with hostside
alone), and the constant of the point-to-line normal equations' bound is measured here, from the CPU oracle (run with -s
to see the figures)."""
import ctypes as C

import numpy as np

from nautilus_amd import _lib, hitl, hostside
from oracle import oracle as O
from tests import hitl_reference as HR, resid_reference as RR


def test_spec_default_is_the_reference_configuration():
    s = hitl.default_spec()
    assert s.line_width == 0.05 and s.point_threshold == 10 and s.reserved == 0     # default_config.lua:88, 91
    assert list(s.line_a) == [0.0] * 4 and list(s.line_b) == [0.0] * 4
    assert C.sizeof(_lib.HitlSpec) == 48
    assert _lib.load().nhip_hitl_spec_default(None) == _lib.NHIP_ERR_ARG
    s = hitl.hitl_spec(HR.LINE_A, HR.LINE_B, 0.25, 3)
    assert list(s.line_a) == list(HR.LINE_A) and list(s.line_b) == list(HR.LINE_B) and s.line_width == 0.25 and s.point_threshold == 3


def test_bad_arguments_are_refused_before_a_device_is_asked_for():
    """With or without a GPU: NHIP_ERR_ARG, never NHIP_ERR_NODEV, and nothing is launched (every pointer is NULL)."""
    lib = _lib.load()
    ok = hitl.default_spec()

    def select(spec, n_scans=0):
        return lib.nhip_hitl_select_dev(None, None, n_scans, None, None if spec is None else C.byref(spec), None, None, None, None, None, None)
    for field, value in (("line_width", float("nan")), ("line_width", float("inf")), ("line_width", -0.05), ("line_width", -float("inf")),
                         ("point_threshold", 0), ("point_threshold", -3)):
        bad = hitl.default_spec()
        setattr(bad, field, value)
        assert select(bad) == _lib.NHIP_ERR_ARG, (field, value)
        assert len(lib.nhip_last_error()) > 0
    assert select(None) == _lib.NHIP_ERR_ARG
    assert select(ok, -1) == _lib.NHIP_ERR_ARG
    pack = lambda n_scans, n_blocks, n_points: lib.nhip_hitl_pack_dev(None, None, n_scans, None, None, None, None, None, n_blocks, n_points,
                                                                      None, None, None, None)
    for sizes in ((-1, 0, 0), (4, -1, 0), (4, 0, -1), (4, 5, 0)):
        assert pack(*sizes) == _lib.NHIP_ERR_ARG, sizes
    neq = lambda nb, n_poses, n_lines: lib.nhip_resid_point_to_line_normal_eq_dev(None, None, None, None, None, nb, None, n_poses, None, n_lines,
                                                                                  None, None)
    for sizes in ((-1, 1, 1), (1, -1, 1), (1, 1, -1)):
        assert neq(*sizes) == _lib.NHIP_ERR_ARG, sizes


def test_selection_inputs_contain_every_category_they_claim():
    s = HR.scans()
    main = "oblique w0.05 t10"
    assert len(s.scans) <= 64 and [len(p) for p in s.scans[:len(HR.SCAN_LENGTHS)]] == list(HR.SCAN_LENGTHS) and max(HR.SCAN_LENGTHS) > 2048
    assert all(p.dtype == np.float32 and p.ndim == 2 for p in s.scans)
    # the plan's counts are what hostside counts, point for point
    counts = []
    for k, (length, na, nb, nc) in enumerate(s.plan):
        on_a, on_b = HR.classes(main, k)
        assert (int(on_a.sum()), int(on_b.sum())) == (na + nc, nb), (k, length)
        counts.append((na + nc, nb))
    assert {9, 10, 11} <= {a for a, _ in counts} and {9, 10, 11} <= {b for _, b in counts}
    e = HR.expected(main)
    a_nodes, b_nodes = [i for i, _ in e.a_poses], [i for i, _ in e.b_poses]
    both = [k for k, (a, b) in enumerate(counts) if a >= 10 and b >= 10]
    assert both and all(k in a_nodes and len(dict(e.a_poses)[k]) == counts[k][0] for k in both), "enough on both: an a-block, a-points only"
    drop = [k for k, (a, b) in enumerate(counts) if a == 9 and b >= 10]
    assert drop and all(k in b_nodes and len(dict(e.b_poses)[k]) == counts[k][1] for k in drop), "9 on a: a b-block without the a-points"
    nine = [k for k, (a, b) in enumerate(counts) if a == 9 and b == 9]
    assert nine and not set(nine) & set(a_nodes + b_nodes), "9 on each: absent"
    assert any(nc > 0 and k in a_nodes for k, (_, _, _, nc) in enumerate(s.plan)), "points near both lines are on a"
    assert a_nodes == sorted(a_nodes) and b_nodes == sorted(b_nodes) and e.n_a >= 5 and e.n_b >= 4
    # thresholds and widths change the selection
    t1, wide = HR.expected("oblique w0.05 t1"), HR.expected("oblique w0.25 t10")
    assert 1 in [i for i, _ in t1.a_poses] and t1.n_a > e.n_a and (wide.n_a, len(wide.points)) != (e.n_a, len(e.points))
    # the width boundary, under the reference's comparison: float32(0.05) > 0.05 is rejected, one step below admitted;
    # float32(0.25) == 0.25 is admitted, one step above rejected -- and a Python-float width decides the first otherwise
    on5, b5 = HR.classes("flat + zero-length b w0.05 t1", s.boundary)
    on25, _ = HR.classes("flat + zero-length b w0.25 t10", s.boundary)
    assert on5[:6].tolist() == [False, True, False, False, False, False] and on25[:6].tolist() == [True, True, True, True, True, False]
    pts = s.scans[s.boundary]
    assert hostside.distance_to_line_segment_f32(pts[:1], np.float32(HR.FLAT))[0] == HR.W5
    assert (hostside.distance_to_line_segment_f32(pts[:1], np.float32(HR.FLAT)) <= 0.05)[0], "numpy no longer compares a Python float in float32"
    # non-finite points: on no line; the zero-length line b selects its cluster
    bad = ~np.isfinite(pts).all(axis=1)
    assert bad.sum() == 6 and not on5[bad].any() and not b5[bad].any() and not on25[bad].any() and b5.sum() == 12
    flat = HR.expected("flat + zero-length b w0.05 t1")
    assert s.boundary in [i for i, _ in flat.a_poses]
    # axis-aligned segments at heading exactly 0: among points whose projection lies inside the segment, closer to the line
    # than the width, both outcomes of IsBetween(projection, end, end)
    assert s.poses[s.quirk][2] == 0.0 and s.poses[s.boundary][2] == 0.0
    h, _ = HR.classes("horizontal then vertical w0.25 t10", s.quirk)
    v, _ = HR.classes("vertical then horizontal w0.05 t10", s.quirk)
    assert 20 <= h[:300].sum() <= 280 and 5 <= v[300:].sum() <= 295, (h[:300].sum(), v[300:].sum())
    assert HR.expected("horizontal then vertical w0.25 t10").n_a >= 1 and HR.expected("vertical then horizontal w0.05 t10").n_a >= 1
    none = HR.expected("nothing selected")
    assert none.n_a == none.n_b == 0 and len(none.points) == 0 and none.block_offsets.tolist() == [0]
    # an oblique segment, a horizontal and a vertical one, a zero-length line b
    shapes = [c[0] for c in HR.CONFIGS.values()]
    assert any(l[0] != l[2] and l[1] != l[3] for l in shapes) and any(l[1] == l[3] for l in shapes) and any(l[0] == l[2] for l in shapes)
    assert any(c[1][:2] == c[1][2:] for c in HR.CONFIGS.values())
    assert {c[2] for c in HR.CONFIGS.values()} == {0.05, 0.25} and {c[3] for c in HR.CONFIGS.values()} == {1, 10}


def test_pose_floats_are_the_ones_hostside_forms():
    s = HR.scans()
    got = hitl.pose_floats(s.poses)
    want = np.array([[np.float32(np.cos(p[2])), np.float32(np.sin(p[2])), np.float32(p[0]), np.float32(p[1])] for p in s.poses], np.float32)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32))


def test_constant_of_the_normal_equations_bound_is_measured_from_the_oracle():
    """K_P2L_NE (tests/hitl_reference.py): the oracle's Jet rows summed in double in row order against the 28 sums of the
    longdouble reference rows, over RR.segments(); what is left of the ratio once the n of the summation is taken out, and the
    ratio of the same rows summed without summation error."""
    excess, rows_only = -np.inf, 0.0
    for c in RR.segments():
        r, n = c.ref, len(c.pts)
        wr, w0, w1 = O.point_to_line_block(c.seg, c.pts, c.pose, c.line)
        ne, m_ne = HR.ne_of_rows(r.res, r.jp, r.jl), HR.ne_of_rows(r.m_res, r.m_jp, r.m_jl)
        q_double, q_ld = RR.ratio(HR.ne_of_rows_in_order(wr, w0, w1), ne, m_ne), RR.ratio(HR.ne_of_rows(wr, w0, w1), ne, m_ne)
        print("%-8s n %4d   double sums: ratio %.3g, ratio - n %.3g   longdouble sums: ratio %.3g" % (c.tag, n, q_double, q_double - n, q_ld))
        assert q_double <= HR.K_P2L_NE + n
        excess, rows_only = max(excess, q_double - n), max(rows_only, q_ld)
    figure = max(excess, rows_only)
    print("point-to-line normal equations: ratio - n %.3g, rows alone %.3g -> K rule %d, K %d" % (excess, rows_only, RR.k_rule(figure), HR.K_P2L_NE))
    assert RR.k_rule(figure) <= HR.K_P2L_NE
    # the blocks the GPU test adds: their references exist, the empty one is zero
    b = HR.ne_blocks()
    assert b.sizes[b.n_cases:].tolist() == list(HR.NE_SIZES) and HR.NE_SIZES[-3:] == (HR.TRIP, HR.TRIP + 1, 2 * HR.TRIP)
    z = b.n_cases + HR.NE_SIZES.index(0)
    assert not b.ne[z].any() and not b.m_ne[z].any() and np.isfinite(b.ne[b.n_cases:]).all()
