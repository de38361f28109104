"""ctypes binding of libnautilus_hip.so (include/nautilus_hip.h).

The library is the product: there is no Python or CPU fallback.  If the shared object is
missing this module raises at import of the symbol table; if no GPU is visible every
compute entry point returns NHIP_ERR_NODEV and `check()` raises NhipError.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# NHIP_LIB lets kernel A/B experiments point at another build of the same library
LIB_PATH = os.environ.get("NHIP_LIB") or os.path.join(_HERE, "lib", "libnautilus_hip.so")

NHIP_OK, NHIP_ERR_ARG, NHIP_ERR_NODEV, NHIP_ERR_HIP, NHIP_ERR_ALLOC, NHIP_ERR_STATE = 0, -1, -2, -3, -4, -5
NHIP_LIDAR_NORMAL, NHIP_LIDAR_POINT = 0, 1
NHIP_SEARCH_EXHAUSTIVE, NHIP_SEARCH_DENSE, NHIP_SEARCH_SHORT_SCANS, NHIP_SEARCH_EXACT_SCORE, NHIP_SEARCH_LATENCY = 1, 2, 4, 8, 16
NHIP_SHORT_SCAN_POINTS = 1088
NHIP_FEATURE_MAX = 64
NHIP_NORMALS_MAX_BINS, NHIP_NORMALS_MAX_SAMPLES = 64, 128
NHIP_GRID_SKIP_MAP, NHIP_GRID_NO_IMAGE = 1, 2
NHIP_TIMER_CSM, NHIP_TIMER_GRID, NHIP_TIMER_RESID, NHIP_TIMER_CORR, NHIP_TIMER_NORMEQ, NHIP_TIMER_GRID_CLEAR = 0, 1, 2, 3, 4, 5
NHIP_TIMER_CSM_BOUNDS, NHIP_TIMER_CSM_CAND, NHIP_TIMER_EXACT_SCORE = 6, 7, 8
NHIP_TIMER_VEC_RASTER, NHIP_TIMER_VEC_VOTES, NHIP_TIMER_VEC_ROUNDS = 9, 10, 11
NHIP_TIMER_OCC_TRACE, NHIP_TIMER_OCC_CLASSIFY = 12, 13
NHIP_OCC_ACCUMULATE = 1
NHIP_PLACE_PAST_ONLY = 1
NHIP_PLACE_WORKSPACE_MAX = 64 << 20
NHIP_RANGESIG_WORKSPACE_MAX = 64 << 20
NHIP_RANGESIG_UNKNOWN_STOPS = 1
NHIP_CONSISTENCY_STATE_BYTES = 8448
NHIP_LOSS_NONE, NHIP_LOSS_HUBER, NHIP_LOSS_SOFT_L1, NHIP_LOSS_CAUCHY = 0, 1, 2, 3
NHIP_RELPOSE_BAD_INFO, NHIP_RELPOSE_BAD_MEASUREMENT, NHIP_RELPOSE_SAME_POSE = 1, 2, 4


class NhipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("nautilus_hip error %d: %s" % (code, msg))
        self.code = code


class GridSpec(C.Structure):
    _fields_ = [("range", C.c_double), ("res", C.c_double), ("sigma", C.c_double),
                ("floor_p", C.c_double), ("max_shift", C.c_int32), ("cell_bits", C.c_int32),
                ("flags", C.c_int32), ("reserved", C.c_int32)]


class GridLayout(C.Structure):
    _fields_ = [("side", C.c_int32), ("pad", C.c_int32), ("pitch", C.c_int32), ("rows", C.c_int32),
                ("blur_radius", C.c_int32), ("cell_bytes", C.c_int32), ("tap_sum", C.c_int64),
                ("grid_bytes", C.c_int64), ("score_floor", C.c_double), ("score_step", C.c_double),
                ("skip_bytes", C.c_int64), ("slot_bytes", C.c_int64), ("pool_bytes", C.c_int64),
                ("pool_pitch", C.c_int32), ("pool_rows", C.c_int32), ("pool4_bytes", C.c_int64),
                ("pool4_pitch", C.c_int32), ("pool4_rows", C.c_int32), ("hi_bytes", C.c_int64),
                ("hi_pitch", C.c_int32), ("hits_pitch", C.c_int32), ("hits_bytes", C.c_int64)]


class Search(C.Structure):
    _fields_ = [("n_theta", C.c_int32), ("nx", C.c_int32), ("ny", C.c_int32), ("flags", C.c_int32),
                ("theta_step", C.c_double)]


class CsmParams(C.Structure):
    _fields_ = [("scanner_range", C.c_double), ("trans_range", C.c_double), ("low_res", C.c_double),
                ("high_res", C.c_double), ("sigma", C.c_double), ("floor_p", C.c_double), ("cell_bits", C.c_int32),
                ("reserved", C.c_int32)]


class FeatureSpec(C.Structure):
    _fields_ = [("threshold", C.c_double), ("distance_threshold", C.c_double), ("max_neighbor_distance", C.c_double),
                ("neighbors_per_side", C.c_int32), ("min_neighbors", C.c_int32), ("max_planar", C.c_int32),
                ("max_edge", C.c_int32)]


class NormalsSpec(C.Structure):
    _fields_ = [("neighborhood_size", C.c_double), ("neighborhood_step_size", C.c_double), ("mean_distance", C.c_double),
                ("bin_number", C.c_int32), ("max_growth_steps", C.c_int32), ("seed", C.c_uint32), ("flags", C.c_int32)]


class VectorizeSpec(C.Structure):
    _fields_ = [("res", C.c_double), ("band", C.c_double), ("cell_x0", C.c_int32), ("cell_y0", C.c_int32),
                ("width", C.c_int32), ("height", C.c_int32), ("min_hits", C.c_int32), ("n_theta", C.c_int32),
                ("min_votes", C.c_int32), ("max_gap", C.c_int32), ("min_length", C.c_int32), ("max_segments", C.c_int32),
                ("flags", C.c_int32), ("reserved", C.c_int32)]


class VectorizeLayout(C.Structure):
    _fields_ = [("counts_offset", C.c_int64), ("cells_offset", C.c_int64), ("votes_offset", C.c_int64),
                ("live_offset", C.c_int64), ("bytes", C.c_int64), ("n_rho", C.c_int32), ("n_along", C.c_int32)]


class OccupancySpec(C.Structure):
    _fields_ = [("res", C.c_double), ("cell_x0", C.c_int32), ("cell_y0", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("max_ray_cells", C.c_int32), ("min_obs", C.c_int32), ("occ_permille", C.c_int32), ("free_permille", C.c_int32),
                ("flags", C.c_int32), ("reserved", C.c_int32)]


class TransientSpec(C.Structure):
    _fields_ = [("res", C.c_double), ("cell_x0", C.c_int32), ("cell_y0", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("support_radius", C.c_int32), ("min_through", C.c_int32), ("transient_permille", C.c_int32), ("flags", C.c_int32),
                ("reserved", C.c_int32)]


class MapwinSpec(C.Structure):
    _fields_ = [("res", C.c_double), ("cell_x0", C.c_int32), ("cell_y0", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("side", C.c_int32), ("occ_min", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32)]


class RangesigSpec(C.Structure):
    _fields_ = [("res", C.c_double), ("unit", C.c_double), ("cell_x0", C.c_int32), ("cell_y0", C.c_int32), ("width", C.c_int32),
                ("height", C.c_int32), ("occ_min", C.c_int32), ("free_max", C.c_int32), ("stride", C.c_int32),
                ("max_ray_cells", C.c_int32), ("rays_per_sector", C.c_int32), ("top_k", C.c_int32), ("min_sep", C.c_int32),
                ("min_sectors", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32)]


class FreespaceSpec(C.Structure):
    _fields_ = [("hit_radius", C.c_int32), ("end_margin", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32)]


NHIP_REFINE_THRESHOLDS, NHIP_REFINE_TARGET_MAX, NHIP_REFINE_TRACE_DOUBLES = 16, 2048, 64
NHIP_REFINE_SKIPPED, NHIP_REFINE_TARGET_TOO_LONG, NHIP_REFINE_FEW, NHIP_REFINE_SINGULAR = 1, 2, 4, 8
NHIP_REFINE_RUNAWAY, NHIP_REFINE_NOT_CONVERGED = 16, 32


class RefineSpec(C.Structure):
    _fields_ = [("thr0", C.c_double), ("shrink", C.c_double), ("thr_min", C.c_double), ("step_tol_m", C.c_double),
                ("step_tol_rad", C.c_double), ("min_spread", C.c_double), ("max_shift_m", C.c_double),
                ("max_turn_sin", C.c_double), ("thr", C.c_float * 16), ("max_iterations", C.c_int32), ("min_corr", C.c_int32),
                ("flags", C.c_int32), ("reserved", C.c_int32)]


class Refined(C.Structure):
    _fields_ = [("c", C.c_double), ("s", C.c_double), ("tx", C.c_double), ("ty", C.c_double), ("info", C.c_double * 6),
                ("cost", C.c_double), ("n_corr", C.c_int32), ("iterations", C.c_int32), ("flags", C.c_uint32),
                ("pad", C.c_uint32)]


class PlaceSpec(C.Structure):
    _fields_ = [("n_rings", C.c_int32), ("range_max", C.c_float), ("top_k", C.c_int32), ("min_separation", C.c_int32),
                ("max_permille", C.c_int32), ("flags", C.c_int32)]


class PlaceSeqSpec(C.Structure):
    _fields_ = [("half_window", C.c_int32), ("step", C.c_int32)]


class ConsistencySpec(C.Structure):
    _fields_ = [("t0", C.c_double), ("t_rate", C.c_double), ("t_max", C.c_double), ("r0", C.c_double), ("r_rate", C.c_double),
                ("r_max", C.c_double), ("max_steps", C.c_int32), ("flags", C.c_int32)]


class LossSpec(C.Structure):
    _fields_ = [("kind", C.c_int32), ("flags", C.c_int32), ("scale", C.c_double)]


class HitlSpec(C.Structure):
    _fields_ = [("line_a", C.c_float * 4), ("line_b", C.c_float * 4), ("line_width", C.c_double),
                ("point_threshold", C.c_int32), ("reserved", C.c_int32)]


class PcgStats(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("flag", C.c_int32), ("relative_residual", C.c_double)]


class Match(C.Structure):
    _fields_ = [("itheta", C.c_int32), ("ix", C.c_int32), ("iy", C.c_int32), ("score", C.c_float)]


_vp, _i32, _i64, _f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double
_P = C.POINTER

# name -> (restype, argtypes); the list is also what tests check against the header.
PROTOTYPES = {
    "nhip_init": (C.c_int, [_P(C.c_int)]),
    "nhip_set_device": (C.c_int, [C.c_int]),
    "nhip_last_error": (C.c_char_p, []),
    "nhip_version": (C.c_char_p, []),
    "nhip_grid_layout": (C.c_int, [_P(GridSpec), _P(GridLayout)]),
    "nhip_grids_bytes": (_i64, [_P(GridSpec), _i64]),
    "nhip_grid_workspace_bytes": (_i64, [_P(GridSpec), _i32]),
    "nhip_grid_tables": (C.c_int, [_P(GridSpec), _vp, _vp]),
    "nhip_csm_rot0": (C.c_int, [_vp, _vp, _i32, _vp]),
    "nhip_csm_delta_table": (C.c_int, [_P(Search), _vp]),
    "nhip_match_to_transform": (C.c_int, [_P(Match), _P(GridSpec), _P(Search), _f64, _i32, _i32,
                                          _P(C.c_float), _P(C.c_float), _P(C.c_float)]),
    "nhip_score_from_sum": (_f64, [_P(GridSpec), _i64, _i32]),
    "nhip_csm_gate_floor": (C.c_int, [_P(GridSpec), _f64, _i32, _P(_i32)]),
    "nhip_dev_status": (C.c_int, [_vp, _P(_i32)]),
    "nhip_host_phases": (C.c_int, [_P(_f64)]),
    "nhip_device_pool_configure": (C.c_int, [_i64]),
    "nhip_device_pool_release": (C.c_int, []),
    "nhip_device_pool_stats": (C.c_int, [_P(_i64), _P(_i64)]),
    "nhip_grid_build_dev": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _P(GridSpec), _vp, _vp, _i64, _vp]),
    "nhip_grid_rebuild_dev": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _P(GridSpec), _vp, _vp, _i64, _vp]),
    "nhip_csm_match_dev": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _P(GridSpec), _vp, _vp, _vp, _vp, _vp, _i32,
                                     _P(Search), _vp, _vp, _vp, _vp, _i64, _vp]),
    "nhip_csm_match_gated_dev": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _P(GridSpec), _vp, _vp, _vp, _vp, _vp, _i32,
                                           _P(Search), _vp, _vp, _vp, _vp, _i64, _vp, _f64]),
    "nhip_submap_member_affines": (C.c_int, [_vp, _i32, _vp, _vp, _i32, _vp]),
    "nhip_submaps_gather_dev": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _i64, _vp, _vp]),
    "nhip_grids_build_submaps": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _P(GridSpec), _P(_vp)]),
    "nhip_csm_workspace_bytes": (_i64, [_i32]),
    "nhip_csm_last_launch": (C.c_int, [_P(_i32)]),
    "nhip_csm_get_transformation_info": (C.c_int, [_vp]),
    "nhip_bnb_stats": (C.c_int, [_P(C.c_uint64), _P(C.c_uint64)]),
    "nhip_bnb_stats_per_pair": (C.c_int, [_vp, _i32]),
    "nhip_bnb_timeline": (C.c_int, [_vp, _i32]),
    "nhip_bnb_timeline_candidates": (C.c_int, [_vp, _i32]),
    "nhip_bnb_stats_levels": (C.c_int, [_P(C.c_uint64)]),
    "nhip_bnb_stats_chunks": (C.c_int, [_P(C.c_uint64)]),
    "nhip_bnb_stats_seeds": (C.c_int, [_P(C.c_uint64)]),
    "nhip_csm_scores_dev": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _P(GridSpec), _i32, _i32, _vp, _vp, _i32, _i32,
                                      _P(Search), _vp, _vp]),
    "nhip_resid_lidar_dev": (C.c_int, [C.c_int, _vp, _vp, _i64, _vp, _vp, _i32, _vp, _i32, _vp,
                                       _vp, _vp, _vp, _vp]),
    "nhip_resid_lidar_normal_eq_dev": (C.c_int, [C.c_int, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp]),
    "nhip_pose_affines": (C.c_int, [_vp, _i32, _vp]),
    "nhip_corr_search_dev": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _vp, _i32, _vp, C.c_float, _vp, _vp, _vp, _vp]),
    "nhip_corr_search_normals_dev": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _vp, _i32, _vp, C.c_float, C.c_float, _vp, _vp, _vp,
                                               _vp]),
    "nhip_corr_compact_dev": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    "nhip_resid_point_to_line_dev": (C.c_int, [_vp, _vp, _vp, _i64, _vp, _vp, _i32, _vp, _i32, _vp, _i32,
                                               _vp, _vp, _vp, _vp]),
    "nhip_resid_point_to_line_normal_eq_dev": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _vp]),
    "nhip_resid_odometry_dev": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _f64, _f64, _vp, _i32, _vp, _vp,
                                          _vp, _vp]),
    "nhip_resid_odometry_normal_eq_dev": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _f64, _f64, _vp, _i32, _vp, _vp]),
    "nhip_resid_odometry_robust_normal_eq_dev": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _f64, _f64, _P(LossSpec), _vp, _i32, _vp, _vp,
                                                           _vp]),
    "nhip_resid_relpose_dev": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "nhip_resid_relpose_normal_eq_dev": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _P(LossSpec), _vp, _i32, _vp, _vp, _vp, _vp]),
    "nhip_resid_relpose": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "nhip_loss_log1p_pinned": (C.c_int, [_vp, _i64, _vp]),
    "nhip_relpose_information": (C.c_int, [_vp, _i32, _f64, _f64, _f64, _vp, _vp]),
    "nhip_bsr_assemble_dev": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "nhip_bsr_pcg_workspace_bytes": (_i64, [_i32, _i32]),
    "nhip_bsr_pcg_dev": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _f64, _f64, _f64, _i32, _i32, _vp, _vp, _i64,
                                   _P(PcgStats), _vp]),
    "nhip_bsr_pcg_columns_workspace_bytes": (_i64, [_i32, _i32, _i32]),
    "nhip_bsr_pcg_columns_dev": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _i32, _f64, _f64, _i32, _i32, _vp, _vp, _i64,
                                           _P(PcgStats), _vp]),
    "nhip_scans_upload": (C.c_int, [_vp, _vp, _i32, _P(_vp)]),
    "nhip_scans_free": (C.c_int, [_vp]),
    "nhip_grids_build": (C.c_int, [_vp, _vp, _i32, _P(GridSpec), _P(_vp)]),
    "nhip_grids_free": (C.c_int, [_vp]),
    "nhip_grids_was_rebuilt": (C.c_int, [_vp]),
    "nhip_grids_download": (C.c_int, [_vp, _i32, _vp]),
    "nhip_grids_download_skip_map": (C.c_int, [_vp, _i32, _vp]),
    "nhip_grids_download_hi_plane": (C.c_int, [_vp, _i32, _vp]),
    "nhip_grids_download_hi_plane_copy": (C.c_int, [_vp, _i32, _i32, _vp]),
    "nhip_grids_download_tiled16": (C.c_int, [_vp, _i32, _vp]),
    "nhip_grids_download_pool": (C.c_int, [_vp, _i32, _vp]),
    "nhip_grids_download_pool4": (C.c_int, [_vp, _i32, _vp]),
    "nhip_grids_download_hits": (C.c_int, [_vp, _i32, _vp]),
    "nhip_csm_match": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _P(Search), _vp, _vp]),
    "nhip_csm_match_gated": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _P(Search), _vp, _vp, _f64]),
    "nhip_csm_scores": (C.c_int, [_vp, _vp, _i32, _i32, _f64, _i32, _i32, _P(Search), _vp]),
    "nhip_lc_scatter_scores_dev": (C.c_int, [_vp, _vp, _i32, _vp, _vp]),
    "nhip_lc_pair_gate_dev": (C.c_int, [_vp, _i32, _vp, _i32, _f64, _i32, _vp, _vp]),
    "nhip_lc_chi_square_gate_dev": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _i32, _f64, _vp, _vp, _vp]),
    "nhip_feature_spec_default": (C.c_int, [_P(FeatureSpec)]),
    "nhip_features_extract_dev": (C.c_int, [_vp, _vp, _i32, _P(FeatureSpec), _vp, _vp, _vp, _vp, _vp, _vp]),
    "nhip_features_pack_dev": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    "nhip_normals_spec_default": (C.c_int, [_P(NormalsSpec)]),
    "nhip_normals_estimate_dev": (C.c_int, [_vp, _vp, _i32, _P(NormalsSpec), _vp, _vp, _vp]),
    "nhip_normals_estimate": (C.c_int, [_vp, _P(NormalsSpec), _vp, _vp]),
    "nhip_vectorize_spec_default": (C.c_int, [_P(VectorizeSpec)]),
    "nhip_vectorize_tables": (C.c_int, [_P(VectorizeSpec), _vp, _vp]),
    "nhip_map_pose_affines": (C.c_int, [_vp, _i32, _vp]),
    "nhip_vectorize_workspace_bytes": (_i64, [_P(VectorizeSpec), _i32]),
    "nhip_vectorize_workspace_layout": (C.c_int, [_P(VectorizeSpec), _i32, _P(VectorizeLayout)]),
    "nhip_vectorize_dev": (C.c_int, [_vp, _vp, _vp, _i32, _P(VectorizeSpec), _i32, _i32, _i32, _vp, _vp, _vp, _i64, _vp]),
    "nhip_vectorize": (C.c_int, [_vp, _vp, _P(VectorizeSpec), _i32, _i32, _i32, _vp, _vp]),
    "nhip_vectorize_endpoints": (C.c_int, [_P(VectorizeSpec), _vp, _i32, _vp]),
    "nhip_occupancy_spec_default": (C.c_int, [_P(OccupancySpec)]),
    "nhip_occupancy_dev": (C.c_int, [_vp, _vp, _vp, _i32, _P(OccupancySpec), _vp, _vp, _vp, _vp, _vp]),
    "nhip_occupancy": (C.c_int, [_vp, _vp, _P(OccupancySpec), _vp, _vp, _vp, _vp]),
    "nhip_transient_spec_default": (C.c_int, [_P(TransientSpec)]),
    "nhip_transient_filter_dev": (C.c_int, [_vp, _vp, _i32, _i32, _vp, _P(TransientSpec), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "nhip_transient_filter": (C.c_int, [_vp, _vp, _P(TransientSpec), _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "nhip_mapwin_spec_default": (C.c_int, [_P(MapwinSpec)]),
    "nhip_mapwin_origins": (C.c_int, [_vp, _i32, _f64, _vp, _vp]),
    "nhip_mapwin_workspace_bytes": (_i64, [_i32]),
    "nhip_mapwin_cells_dev": (C.c_int, [_vp, _P(MapwinSpec), _i32, _vp, _vp, _vp, _vp]),
    "nhip_mapwin_gather_dev": (C.c_int, [_vp, _vp, _P(MapwinSpec), _vp, _i32, _vp, _i64, _vp, _vp, _vp, _i64, _vp]),
    "nhip_map_windows": (C.c_int, [_vp, _P(MapwinSpec), _vp, _i32, _vp, _i64, _vp, _vp]),
    "nhip_rangesig_spec_default": (C.c_int, [_P(RangesigSpec)]),
    "nhip_rangesig_tables": (C.c_int, [_P(RangesigSpec), _vp, _vp]),
    "nhip_rangesig_workspace_bytes": (_i64, [_P(RangesigSpec), _i32, _i32]),
    "nhip_rangesig_anchors_dev": (C.c_int, [_vp, _P(RangesigSpec), _i32, _vp, _vp, _vp, _i64, _vp]),
    "nhip_rangesig_map_dev": (C.c_int, [_vp, _P(RangesigSpec), _vp, _vp, _i32, _vp, _vp, _vp]),
    "nhip_rangesig_scans_dev": (C.c_int, [_vp, _vp, _i32, _P(RangesigSpec), _vp, _vp]),
    "nhip_rangesig_match_dev": (C.c_int, [_vp, _i32, _vp, _vp, _i32, _P(RangesigSpec), _vp, _vp, _vp, _i64, _vp]),
    "nhip_rangesig_candidates": (C.c_int, [_vp, _P(RangesigSpec), _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "nhip_freespace_spec_default": (C.c_int, [_P(FreespaceSpec)]),
    "nhip_freespace_planes_bytes": (_i64, [_P(GridSpec), _i64]),
    "nhip_freespace_trace_dev": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _P(GridSpec), _vp, _vp, _vp]),
    "nhip_freespace_check_dev": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _P(GridSpec), _vp, _vp, _vp, _vp, _vp, _i32, _P(Search),
                                           _vp, _vp, _P(FreespaceSpec), _vp, _vp]),
    "nhip_csm_freespace": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _P(Search), _vp, _P(FreespaceSpec), _vp]),
    "nhip_refine_spec_default": (C.c_int, [_P(RefineSpec)]),
    "nhip_refine_start_poses": (C.c_int, [_vp, _vp, _vp, _i32, _P(GridSpec), _P(Search), _vp]),
    "nhip_refine_icp_dev": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _vp, _vp, _i32, _P(RefineSpec), _vp, _vp, _vp]),
    "nhip_refine_icp": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _vp, _vp, _i32, _P(RefineSpec), _vp, _vp]),
    "nhip_refined_to_transform": (C.c_int, [_P(Refined), _P(_f64), _P(_f64), _P(_f64)]),
    "nhip_place_spec_default": (C.c_int, [_P(PlaceSpec)]),
    "nhip_place_tables": (C.c_int, [_P(PlaceSpec), _vp, _vp]),
    "nhip_place_workspace_bytes": (_i64, [_P(PlaceSpec), _i32]),
    "nhip_place_describe_dev": (C.c_int, [_vp, _vp, _i32, _P(PlaceSpec), _vp, _vp, _vp]),
    "nhip_place_match_dev": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _P(PlaceSpec), _vp, _vp, _vp, _i64, _vp]),
    "nhip_place_candidates": (C.c_int, [_vp, _vp, _i32, _P(PlaceSpec), _vp, _vp, _vp, _vp]),
    "nhip_place_seq_spec_default": (C.c_int, [_P(PlaceSeqSpec)]),
    "nhip_place_seq_workspace_bytes": (_i64, [_P(PlaceSpec), _P(PlaceSeqSpec), _i32, _i32]),
    "nhip_place_seq_match_dev": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _P(PlaceSpec), _P(PlaceSeqSpec), _vp, _vp, _vp, _i64, _vp]),
    "nhip_place_seq_candidates": (C.c_int, [_vp, _vp, _i32, _P(PlaceSpec), _P(PlaceSeqSpec), _vp, _vp]),
    "nhip_consistency_spec_default": (C.c_int, [_P(ConsistencySpec)]),
    "nhip_consistency_workspace_bytes": (_i64, [_i32]),
    "nhip_consistency_adjacency_dev": (C.c_int, [_vp, _i32, _P(ConsistencySpec), _vp, _vp, _vp, _vp]),
    "nhip_consistency_set_dev": (C.c_int, [_vp, _vp, _i32, _P(ConsistencySpec), _i32, _vp, _vp, _vp, _vp, _i64, _vp]),
    "nhip_consistency": (C.c_int, [_vp, _i32, _P(ConsistencySpec), _vp, _vp, _vp]),
    "nhip_hitl_spec_default": (C.c_int, [_P(HitlSpec)]),
    "nhip_hitl_select_dev": (C.c_int, [_vp, _vp, _i32, _vp, _P(HitlSpec), _vp, _vp, _vp, _vp, _vp, _vp]),
    "nhip_hitl_pack_dev": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp]),
    "nhip_features_extract": (C.c_int, [_vp, _P(FeatureSpec), _vp, _vp, _vp, _vp, _vp]),
    "nhip_lc_chi_square_gate": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _i32, _f64, _vp, _vp]),
    "nhip_lc_scatter_scores": (C.c_int, [_vp, _vp]),
    "nhip_lc_pair_gate": (C.c_int, [_vp, _i32, _vp, _i32, _f64, _i32, _vp]),
    "nhip_csm_cache_configure": (C.c_int, [_i64]),
    "nhip_csm_cache_clear": (C.c_int, []),
    "nhip_csm_cache_stats": (C.c_int, [_P(_i64), _P(_i64), _P(_i64), _P(_i64)]),
    "nhip_csm_get_transformation": (C.c_int, [_P(CsmParams), _vp, _i32, _vp, _i32, _f64, _f64, _f64, _P(_f64),
                                              _P(C.c_float), _P(C.c_float), _P(C.c_float)]),
    "nhip_resid_batch_create": (C.c_int, [C.c_int, _vp, _vp, _vp, _vp, _i32, _i32, _P(_vp)]),
    "nhip_resid_batch_eval": (C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "nhip_resid_batch_eval_compact": (C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "nhip_resid_batch_eval_q": (C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "nhip_resid_jacobians_from_q": (C.c_int, [C.c_int, _vp, _vp, _vp, _i64, _vp, _vp]),
    "nhip_resid_batch_eval_block": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "nhip_resid_batch_free": (C.c_int, [_vp]),
    "nhip_host_alloc": (C.c_int, [C.c_size_t, _P(_vp)]),
    "nhip_host_free": (C.c_int, [_vp]),
    "nhip_resid_odometry": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _f64, _f64, _vp, _i32, _vp, _vp, _vp]),
    "nhip_resid_point_to_line": (C.c_int, [_vp, _vp, _vp, _i64, _vp, _vp, _i32, _vp, _i32, _vp, _i32,
                                           _vp, _vp, _vp]),
    "nhip_allgather_matches": (C.c_int, [_vp, _vp, _i32, _vp, _vp]),
    "nhip_round_norm_dev": (C.c_int, [_vp, _vp, _i64, _i32, _vp, _vp]),
    "nhip_timing_enable": (C.c_int, [C.c_int]),
    "nhip_timing_reset": (C.c_int, []),
    "nhip_timing_get": (C.c_int, [C.c_int, _P(_f64), _P(_i32)]),
}

_lib = None


def load():
    """Load the shared library (once) and bind every prototype.  Fails loudly."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "nautilus_amd: %s is missing -- build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` or `make -C nautilus_amd/csrc`; there is no CPU fallback" % LIB_PATH)
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so.7 (same SONAME as
    # /opt/rocm's).  If ours were resolved first, torch would later bind to the system runtime
    # and see no GPUs.  Importing torch first makes both share torch's copy; without torch
    # (a C++ host) the library binds to /opt/rocm as linked.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc):
    if rc != NHIP_OK:
        raise NhipError(rc, load().nhip_last_error().decode("utf-8", "replace"))


def device_count():
    n = C.c_int(0)
    load().nhip_init(C.byref(n))
    return n.value


def ptr(a):
    """void* of a numpy array (None -> NULL)."""
    return None if a is None else a.ctypes.data_as(C.c_void_p)
