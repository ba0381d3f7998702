"""ctypes mirror of include/isdf_accel.h (the C-ABI drop-in boundary).

Host-side plumbing only: structure layouts, enum values and the loader of libisdf_accel.so.
The library is the product; there is NO CPU fallback — if the shared object is missing, loading fails loudly.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libisdf_accel.so")

# enums (keep in sync with include/isdf_accel.h)
ISDF_OK = 0
ISDF_ERR_INVALID_ARG, ISDF_ERR_NO_DEVICE, ISDF_ERR_HIP, ISDF_ERR_STATE, ISDF_ERR_OVERFLOW, ISDF_ERR_UNSUPPORTED = -1, -2, -3, -4, -5, -6
V1_SWEPT, V2_OCC_TILE, V3_ESDF_TILE = 1, 2, 3
GRID_OCCUPANCY, GRID_ESDF = 0, 1
U8, F32, F64 = 0, 1, 2
(SHAPE_TORUS, SHAPE_CAPPEDTORUS, SHAPE_CAPPEDCONE, SHAPE_ROUNDEDCONE, SHAPE_WIREFRAMEBOX, SHAPE_BENDLINEAR,
 SHAPE_TWISTBOX, SHAPE_BENDBOX, SHAPE_TABLE, SHAPE_TREFOIL, SHAPE_SMOOTHDIFFERENCE, SHAPE_SMOOTHINTERSECTION,
 SHAPE_CSG, SHAPE_BOX, SHAPE_BALL, SHAPE_MESH) = range(16)
GRAD_DEFAULT, GRAD_CENTRAL, GRAD_BOX_FORWARD, GRAD_ANALYTIC_BALL = 0, 1, 2, 3

SHAPE_NAMES = ["Torus", "Cappedtorus", "CappedCone", "RoundedCone", "WireframeBox", "BendLinear", "TwistBox",
               "BendBox", "Table", "Trefoil", "SmoothDifference", "SmoothIntersection", "CSG", "Box", "Ball", "Mesh"]


class IsdfShape(C.Structure):
    _fields_ = [("kind", C.c_int32), ("grad_mode", C.c_int32), ("params", C.c_double * 16),
                ("trans", C.c_double * 3), ("rotate", C.c_double * 9), ("bound_radius", C.c_double),
                ("bbox_center", C.c_double * 3), ("bbox_half", C.c_double * 3),
                ("mesh_vertices", C.POINTER(C.c_double)), ("mesh_faces", C.POINTER(C.c_int32)),
                ("n_vertices", C.c_int32), ("n_faces", C.c_int32)]


class IsdfConfig(C.Structure):
    _fields_ = [("device", C.c_int32), ("variant", C.c_int32), ("kernel_size", C.c_int32),
                ("integral_intervs", C.c_int32), ("enable_dyn", C.c_int32), ("enable_pos", C.c_int32),
                ("enable_cull", C.c_int32), ("reserved0", C.c_int32),
                ("safety_hor", C.c_double), ("weight_p", C.c_double), ("weight_v", C.c_double),
                ("weight_omg", C.c_double), ("weight_theta", C.c_double), ("vmax", C.c_double),
                ("omgmax", C.c_double), ("thetamax", C.c_double), ("smoothing_eps", C.c_double),
                ("occ_thresh", C.c_double), ("vehicle_mass", C.c_double), ("grav_acc", C.c_double),
                ("horiz_drag", C.c_double), ("vert_drag", C.c_double), ("paras_drag", C.c_double),
                ("speed_eps", C.c_double)]


class IsdfStats(C.Structure):
    _fields_ = [("n_units", C.c_int64), ("n_units_culled", C.c_int64), ("n_pairs", C.c_int64),
                ("n_grad_pairs", C.c_int64), ("overflow", C.c_int32), ("reserved", C.c_int32)]


class IsdfLbfgsParams(C.Structure):
    _fields_ = [("mem_size", C.c_int32), ("past", C.c_int32), ("max_iterations", C.c_int32), ("max_linesearch", C.c_int32),
                ("weak_wolfe", C.c_int32), ("reference_patches", C.c_int32),
                ("g_epsilon", C.c_double), ("delta", C.c_double), ("min_step", C.c_double), ("max_step", C.c_double),
                ("f_dec_coeff", C.c_double), ("s_curv_coeff", C.c_double), ("cautious_factor", C.c_double),
                ("machine_prec", C.c_double), ("dir_norm_cap", C.c_double)]


class IsdfFrontendConfig(C.Structure):
    _fields_ = [("kernel_size", C.c_int32), ("reserved", C.c_int32), ("kernel_max_roll", C.c_double), ("kernel_max_pitch", C.c_double),
                ("kernel_ang_res", C.c_double), ("front_end_safeh", C.c_double)]


def frontend_config(kernel_size=13, max_roll=45.0, max_pitch=45.0, ang_res=9.0, safeh=0.0):
    """The shipped configs' front-end values (config_*.yaml: kernel_max_roll 45, kernel_ang_res 9, front_end_safeh 0)."""
    c = IsdfFrontendConfig()
    c.kernel_size = int(kernel_size); c.kernel_max_roll = float(max_roll); c.kernel_max_pitch = float(max_pitch)
    c.kernel_ang_res = float(ang_res); c.front_end_safeh = float(safeh)
    return c


class IsdfAstarResult(C.Structure):
    """isdf_astar_result (include/isdf_accel.h)."""
    _fields_ = [("success", C.c_int32), ("n_path", C.c_int32), ("expansions", C.c_int64), ("checks", C.c_int64),
                ("cspace_ms", C.c_double), ("table_ms", C.c_double), ("search_ms", C.c_double)]


class IsdfFrontendFieldParams(C.Structure):
    """isdf_frontend_field_params (include/isdf_accel.h)."""
    _fields_ = [("max_rounds", C.c_int32), ("reserved", C.c_int32)]


class IsdfFrontendFieldInfo(C.Structure):
    """isdf_frontend_field_info (include/isdf_accel.h)."""
    _fields_ = [("reachable", C.c_int32), ("status", C.c_int32), ("rounds", C.c_int32), ("bricks", C.c_int32), ("brick_visits", C.c_int64),
                ("free_voxels", C.c_int64), ("reached_voxels", C.c_int64), ("device_ms", C.c_double)]


FIELD_REPAIR_DROP, FIELD_REPAIR_REPAIR = 0, 1           # isdf_frontend_field_set_repair


class IsdfFieldRepairInfo(C.Structure):
    """isdf_field_repair_info (include/isdf_accel.h)."""
    _fields_ = [("closed_voxels", C.c_int64), ("closed_reached", C.c_int64), ("tau", C.c_double), ("reset_voxels", C.c_int64),
                ("brick_visits", C.c_int64), ("free_voxels", C.c_int64), ("reached_voxels", C.c_int64), ("seeded_bricks", C.c_int32),
                ("rounds", C.c_int32), ("reachable", C.c_int32), ("status", C.c_int32), ("device_ms", C.c_double)]


FIELD_REOPEN_DROP, FIELD_REOPEN_LOWER = 0, 1             # isdf_frontend_field_set_reopen


FIELD_KNOWN_FOLLOW_DROP, FIELD_KNOWN_FOLLOW_FOLLOW = 0, 1    # isdf_frontend_field_set_known_follow


class IsdfFieldFollowInfo(C.Structure):
    """isdf_field_follow_info (include/isdf_accel.h)."""
    _fields_ = [("opening", C.c_int32), ("closing", C.c_int32), ("radius_used", C.c_int32), ("border", C.c_int32), ("known_voxels", C.c_int64),
                ("eroded_voxels", C.c_int64), ("opened_voxels", C.c_int64), ("closed_voxels", C.c_int64), ("free_voxels", C.c_int64),
                ("reached_voxels", C.c_int64), ("reachable", C.c_int32), ("status", C.c_int32), ("erode_ms", C.c_double), ("device_ms", C.c_double)]


class IsdfFieldReopenInfo(C.Structure):
    """isdf_field_reopen_info (include/isdf_accel.h)."""
    _fields_ = [("opened_voxels", C.c_int64), ("opened_reached", C.c_int64), ("reached_before", C.c_int64), ("reached_voxels", C.c_int64),
                ("free_voxels", C.c_int64), ("brick_visits", C.c_int64), ("seeded_bricks", C.c_int32), ("rounds", C.c_int32),
                ("goal_opened", C.c_int32), ("reachable", C.c_int32), ("status", C.c_int32), ("reserved", C.c_int32), ("device_ms", C.c_double)]


FIELD_SHIFT_DROP, FIELD_SHIFT_CARRY = 0, 1               # isdf_frontend_field_set_shift
FIELD_SHIFT_GOAL_LEFT = 3                                # isdf_frontend_field_shift_host: the goal cell left the window


class IsdfFieldShiftInfo(C.Structure):
    """isdf_field_shift_info (include/isdf_accel.h)."""
    _fields_ = [("shift", C.c_int32 * 3), ("goal_new", C.c_int32 * 3), ("left_reached", C.c_int64), ("closed_voxels", C.c_int64),
                ("closed_reached", C.c_int64), ("tau", C.c_double), ("reset_voxels", C.c_int64), ("opened_voxels", C.c_int64),
                ("opened_reached", C.c_int64), ("brick_visits", C.c_int64), ("free_voxels", C.c_int64), ("reached_voxels", C.c_int64),
                ("seeded_bricks_close", C.c_int32), ("rounds_close", C.c_int32), ("seeded_bricks_open", C.c_int32), ("rounds_open", C.c_int32),
                ("goal_opened", C.c_int32), ("reachable", C.c_int32), ("status", C.c_int32), ("reserved", C.c_int32), ("device_ms", C.c_double)]


MAP_UPDATE_NONE, MAP_UPDATE_INCREMENTAL, MAP_UPDATE_FULL = 0, 1, 2      # isdf_map_update_info.path


class IsdfMapUpdateParams(C.Structure):
    """isdf_map_update_params (include/isdf_accel.h)."""
    _fields_ = [("max_new_voxels", C.c_int64), ("full_fraction", C.c_double), ("refresh_esdf", C.c_int32), ("refresh_frontend", C.c_int32)]


class IsdfMapUpdateInfo(C.Structure):
    """isdf_map_update_info (include/isdf_accel.h)."""
    _fields_ = [("n_points", C.c_int64), ("n_new_voxels", C.c_int64), ("dirty_lo", C.c_int32 * 3), ("dirty_hi", C.c_int32 * 3),
                ("path", C.c_int32), ("esdf_refreshed", C.c_int32), ("frontend_refreshed", C.c_int32), ("cspace_refreshed", C.c_int32),
                ("host_table_patched", C.c_int32), ("field_dropped", C.c_int32), ("esdf_voxels_lowered", C.c_int64),
                ("cspace_voxels_recomputed", C.c_int64), ("count_ms", C.c_double), ("esdf_ms", C.c_double), ("frontend_ms", C.c_double)]


MAP_CLEAR_NONE, MAP_CLEAR_INCREMENTAL, MAP_CLEAR_FULL = 0, 1, 2         # isdf_map_clear_info.path


class IsdfMapClearParams(C.Structure):
    """isdf_map_clear_params (include/isdf_accel.h)."""
    _fields_ = [("max_cleared_voxels", C.c_int64), ("full_fraction", C.c_double), ("refresh_esdf", C.c_int32), ("refresh_frontend", C.c_int32)]


class IsdfMapClearInfo(C.Structure):
    """isdf_map_clear_info (include/isdf_accel.h)."""
    _fields_ = [("n_points", C.c_int64), ("n_points_ignored", C.c_int64), ("n_cleared_voxels", C.c_int64), ("dirty_lo", C.c_int32 * 3),
                ("dirty_hi", C.c_int32 * 3), ("touched_lo", C.c_int32 * 3), ("touched_hi", C.c_int32 * 3), ("path", C.c_int32),
                ("esdf_refreshed", C.c_int32), ("frontend_refreshed", C.c_int32), ("cspace_refreshed", C.c_int32),
                ("host_table_patched", C.c_int32), ("field_dropped", C.c_int32), ("watch_rechecked", C.c_int32), ("reserved", C.c_int32),
                ("esdf_voxels_recomputed", C.c_int64), ("esdf_voxels_raised", C.c_int64), ("cspace_voxels_recomputed", C.c_int64),
                ("count_ms", C.c_double), ("esdf_ms", C.c_double), ("frontend_ms", C.c_double)]


MAP_SHIFT_NONE, MAP_SHIFT_INCREMENTAL, MAP_SHIFT_FULL = 0, 1, 2         # isdf_map_shift_info.path


class IsdfMapShiftParams(C.Structure):
    """isdf_map_shift_params (include/isdf_accel.h)."""
    _fields_ = [("full_fraction", C.c_double), ("force_path", C.c_int32), ("reserved", C.c_int32 * 5)]


class IsdfMapShiftInfo(C.Structure):
    """isdf_map_shift_info (include/isdf_accel.h)."""
    _fields_ = [("path", C.c_int32), ("shift", C.c_int32 * 3), ("bmin_new", C.c_double * 3), ("voxels_entered", C.c_int64), ("occupied_left", C.c_int64),
                ("counts_left", C.c_int64), ("n_boxes", C.c_int32), ("host_table_patched", C.c_int32), ("field_dropped", C.c_int32),
                ("watch_rechecked", C.c_int32), ("cspace_voxels", C.c_int64), ("translate_ms", C.c_double), ("esdf_ms", C.c_double),
                ("frontend_ms", C.c_double), ("wall_ms", C.c_double)]


class IsdfMapKnownInfo(C.Structure):
    """isdf_map_known_info (include/isdf_accel.h)."""
    _fields_ = [("n_known", C.c_int64), ("n_unknown", C.c_int64), ("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3), ("newly_known", C.c_int64),
                ("merges", C.c_int64)]


class IsdfMapFrontierInfo(C.Structure):
    """isdf_map_frontier_info (include/isdf_accel.h)."""
    _fields_ = [("n_frontier", C.c_int64), ("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3), ("kernel_ms", C.c_double)]


class IsdfTrajKnownParams(C.Structure):
    """isdf_traj_known_params (include/isdf_accel.h)."""
    _fields_ = [("margin", C.c_double), ("mode", C.c_int32), ("reserved", C.c_int32)]


class IsdfTrajKnownInfo(C.Structure):
    """isdf_traj_known_info (include/isdf_accel.h)."""
    _fields_ = [("unknown_in_box", C.c_int64), ("candidates", C.c_int64), ("qualified", C.c_int64), ("n_below_margin", C.c_int64),
                ("n_penetrating", C.c_int64), ("horizon_t", C.c_double), ("horizon_voxel", C.c_int64), ("horizon_value", C.c_double),
                ("horizon_point", C.c_double * 3), ("horizon_piece", C.c_int32), ("culled", C.c_int32), ("min_clearance", C.c_double),
                ("min_voxel", C.c_int64), ("duration", C.c_double), ("margin", C.c_double), ("far_r", C.c_double), ("select_ms", C.c_double),
                ("field_ms", C.c_double), ("reduce_ms", C.c_double)]


class IsdfViewGainParams(C.Structure):
    """isdf_view_gain_params (include/isdf_accel.h)."""
    _fields_ = [("stride_u", C.c_int32), ("stride_v", C.c_int32), ("max_range_m", C.c_double), ("scratch_bytes", C.c_int64), ("reserved", C.c_int32 * 4)]


class IsdfViewGainInfo(C.Structure):
    """isdf_view_gain_info (include/isdf_accel.h)."""
    _fields_ = [("n_views", C.c_int64), ("n_scored", C.c_int64), ("n_rays_per_view", C.c_int64), ("best_view", C.c_int64), ("best_gain", C.c_int64),
                ("gain_total", C.c_int64), ("chunks", C.c_int32), ("reserved", C.c_int32), ("gain_ms", C.c_double)]


class IsdfFrontierClusterParams(C.Structure):
    """isdf_frontier_cluster_params (include/isdf_accel.h)."""
    _fields_ = [("connectivity", C.c_int32), ("reserved", C.c_int32), ("min_size", C.c_int64)]


class IsdfFrontierClusterInfo(C.Structure):
    """isdf_frontier_cluster_info (include/isdf_accel.h)."""
    _fields_ = [("n_voxels", C.c_int64), ("n_clusters", C.c_int64), ("n_rows", C.c_int64), ("n_voxels_dropped", C.c_int64), ("largest_size", C.c_int64),
                ("largest_label", C.c_int64), ("frontier_ms", C.c_double), ("label_ms", C.c_double), ("stats_ms", C.c_double)]


class IsdfViewCandidatesParams(C.Structure):
    """isdf_view_candidates_params (include/isdf_accel.h)."""
    _fields_ = [("gain", IsdfViewGainParams), ("clearance_voxels", C.c_int32), ("k_best", C.c_int32), ("min_gain", C.c_int64), ("reserved", C.c_int32 * 4)]


class IsdfViewCandidatesInfo(C.Structure):
    """isdf_view_candidates_info (include/isdf_accel.h)."""
    _fields_ = [("n_targets", C.c_int64), ("n_offsets", C.c_int64), ("n_candidates", C.c_int64), ("n_kept", C.c_int64), ("n_bad", C.c_int64),
                ("n_occupied", C.c_int64), ("n_unknown", C.c_int64), ("n_close", C.c_int64), ("n_blocked", C.c_int64), ("n_scored", C.c_int64),
                ("best_target", C.c_int64), ("best_candidate", C.c_int64), ("best_gain", C.c_int64), ("chunks", C.c_int32), ("reserved", C.c_int32),
                ("filter_ms", C.c_double), ("gain_ms", C.c_double), ("select_ms", C.c_double)]


class IsdfViewSelectParams(C.Structure):
    """isdf_view_select_params (include/isdf_accel.h)."""
    _fields_ = [("gain", IsdfViewGainParams), ("k_select", C.c_int32), ("reserved0", C.c_int32), ("min_gain", C.c_int64), ("reserved", C.c_int32 * 4)]


class IsdfViewSelectInfo(C.Structure):
    """isdf_view_select_info (include/isdf_accel.h)."""
    _fields_ = [("n_views", C.c_int64), ("n_scored", C.c_int64), ("n_selected", C.c_int64), ("gain_selected", C.c_int64), ("gain_solo_sum", C.c_int64),
                ("best_single_gain", C.c_int64), ("list_words", C.c_int64), ("chunks", C.c_int32), ("reserved", C.c_int32), ("gain_ms", C.c_double),
                ("lists_ms", C.c_double), ("select_ms", C.c_double)]


class IsdfViewSelectRoutedParams(C.Structure):
    """isdf_view_select_routed_params (include/isdf_accel.h)."""
    _fields_ = [("select", IsdfViewSelectParams), ("cost0", C.c_double), ("max_cost", C.c_double), ("path_cap", C.c_int32), ("reserved", C.c_int32 * 5)]


class IsdfViewSelectRoutedInfo(C.Structure):
    """isdf_view_select_routed_info (include/isdf_accel.h)."""
    _fields_ = [("select", IsdfViewSelectInfo), ("n_eligible", C.c_int64), ("n_unreachable", C.c_int64), ("n_over_budget", C.c_int64),
                ("cost_selected", C.c_double), ("cost_source", C.c_int32), ("reserved", C.c_int32), ("cost_ms", C.c_double), ("paths_ms", C.c_double)]


class IsdfKnownErodeParams(C.Structure):
    """isdf_known_erode_params (include/isdf_accel.h)."""
    _fields_ = [("radius", C.c_int32), ("border", C.c_int32)]


class IsdfKnownErodeInfo(C.Structure):
    """isdf_known_erode_info (include/isdf_accel.h)."""
    _fields_ = [("radius_used", C.c_int32), ("border", C.c_int32), ("known_voxels", C.c_int64), ("eroded_voxels", C.c_int64), ("erode_ms", C.c_double)]


VIEW_SELECT_ROW = 4                     # int64 per round: view, marginal, cumulative, overlap; a round that did not happen: -1, 0, 0, 0
# int64 per cluster: label, size, lo xyz, hi xyz, sum xyz, rep_voxel, rep_d2, first_pos, 0, 0
FRONTIER_CLUSTER_ROW = 16
# int64 per candidate view: status, eye_voxel, los_steps, gain, n_hits, steps_total, n_rays_unknown, rank; the statuses in the order of the tests
VIEW_CANDIDATE_ROW = 8
VIEW_CAND_KEPT, VIEW_CAND_BAD, VIEW_CAND_OCCUPIED, VIEW_CAND_UNKNOWN, VIEW_CAND_CLOSE, VIEW_CAND_BLOCKED = 0, 1, 2, 3, 4, 5
VIEW_GAIN_ROW = 8                       # int64 per view: status, gain, n_rays, n_skipped, n_hits, steps_total, n_rays_unknown, 0


class IsdfMapScanParams(C.Structure):
    """isdf_map_scan_params (include/isdf_accel.h)."""
    _fields_ = [("miss_weight", C.c_int32), ("reserved", C.c_int32), ("clear", IsdfMapClearParams), ("update", IsdfMapUpdateParams)]


class IsdfMapScanInfo(C.Structure):
    """isdf_map_scan_info (include/isdf_accel.h)."""
    _fields_ = [("n_rays", C.c_int64), ("n_rays_skipped", C.c_int64), ("n_hits", C.c_int64), ("n_free_voxels", C.c_int64),
                ("n_hit_voxels", C.c_int64), ("ray_lo", C.c_int32 * 3), ("ray_hi", C.c_int32 * 3), ("trace_ms", C.c_double),
                ("clear", IsdfMapClearInfo), ("update", IsdfMapUpdateInfo)]


class IsdfMapRaycastParams(C.Structure):
    """isdf_map_raycast_params (include/isdf_accel.h)."""
    _fields_ = [("test_origin_voxel", C.c_int32), ("per_ray_origin", C.c_int32), ("reserved", C.c_int32 * 2)]


class IsdfMapRaycastInfo(C.Structure):
    """isdf_map_raycast_info (include/isdf_accel.h)."""
    _fields_ = [("n_rays", C.c_int64), ("n_skipped", C.c_int64), ("n_origin_outside", C.c_int64), ("n_hits", C.c_int64), ("n_clear", C.c_int64),
                ("steps_total", C.c_int64), ("cast_ms", C.c_double)]


class IsdfDepthCamera(C.Structure):
    """isdf_depth_camera (include/isdf_accel.h)."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double)]


class IsdfDepthRenderParams(C.Structure):
    """isdf_depth_render_params (include/isdf_accel.h)."""
    _fields_ = [("splat_m", C.c_double), ("min_depth_m", C.c_double), ("max_splat_px", C.c_int32), ("source", C.c_int32), ("reserved", C.c_int32 * 4)]


class IsdfDepthRenderInfo(C.Structure):
    """isdf_depth_render_info (include/isdf_accel.h)."""
    _fields_ = [("n_points", C.c_int64), ("n_behind", C.c_int64), ("n_outside", C.c_int64), ("n_near", C.c_int64), ("n_splat_pixels", C.c_int64),
                ("n_pixels_set", C.c_int64), ("render_ms", C.c_double)]


class IsdfDepthRaysParams(C.Structure):
    """isdf_depth_rays_params (include/isdf_accel.h)."""
    _fields_ = [("stride_u", C.c_int32), ("stride_v", C.c_int32), ("min_range_m", C.c_double), ("max_range_m", C.c_double), ("no_return_is_free", C.c_int32),
                ("reserved", C.c_int32 * 3)]


class IsdfDepthRaysInfo(C.Structure):
    """isdf_depth_rays_info (include/isdf_accel.h)."""
    _fields_ = [("n_pixels", C.c_int64), ("n_no_return", C.c_int64), ("n_below_min", C.c_int64), ("n_truncated", C.c_int64), ("n_clipped", C.c_int64),
                ("n_hits", C.c_int64), ("rays_ms", C.c_double)]


DEPTH_SOURCE_CLOUD, DEPTH_SOURCE_MAP = 0, 1
DEPTH_I32_MM, DEPTH_U16_MM, DEPTH_F32_M = 0, 1, 2
DEPTH_EMPTY_MM = 999999
RAYCAST_CLEAR, RAYCAST_HIT, RAYCAST_END_OUTSIDE, RAYCAST_ORIGIN_OUTSIDE = 0, 1, 2, 3       # a row's status
RAYCAST_ROW = 8                                                                           # int32 per ray: status, steps, i, j, k, axis, num, den


class IsdfPlanConfig(C.Structure):
    """isdf_plan_config: what a plan needs from the reference's yaml files (include/isdf_accel.h)."""
    _fields_ = [("sweep", IsdfConfig), ("frontend", IsdfFrontendConfig), ("occupancy_resolution", C.c_double),
                ("sta_threshold", C.c_int32), ("threads_num", C.c_int32), ("rho", C.c_double), ("inittime", C.c_double),
                ("momentum", C.c_double), ("traj_parlength", C.c_double), ("poly_params", C.c_double * 6),
                ("offset_aabb", C.c_double * 3), ("box", C.c_double * 3), ("map_bound", C.c_double * 6),
                ("inputdata", C.c_char * 256), ("pcdmapname", C.c_char * 128)]


class IsdfMidendParams(C.Structure):
    """isdf_midend_params (include/isdf_accel.h): the mid end's weights and its driver's parameters."""
    _fields_ = [("weight_pr", C.c_double), ("rho_mid_end", C.c_double), ("rel_cost_tol", C.c_double), ("min_step", C.c_double),
                ("g_epsilon", C.c_double), ("integral_intervs", C.c_int32), ("mem_size", C.c_int32), ("past", C.c_int32),
                ("reserved", C.c_int32)]


class IsdfLbfgsResult(C.Structure):
    _fields_ = [("f", C.c_double), ("wall_ms", C.c_double), ("status", C.c_int32), ("iterations", C.c_int32),
                ("evaluations", C.c_int32), ("reserved", C.c_int32)]


SWEPT_FIELD_PLANNER, SWEPT_FIELD_CLOSED = 0, 1


class IsdfSweptMeshParams(C.Structure):
    _fields_ = [("eps", C.c_double), ("iso", C.c_double), ("mode", C.c_int32), ("band", C.c_int32), ("lipschitz", C.c_double),
                ("use_bbox", C.c_int32), ("reserved", C.c_int32), ("bmin", C.c_double * 3), ("bmax", C.c_double * 3)]


class IsdfSweptMeshInfo(C.Structure):
    _fields_ = [("dims", C.c_int32 * 3), ("reserved", C.c_int32), ("origin", C.c_double * 3), ("eps", C.c_double),
                ("coarse_points", C.c_int64), ("fine_points", C.c_int64), ("band_cells", C.c_int64), ("n_vertices", C.c_int64),
                ("n_triangles", C.c_int64), ("unqualified_edges", C.c_int64), ("field_ms", C.c_double), ("mesh_ms", C.c_double)]


class IsdfTrajCheckParams(C.Structure):
    _fields_ = [("margin", C.c_double), ("mode", C.c_int32), ("reserved", C.c_int32)]


class IsdfTrajCheckInfo(C.Structure):
    _fields_ = [("occupied_in_box", C.c_int64), ("candidates", C.c_int64), ("qualified", C.c_int64), ("n_below_margin", C.c_int64),
                ("n_penetrating", C.c_int64), ("min_clearance", C.c_double), ("min_tstar", C.c_double), ("min_point", C.c_double * 3),
                ("min_voxel", C.c_int64), ("min_piece", C.c_int32), ("culled", C.c_int32), ("margin", C.c_double), ("far_r", C.c_double),
                ("select_ms", C.c_double), ("field_ms", C.c_double), ("reduce_ms", C.c_double)]


TRAJ_WATCH_OFF, TRAJ_WATCH_FOLD = 0, 1                  # isdf_traj_check_set_watch
TRAJ_WATCH_PATH_NONE, TRAJ_WATCH_PATH_LIST, TRAJ_WATCH_PATH_FULL = 0, 1, 2      # isdf_traj_watch_info.path


class IsdfTrajWatchInfo(C.Structure):
    """isdf_traj_watch_info (include/isdf_accel.h)."""
    _fields_ = [("updates_folded", C.c_int64), ("new_voxels", C.c_int64), ("new_in_box", C.c_int64), ("new_candidates", C.c_int64),
                ("new_qualified", C.c_int64), ("new_below_margin", C.c_int64), ("new_penetrating", C.c_int64),
                ("new_min_clearance", C.c_double), ("new_min_tstar", C.c_double), ("new_min_voxel", C.c_int64),
                ("new_min_piece", C.c_int32), ("path", C.c_int32), ("min_changed", C.c_int32), ("reserved", C.c_int32),
                ("select_ms", C.c_double), ("field_ms", C.c_double), ("reduce_ms", C.c_double), ("merge_ms", C.c_double)]


LIMITS_CHANNELS, TRAJ_SAMPLE_ROW = 6, 20
LIMIT_SPEED, LIMIT_ACC, LIMIT_OMG, LIMIT_TILT, LIMIT_THRUST_MAX, LIMIT_THRUST_MIN = range(6)
LIMIT_NAMES = ["speed", "acc", "omg", "tilt", "thrust_max", "thrust_min"]


class IsdfTrajLimitsParams(C.Structure):
    _fields_ = [("samples", C.c_int32), ("reserved", C.c_int32), ("tol_t", C.c_double), ("max_acc", C.c_double),
                ("max_thrust", C.c_double), ("min_thrust", C.c_double)]


class IsdfTrajLimitsInfo(C.Structure):
    _fields_ = [("value", C.c_double * 6), ("time", C.c_double * 6), ("limit", C.c_double * 6), ("piece", C.c_int32 * 6),
                ("n_pieces_over", C.c_int32 * 6), ("judged", C.c_int32), ("feasible", C.c_int32), ("samples", C.c_int32),
                ("reserved", C.c_int32), ("tol_t", C.c_double), ("device_ms", C.c_double)]


RETIME_OK, RETIME_AT_LOWER, RETIME_NOT_REACHABLE = 0, 1, 2
TRAJ_RETIME_MAX_PIECES = 1 << 20


class IsdfTrajRetimeParams(C.Structure):
    _fields_ = [("s_lo", C.c_double), ("s_hi", C.c_double), ("ladder", C.c_int32), ("rounds", C.c_int32), ("check", C.c_int32),
                ("reserved", C.c_int32), ("limits", IsdfTrajLimitsParams)]


class IsdfTrajRetimeInfo(C.Structure):
    _fields_ = [("scale", C.c_double), ("scale_below", C.c_double), ("status", C.c_int32), ("rounds", C.c_int32), ("candidates", C.c_int32),
                ("nonmonotone", C.c_int32), ("binding", C.c_int32), ("checked", C.c_int32), ("duration_in", C.c_double),
                ("duration_out", C.c_double), ("limits", IsdfTrajLimitsInfo), ("check", IsdfTrajCheckInfo), ("device_ms", C.c_double)]


REALLOC_OK, REALLOC_ALREADY, REALLOC_NOT_REACHED = 0, 1, 2
TRAJ_REALLOC_MAX_ROUNDS, TRAJ_REALLOC_MAX_N = 16, 400


class IsdfTrajReallocParams(C.Structure):
    _fields_ = [("rounds", C.c_int32), ("check", C.c_int32), ("headroom", C.c_double), ("f_max", C.c_double), ("limits", IsdfTrajLimitsParams)]


class IsdfTrajReallocInfo(C.Structure):
    _fields_ = [("status", C.c_int32), ("rounds", C.c_int32), ("pieces_changed", C.c_int32), ("binding", C.c_int32), ("checked", C.c_int32),
                ("reserved", C.c_int32), ("duration_in", C.c_double), ("duration_out", C.c_double), ("max_factor", C.c_double),
                ("limits", IsdfTrajLimitsInfo), ("check", IsdfTrajCheckInfo), ("device_ms", C.c_double)]


class IsdfPointsMergeInfo(C.Structure):
    _fields_ = [("M_before", C.c_int32), ("M_after", C.c_int32), ("n_rows", C.c_int32), ("n_added", C.c_int32),
                ("n_duplicate", C.c_int32), ("n_outside", C.c_int32), ("reserved", C.c_int32 * 2), ("merge_ms", C.c_double)]


class IsdfRefineParams(C.Structure):
    _fields_ = [("max_rounds", C.c_int32), ("mode", C.c_int32), ("margin", C.c_double), ("below", C.c_double)]


class IsdfRefineResult(C.Structure):
    _fields_ = [("rounds", C.c_int32), ("clear", C.c_int32), ("stalled", C.c_int32), ("reserved", C.c_int32),
                ("M_round", C.c_int32 * 16), ("last_opt", IsdfLbfgsResult), ("last_check", IsdfTrajCheckInfo)]


EVALUATE_FN = C.CFUNCTYPE(C.c_double, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int)
PROGRESS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.c_double, C.c_int, C.c_int)   # isdf_progress_fn


# every symbol include/isdf_accel.h declares (tests check the .so exports all of them)
EXPORTED_SYMBOLS = [
    "isdf_config_default", "isdf_shape_default", "isdf_shape_from_name", "isdf_create", "isdf_destroy",
    "isdf_last_error", "isdf_abi_version", "isdf_set_grid", "isdf_set_shape", "isdf_set_points",
    "isdf_set_shard", "isdf_eval", "isdf_eval_device", "isdf_eval_swept_at_tstar", "isdf_eval_swept_at_tstar_host", "isdf_out_stride", "isdf_profile_enable",
    "isdf_profile_read", "isdf_profile_read_secondary", "isdf_get_stats",
    "isdf_set_trajectory", "isdf_num_variables", "isdf_pack_variables", "isdf_unpack_variables",
    "isdf_cost_function", "isdf_cost_function_lmbm", "isdf_cost_parts",
    "isdf_cost_function_launch", "isdf_cost_function_finish", "isdf_set_minco_mode", "isdf_minco_path",
    "isdf_lbfgs_params_default", "isdf_lbfgs_minimize", "isdf_optimize_lbfgs", "isdf_optimize_lbfgs_batch",
    "isdf_set_pointcloud", "isdf_generate_esdf", "isdf_get_grid", "isdf_gather_points", "isdf_get_points", "isdf_shape_eval",
    "isdf_esdf_sample", "isdf_esdf_sample_device", "isdf_esdf_sample_scattered", "isdf_esdf_sample_scattered_device",
    "isdf_frontend_build", "isdf_frontend_get_shape_kernels", "isdf_frontend_get_map_kernel", "isdf_frontend_check", "isdf_frontend_cspace",
    "isdf_frontend_astar_search", "isdf_frontend_astar_path", "isdf_host_info", "isdf_debug_live_bytes", "isdf_debug_live_events",
    "isdf_read_pcd", "isdf_read_obj", "isdf_poly_rotation", "isdf_body_transform", "isdf_plan_config_default", "isdf_load_yaml_config",
    "isdf_shape_from_config",
    "isdf_host_path", "isdf_mesh_atan2f", "isdf_create_multi", "isdf_multi_info", "isdf_set_shape_grid", "isdf_set_shape_sampled",
    "isdf_xchg_create", "isdf_xchg_connect", "isdf_xchg_allreduce", "isdf_xchg_fuse", "isdf_xchg_status", "isdf_xchg_destroy",
    "isdf_xchg_timeout_ms", "isdf_xchg_set_timeout_ms", "isdf_lbfgs_minimize_progress", "isdf_set_progress", "isdf_mesh_info",
    "isdf_swept_sdf", "isdf_swept_sdf_device", "isdf_swept_mesh_params_default", "isdf_swept_mesh_build", "isdf_swept_mesh_get",
    "isdf_swept_mesh_release", "isdf_lattice_mesh_build", "isdf_write_obj", "isdf_traj_check_params_default", "isdf_traj_check", "isdf_traj_check_device",
    "isdf_traj_check_get", "isdf_traj_check_release", "isdf_traj_collide",
    "isdf_traj_check_set_watch", "isdf_traj_check_watch_info", "isdf_traj_check_watch_sizes", "isdf_traj_check_fold_host",
    "isdf_points_merge_check", "isdf_refine_params_default", "isdf_optimize_lbfgs_checked",
    "isdf_midend_params_default", "isdf_load_yaml_midend", "isdf_midend_cost", "isdf_midend_cost_batch", "isdf_midend_fit",
    "isdf_midend_fit_batch",
    "isdf_set_shape_program", "isdf_shape_program_eval_host", "isdf_shape_program_validate",
    "isdf_traj_limits_params_default", "isdf_traj_limits", "isdf_traj_limits_device", "isdf_traj_limits_batch", "isdf_traj_limits_host",
    "isdf_traj_sample", "isdf_traj_sample_device", "isdf_traj_sample_host", "isdf_traj_limits_sizes",
    "isdf_traj_retime_params_default", "isdf_traj_retime", "isdf_traj_retime_device", "isdf_traj_retime_batch", "isdf_traj_retime_host",
    "isdf_traj_scale_host", "isdf_traj_retime_sizes",
    "isdf_traj_realloc_params_default", "isdf_traj_realloc", "isdf_traj_realloc_device", "isdf_traj_realloc_batch", "isdf_traj_realloc_host",
    "isdf_traj_minco_host", "isdf_traj_realloc_sizes",
    "isdf_frontend_field_params_default", "isdf_frontend_field_build", "isdf_frontend_field_get", "isdf_frontend_field_value",
    "isdf_frontend_field_paths", "isdf_frontend_field_paths_device", "isdf_frontend_field_host", "isdf_frontend_field_release",
    "isdf_frontend_field_set_repair", "isdf_frontend_field_repair_info", "isdf_frontend_field_repair_sizes", "isdf_frontend_field_repair_host",
    "isdf_frontend_field_set_reopen", "isdf_frontend_field_reopen_info", "isdf_frontend_field_reopen_sizes", "isdf_frontend_field_reopen_host",
    "isdf_frontend_field_set_shift", "isdf_frontend_field_shift_info", "isdf_frontend_field_shift_sizes", "isdf_frontend_field_shift_host",
    "isdf_map_update_params_default", "isdf_map_update_sizes", "isdf_update_pointcloud", "isdf_update_voxels", "isdf_map_counts_get", "isdf_frontend_cspace_get",
    "isdf_map_clear_params_default", "isdf_map_clear_sizes", "isdf_clear_pointcloud", "isdf_clear_voxels", "isdf_clear_esdf_host", "isdf_clear_touched_host",
    "isdf_map_scan_params_default", "isdf_map_scan_sizes", "isdf_integrate_scan", "isdf_scan_sets_host", "isdf_scan_ray_host",
    "isdf_map_raycast_params_default", "isdf_map_raycast_sizes", "isdf_map_raycast", "isdf_map_raycast_device", "isdf_raycast_host",
    "isdf_depth_render_params_default", "isdf_depth_render_sizes", "isdf_depth_render", "isdf_depth_render_device", "isdf_depth_render_host",
    "isdf_depth_rays_params_default", "isdf_depth_rays_sizes", "isdf_depth_rays_rows", "isdf_depth_rays", "isdf_depth_rays_device", "isdf_depth_rays_host",
    "isdf_integrate_depth",
    "isdf_map_shift_params_default", "isdf_map_shift_sizes", "isdf_shift_map", "isdf_map_follow", "isdf_shift_geometry_host", "isdf_shift_grid_host",
    "isdf_shift_bands_host",
    "isdf_map_known_sizes", "isdf_map_known_enable", "isdf_map_known_fill", "isdf_map_known_merge_ms", "isdf_map_known_get", "isdf_map_frontier",
    "isdf_traj_known_params_default", "isdf_traj_known_horizon", "isdf_traj_known_horizon_device",
    "isdf_known_merge_host", "isdf_known_shift_host", "isdf_known_fill_host", "isdf_known_frontier_host",
    "isdf_view_gain_params_default", "isdf_view_gain_sizes", "isdf_view_gain", "isdf_view_gain_device", "isdf_view_gain_host",
    "isdf_frontier_cluster_params_default", "isdf_frontier_cluster_sizes", "isdf_map_frontier_clusters", "isdf_known_clusters_host",
    "isdf_view_candidates_params_default", "isdf_view_candidates_sizes", "isdf_view_candidates", "isdf_view_candidates_host",
    "isdf_view_select_params_default", "isdf_view_select_sizes", "isdf_view_select", "isdf_view_select_host",
    "isdf_view_select_routed_params_default", "isdf_view_select_routed_sizes", "isdf_view_select_routed", "isdf_view_select_routed_host",
    "isdf_known_erode_params_default", "isdf_known_erode_sizes", "isdf_map_known_erode", "isdf_known_erode_host", "isdf_frontend_field_build_known",
    "isdf_frontend_field_known_info",
    "isdf_frontend_field_set_known_follow", "isdf_frontend_field_follow_info", "isdf_frontend_field_follow_sizes",
]

HOST_PATH_COPY, HOST_PATH_DIRECT_MAPPED, HOST_PATH_DIRECT_BAR, HOST_PATH_DEVICE_CALLBACK = 0, 1, 2, 3
MINCO_AUTO, MINCO_HOST, MINCO_DEVICE = 0, 1, 2
MULTI_NONE, MULTI_PEER_SUM, MULTI_STAGED, MULTI_RCCL = 0, 1, 2, 3

SDF_WITH_GRAD_FN = C.CFUNCTYPE(C.c_double, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double))   # isdf_sdf_with_grad_fn
SHAPE_GRID, GRAD_GRID = 16, 4
SHAPE_PROGRAM = 17
PROGRAM_MAX_INSTR, PROGRAM_MAX_DEPTH = 64, 8


class IsdfShapeInstr(C.Structure):      # isdf_shape_instr
    _fields_ = [("op", C.c_int32), ("reserved", C.c_int32), ("p", C.c_double * 9)]


# isdf_shape_op
(OP_SPHERE, OP_CAPSULE, OP_BOX, OP_ROUNDED_BOX, OP_WIREFRAME_BOX, OP_TORUS, OP_CYLINDER, OP_CAPPED_CYLINDER, OP_ROUNDED_CYLINDER,
 OP_CAPPED_CONE, OP_ROUNDED_CONE, OP_ELLIPSOID, OP_PYRAMID, OP_TETRAHEDRON, OP_OCTAHEDRON, OP_DODECAHEDRON, OP_ICOSAHEDRON) = range(1, 18)
OP_TRANSLATE, OP_SCALE, OP_ROTATE, OP_ROTATE_TO, OP_TWIST, OP_BEND = range(32, 38)
OP_MUL, OP_NEGATE, OP_DILATE, OP_ERODE, OP_SHELL = range(48, 53)
OP_UNION, OP_DIFFERENCE, OP_INTERSECTION, OP_BLEND = range(64, 68)

_lib = None


def load_library(path=None):
    """dlopen libisdf_accel.so (built by __graft_entry__.build()).  Raises if it is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("ISDF_ACCEL_LIB") or LIB_PATH      # ISDF_ACCEL_LIB: developer A/B of two builds on one box
    if not os.path.exists(p):
        raise RuntimeError(f"{p} not found: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()'). "
                           "There is no CPU fallback for the product path.")
    lib = C.CDLL(p)
    dp = C.POINTER(C.c_double)
    lib.isdf_config_default.argtypes = [C.POINTER(IsdfConfig)]
    lib.isdf_config_default.restype = None
    lib.isdf_shape_default.argtypes = [C.POINTER(IsdfShape), C.c_int]
    lib.isdf_shape_from_name.argtypes = [C.POINTER(IsdfShape), C.c_char_p]
    lib.isdf_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(IsdfConfig)]
    lib.isdf_destroy.argtypes = [C.c_void_p]
    lib.isdf_create_multi.argtypes = [C.POINTER(C.c_void_p), C.POINTER(IsdfConfig), C.POINTER(C.c_int), C.c_int]
    lib.isdf_multi_info.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.isdf_last_error.argtypes = [C.c_void_p]
    lib.isdf_last_error.restype = C.c_char_p
    lib.isdf_set_grid.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, dp, dp, C.c_double, C.c_int]
    lib.isdf_set_shape.argtypes = [C.c_void_p, C.POINTER(IsdfShape)]
    lib.isdf_set_points.argtypes = [C.c_void_p, dp, C.c_int]
    lib.isdf_set_shape_grid.argtypes = [C.c_void_p, dp, C.c_int, C.c_int, C.c_int, dp, C.c_double, C.c_double, dp, dp]
    lib.isdf_set_shape_sampled.argtypes = [C.c_void_p, SDF_WITH_GRAD_FN, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, dp, dp]
    ins = C.POINTER(IsdfShapeInstr)
    lib.isdf_set_shape_program.argtypes = [C.c_void_p, ins, C.c_int, dp, dp, C.c_double, dp, dp]
    lib.isdf_shape_program_eval_host.argtypes = [ins, C.c_int, dp, dp, dp, C.c_longlong, dp, dp]
    lib.isdf_shape_program_validate.argtypes = [ins, C.c_int, C.c_char_p, C.c_int]
    lib.isdf_set_shard.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.isdf_eval.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(dp), C.POINTER(dp), dp,
                              C.POINTER(dp), C.POINTER(dp), dp]
    lib.isdf_eval_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.isdf_eval_swept_at_tstar.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.isdf_eval_swept_at_tstar_host.argtypes = [C.c_void_p, C.c_int, dp, dp, dp, dp, dp, dp]
    lib.isdf_out_stride.argtypes = [C.c_int]
    lib.isdf_out_stride.restype = C.c_size_t
    lib.isdf_profile_enable.argtypes = [C.c_void_p, C.c_int]
    lib.isdf_profile_read.argtypes = [C.c_void_p, C.POINTER(C.c_int), dp]
    lib.isdf_profile_read_secondary.argtypes = [C.c_void_p, dp]
    lib.isdf_get_stats.argtypes = [C.c_void_p, C.POINTER(IsdfStats)]
    lib.isdf_host_path.argtypes = [C.c_void_p]
    lib.isdf_mesh_atan2f.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_longlong, C.POINTER(C.c_float)]
    lib.isdf_set_trajectory.argtypes = [C.c_void_p, C.c_int, dp, dp, C.c_double]
    lib.isdf_num_variables.argtypes = [C.c_void_p]
    lib.isdf_pack_variables.argtypes = [C.c_void_p, dp, dp, dp]
    lib.isdf_unpack_variables.argtypes = [C.c_void_p, dp, dp, dp]
    lib.isdf_cost_function.argtypes = [C.c_void_p, dp, dp, C.c_int, dp]
    lib.isdf_cost_function_lmbm.argtypes = [C.c_void_p, dp, dp, C.c_int]
    lib.isdf_cost_function_lmbm.restype = C.c_double
    lib.isdf_cost_parts.argtypes = [C.c_void_p, dp]
    lib.isdf_cost_function_launch.argtypes = [C.c_void_p, dp, C.c_int, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    lib.isdf_cost_function_finish.argtypes = [C.c_void_p, dp, dp, C.c_void_p]
    lib.isdf_set_minco_mode.argtypes = [C.c_void_p, C.c_int]
    lib.isdf_minco_path.argtypes = [C.c_void_p]
    ip = C.POINTER(C.c_int)
    lib.isdf_set_pointcloud.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_longlong, dp, dp, C.c_double, C.c_int, ip]
    lib.isdf_generate_esdf.argtypes = [C.c_void_p]
    lib.isdf_get_grid.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, ip, dp, dp]
    lib.isdf_gather_points.argtypes = [C.c_void_p, dp, C.c_int, dp, dp, ip]
    lib.isdf_get_points.argtypes = [C.c_void_p, dp, C.c_int]
    lib.isdf_shape_eval.argtypes = [C.c_void_p, dp, C.c_int, dp, dp]
    lib.isdf_esdf_sample.argtypes = [C.c_void_p, dp, C.c_longlong, dp, dp]
    lib.isdf_esdf_sample_device.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.isdf_esdf_sample_scattered.argtypes = [C.c_void_p, dp, C.c_longlong, dp, dp]
    lib.isdf_esdf_sample_scattered_device.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.isdf_frontend_build.argtypes = [C.c_void_p, C.POINTER(IsdfFrontendConfig)]
    lib.isdf_frontend_get_shape_kernels.argtypes = [C.c_void_p, C.c_void_p, ip]
    lib.isdf_frontend_get_map_kernel.argtypes = [C.c_void_p, C.c_void_p, ip]
    lib.isdf_xchg_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p]
    lib.isdf_xchg_connect.argtypes = [C.c_void_p, C.c_void_p]
    lib.isdf_xchg_allreduce.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.isdf_xchg_fuse.argtypes = [C.c_void_p, C.c_int]
    lib.isdf_xchg_status.argtypes = [C.c_void_p]
    lib.isdf_xchg_destroy.argtypes = [C.c_void_p]
    lib.isdf_xchg_timeout_ms.argtypes = [C.c_void_p]
    lib.isdf_xchg_timeout_ms.restype = C.c_double
    lib.isdf_xchg_set_timeout_ms.argtypes = [C.c_void_p, C.c_double]
    lib.isdf_frontend_cspace.argtypes = [C.c_void_p, C.c_void_p, dp]
    lib.isdf_host_info.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    lib.isdf_debug_live_bytes.argtypes = [C.POINTER(C.c_longlong)]
    lib.isdf_debug_live_bytes.restype = None
    lib.isdf_debug_live_events.argtypes = []
    lib.isdf_debug_live_events.restype = C.c_longlong
    lib.isdf_frontend_astar_search.argtypes = [C.c_void_p, dp, dp, C.POINTER(IsdfAstarResult)]
    lib.isdf_frontend_astar_path.argtypes = [C.c_void_p, C.c_int, dp, dp, dp]
    lib.isdf_frontend_field_params_default.argtypes = [C.POINTER(IsdfFrontendFieldParams)]
    lib.isdf_frontend_field_params_default.restype = None
    lib.isdf_frontend_field_build.argtypes = [C.c_void_p, dp, C.POINTER(IsdfFrontendFieldParams), C.POINTER(IsdfFrontendFieldInfo)]
    lib.isdf_frontend_field_get.argtypes = [C.c_void_p, dp]
    lib.isdf_frontend_field_value.argtypes = [C.c_void_p, dp, C.c_int, dp]
    lib.isdf_frontend_field_paths.argtypes = [C.c_void_p, dp, C.c_int, C.c_int, C.c_void_p, dp, dp]
    lib.isdf_frontend_field_paths_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.isdf_frontend_field_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, dp]
    lib.isdf_frontend_field_release.argtypes = [C.c_void_p]
    lib.isdf_frontend_check.argtypes = [C.c_void_p, C.c_int, C.c_void_p, dp, dp, C.c_void_p, dp, dp, C.c_void_p]
    lib.isdf_lbfgs_params_default.argtypes = [C.POINTER(IsdfLbfgsParams)]
    lib.isdf_lbfgs_params_default.restype = None
    lib.isdf_lbfgs_minimize.argtypes = [EVALUATE_FN, C.c_void_p, dp, C.c_int, C.POINTER(IsdfLbfgsParams), C.POINTER(IsdfLbfgsResult)]
    lib.isdf_lbfgs_minimize_progress.argtypes = [EVALUATE_FN, PROGRESS_FN, C.c_void_p, dp, C.c_int, C.POINTER(IsdfLbfgsParams), C.POINTER(IsdfLbfgsResult)]
    lib.isdf_mesh_info.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    lib.isdf_set_progress.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    lib.isdf_optimize_lbfgs_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, dp, dp, C.c_double, dp, C.POINTER(IsdfLbfgsParams),
                                              C.POINTER(IsdfLbfgsResult), dp]
    lib.isdf_optimize_lbfgs.argtypes = [C.c_void_p, dp, C.c_int, C.POINTER(IsdfLbfgsParams), C.POINTER(IsdfLbfgsResult)]
    lib.isdf_read_pcd.argtypes = [C.c_char_p, C.POINTER(C.c_float), C.c_longlong]
    lib.isdf_read_pcd.restype = C.c_longlong
    lib.isdf_read_obj.argtypes = [C.c_char_p, dp, C.c_int, C.POINTER(C.c_int32), C.c_int, ip, ip]
    lib.isdf_poly_rotation.argtypes = [dp, dp]
    lib.isdf_body_transform.argtypes = [dp, dp, C.c_int, dp, dp]
    lib.isdf_plan_config_default.argtypes = [C.POINTER(IsdfPlanConfig)]
    lib.isdf_plan_config_default.restype = None
    lib.isdf_load_yaml_config.argtypes = [C.c_char_p, C.POINTER(IsdfPlanConfig)]
    mp = C.POINTER(IsdfMidendParams)
    lib.isdf_midend_params_default.argtypes = [mp]
    lib.isdf_midend_params_default.restype = None
    lib.isdf_load_yaml_midend.argtypes = [C.c_char_p, mp]
    lib.isdf_midend_cost.argtypes = [C.c_void_p, mp, dp, dp, dp, C.c_int, dp, dp]
    lib.isdf_midend_cost_batch.argtypes = [C.c_void_p, mp, C.c_int, dp, dp, dp, dp, dp, dp]
    lib.isdf_midend_fit.argtypes = [C.c_void_p, mp, dp, dp, dp, dp, dp, C.POINTER(IsdfLbfgsResult)]
    lib.isdf_midend_fit_batch.argtypes = [C.c_void_p, mp, C.c_int, C.c_int, dp, dp, dp, dp, dp, C.POINTER(IsdfLbfgsResult), dp]
    lib.isdf_shape_from_config.argtypes = [C.POINTER(IsdfShape), C.POINTER(IsdfPlanConfig), C.c_char_p, dp, C.c_int, C.POINTER(C.c_int32), C.c_int]
    lib.isdf_swept_sdf.argtypes = [C.c_void_p, C.c_int, dp, dp, dp, C.c_longlong, C.c_int, dp, dp]
    lib.isdf_swept_sdf_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p,
                                          C.c_void_p, C.c_void_p]
    lib.isdf_swept_mesh_params_default.argtypes = [C.POINTER(IsdfSweptMeshParams)]
    lib.isdf_swept_mesh_params_default.restype = None
    lib.isdf_swept_mesh_build.argtypes = [C.c_void_p, C.c_int, dp, dp, C.POINTER(IsdfSweptMeshParams), C.POINTER(IsdfSweptMeshInfo)]
    lib.isdf_swept_mesh_get.argtypes = [C.c_void_p, dp, C.c_int, C.POINTER(C.c_int32), C.c_int]
    lib.isdf_swept_mesh_release.argtypes = [C.c_void_p]
    lib.isdf_lattice_mesh_build.argtypes = [C.c_void_p, C.POINTER(C.c_int32), dp, C.c_double, C.c_double, dp, C.POINTER(IsdfSweptMeshInfo)]
    lib.isdf_write_obj.argtypes = [C.c_char_p, dp, C.c_int, C.POINTER(C.c_int32), C.c_int]
    lib.isdf_traj_check_params_default.argtypes = [C.POINTER(IsdfTrajCheckParams)]
    lib.isdf_traj_check_params_default.restype = None
    lib.isdf_traj_check.argtypes = [C.c_void_p, C.c_int, dp, dp, C.POINTER(IsdfTrajCheckParams), C.POINTER(IsdfTrajCheckInfo), dp]
    lib.isdf_traj_check_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(IsdfTrajCheckParams),
                                           C.POINTER(IsdfTrajCheckInfo), C.c_void_p, C.c_void_p]
    lib.isdf_traj_check_get.argtypes = [C.c_void_p, dp, C.c_longlong]
    lib.isdf_traj_check_release.argtypes = [C.c_void_p]
    lib.isdf_traj_check_set_watch.argtypes = [C.c_void_p, C.c_int]
    lib.isdf_traj_check_watch_info.argtypes = [C.c_void_p, C.POINTER(IsdfTrajCheckInfo), dp, C.POINTER(IsdfTrajWatchInfo)]
    lib.isdf_traj_check_watch_sizes.argtypes = [C.POINTER(C.c_int)]
    lib.isdf_traj_check_watch_sizes.restype = None
    lib.isdf_traj_check_fold_host.argtypes = [C.c_int, C.POINTER(IsdfTrajCheckInfo), dp, dp, C.c_void_p, C.POINTER(IsdfTrajCheckInfo), dp, dp, C.c_void_p,
                                              C.POINTER(IsdfTrajCheckInfo), dp, dp, C.c_void_p, C.c_longlong]
    wsz = (C.c_int * 1)()
    lib.isdf_traj_check_watch_sizes(wsz)
    if wsz[0] != C.sizeof(IsdfTrajWatchInfo):
        raise RuntimeError(f"isdf_traj_watch_info: the library has {wsz[0]}, the mirror {C.sizeof(IsdfTrajWatchInfo)}")
    lib.isdf_traj_collide.argtypes = [C.c_void_p, C.c_int, dp, dp]
    lib.isdf_points_merge_check.argtypes = [C.c_void_p, C.c_double, C.POINTER(IsdfPointsMergeInfo)]
    lib.isdf_refine_params_default.argtypes = [C.POINTER(IsdfRefineParams)]
    lib.isdf_refine_params_default.restype = None
    lib.isdf_optimize_lbfgs_checked.argtypes = [C.c_void_p, dp, C.c_int, C.POINTER(IsdfLbfgsParams), C.POINTER(IsdfRefineParams),
                                                C.POINTER(IsdfRefineResult)]
    lp, li = C.POINTER(IsdfTrajLimitsParams), C.POINTER(IsdfTrajLimitsInfo)
    lib.isdf_traj_limits_params_default.argtypes = [lp]
    lib.isdf_traj_limits_params_default.restype = None
    lib.isdf_traj_limits_sizes.argtypes = [ip]
    lib.isdf_traj_limits_sizes.restype = None
    lib.isdf_traj_limits.argtypes = [C.c_void_p, C.c_int, dp, dp, lp, li, dp]
    lib.isdf_traj_limits_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, lp, li, C.c_void_p, C.c_void_p]
    lib.isdf_traj_limits_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, dp, dp, lp, li, dp]
    lib.isdf_traj_limits_host.argtypes = [C.POINTER(IsdfConfig), C.c_int, dp, dp, lp, li, dp]
    lib.isdf_traj_sample.argtypes = [C.c_void_p, C.c_int, dp, dp, C.c_longlong, dp, dp]
    lib.isdf_traj_sample_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.isdf_traj_sample_host.argtypes = [C.POINTER(IsdfConfig), C.c_int, dp, dp, C.c_longlong, dp, dp]
    rp, ri = C.POINTER(IsdfTrajRetimeParams), C.POINTER(IsdfTrajRetimeInfo)
    lib.isdf_traj_retime_params_default.argtypes = [rp]
    lib.isdf_traj_retime_params_default.restype = None
    lib.isdf_traj_retime_sizes.argtypes = [ip]
    lib.isdf_traj_retime_sizes.restype = None
    lib.isdf_traj_retime.argtypes = [C.c_void_p, C.c_int, dp, dp, rp, dp, dp, ri]
    lib.isdf_traj_retime_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, rp, C.c_void_p, C.c_void_p, ri, C.c_void_p]
    lib.isdf_traj_retime_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, dp, dp, rp, dp, dp, ri]
    lib.isdf_traj_retime_host.argtypes = [C.POINTER(IsdfConfig), C.c_int, dp, dp, rp, dp, dp, ri]
    lib.isdf_traj_scale_host.argtypes = [C.c_int, dp, dp, C.c_double, dp, dp]
    sz = (C.c_int * 2)()
    lib.isdf_traj_retime_sizes(sz)
    if list(sz) != [C.sizeof(IsdfTrajRetimeParams), C.sizeof(IsdfTrajRetimeInfo)]:
        raise RuntimeError(f"isdf_traj_retime structs: the library has {list(sz)}, the mirror "
                           f"{[C.sizeof(IsdfTrajRetimeParams), C.sizeof(IsdfTrajRetimeInfo)]}")
    ap, ai = C.POINTER(IsdfTrajReallocParams), C.POINTER(IsdfTrajReallocInfo)
    lib.isdf_traj_realloc_params_default.argtypes = [ap]
    lib.isdf_traj_realloc_params_default.restype = None
    lib.isdf_traj_realloc_sizes.argtypes = [ip]
    lib.isdf_traj_realloc_sizes.restype = None
    lib.isdf_traj_realloc.argtypes = [C.c_void_p, C.c_int, dp, dp, dp, dp, ap, dp, dp, ai]
    lib.isdf_traj_realloc_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, ap, C.c_void_p, C.c_void_p, ai, C.c_void_p]
    lib.isdf_traj_realloc_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, dp, dp, dp, dp, ap, dp, dp, ai]
    lib.isdf_traj_realloc_host.argtypes = [C.POINTER(IsdfConfig), C.c_int, dp, dp, dp, dp, ap, dp, dp, ai]
    lib.isdf_traj_minco_host.argtypes = [C.c_int, dp, dp, dp, dp, dp]
    lib.isdf_traj_realloc_sizes(sz)
    if list(sz) != [C.sizeof(IsdfTrajReallocParams), C.sizeof(IsdfTrajReallocInfo)]:
        raise RuntimeError(f"isdf_traj_realloc structs: the library has {list(sz)}, the mirror "
                           f"{[C.sizeof(IsdfTrajReallocParams), C.sizeof(IsdfTrajReallocInfo)]}")
    up, ui = C.POINTER(IsdfMapUpdateParams), C.POINTER(IsdfMapUpdateInfo)
    lib.isdf_map_update_params_default.argtypes = [up]
    lib.isdf_map_update_params_default.restype = None
    lib.isdf_map_update_sizes.argtypes = [ip]
    lib.isdf_map_update_sizes.restype = None
    lib.isdf_update_pointcloud.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_longlong, up, ui]
    lib.isdf_update_voxels.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_longlong, up, ui]
    lib.isdf_map_counts_get.argtypes = [C.c_void_p, C.c_void_p]
    lib.isdf_frontend_cspace_get.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.isdf_map_update_sizes(sz)
    if list(sz) != [C.sizeof(IsdfMapUpdateParams), C.sizeof(IsdfMapUpdateInfo)]:
        raise RuntimeError(f"isdf_map_update structs: the library has {list(sz)}, the mirror "
                           f"{[C.sizeof(IsdfMapUpdateParams), C.sizeof(IsdfMapUpdateInfo)]}")
    cp, ci = C.POINTER(IsdfMapClearParams), C.POINTER(IsdfMapClearInfo)
    lib.isdf_map_clear_params_default.argtypes = [cp]
    lib.isdf_map_clear_params_default.restype = None
    lib.isdf_map_clear_sizes.argtypes = [ip]
    lib.isdf_map_clear_sizes.restype = None
    lib.isdf_clear_pointcloud.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_longlong, cp, ci]
    lib.isdf_clear_voxels.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_longlong, cp, ci]
    lib.isdf_clear_esdf_host.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_double, C.c_void_p, C.c_longlong, ci]
    lib.isdf_clear_touched_host.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_double, C.c_void_p, C.c_longlong, C.c_void_p]
    lib.isdf_clear_touched_host.restype = C.c_longlong
    lib.isdf_map_clear_sizes(sz)
    if list(sz) != [C.sizeof(IsdfMapClearParams), C.sizeof(IsdfMapClearInfo)]:
        raise RuntimeError(f"isdf_map_clear structs: the library has {list(sz)}, the mirror "
                           f"{[C.sizeof(IsdfMapClearParams), C.sizeof(IsdfMapClearInfo)]}")
    sp, si = C.POINTER(IsdfMapScanParams), C.POINTER(IsdfMapScanInfo)
    lib.isdf_map_scan_params_default.argtypes = [sp]
    lib.isdf_map_scan_params_default.restype = None
    lib.isdf_map_scan_sizes.argtypes = [ip]
    lib.isdf_map_scan_sizes.restype = None
    lib.isdf_integrate_scan.argtypes = [C.c_void_p, dp, C.POINTER(C.c_float), C.c_void_p, C.c_longlong, sp, si]
    lib.isdf_scan_sets_host.argtypes = [dp, dp, C.c_double, C.POINTER(C.c_int32), dp, C.POINTER(C.c_float), C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p,
                                        C.POINTER(C.c_longlong)]
    lib.isdf_scan_sets_host.restype = C.c_longlong
    lib.isdf_scan_ray_host.argtypes = [dp, dp, C.c_double, C.POINTER(C.c_int32), dp, C.POINTER(C.c_float), C.c_void_p, C.c_longlong]
    lib.isdf_scan_ray_host.restype = C.c_longlong
    lib.isdf_map_scan_sizes(sz)
    if list(sz) != [C.sizeof(IsdfMapScanParams), C.sizeof(IsdfMapScanInfo)]:
        raise RuntimeError(f"isdf_map_scan structs: the library has {list(sz)}, the mirror "
                           f"{[C.sizeof(IsdfMapScanParams), C.sizeof(IsdfMapScanInfo)]}")
    rp, ri = C.POINTER(IsdfMapRaycastParams), C.POINTER(IsdfMapRaycastInfo)
    lib.isdf_map_raycast_params_default.argtypes = [rp]
    lib.isdf_map_raycast_params_default.restype = None
    lib.isdf_map_raycast_sizes.argtypes = [ip]
    lib.isdf_map_raycast_sizes.restype = None
    lib.isdf_map_raycast.argtypes = [C.c_void_p, dp, C.POINTER(C.c_float), C.c_longlong, rp, C.c_void_p, ri]
    lib.isdf_map_raycast_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, rp, C.c_void_p, ri, C.c_void_p]
    lib.isdf_raycast_host.argtypes = [C.c_void_p, dp, dp, C.c_double, C.POINTER(C.c_int32), dp, C.POINTER(C.c_float), C.c_longlong, rp, C.c_void_p]
    lib.isdf_raycast_host.restype = C.c_longlong
    lib.isdf_map_raycast_sizes(sz)
    if list(sz) != [C.sizeof(IsdfMapRaycastParams), C.sizeof(IsdfMapRaycastInfo)]:
        raise RuntimeError(f"isdf_map_raycast structs: the library has {list(sz)}, the mirror "
                           f"{[C.sizeof(IsdfMapRaycastParams), C.sizeof(IsdfMapRaycastInfo)]}")
    cp, qp, qi = C.POINTER(IsdfDepthCamera), C.POINTER(IsdfDepthRenderParams), C.POINTER(IsdfDepthRenderInfo)
    yp, yi = C.POINTER(IsdfDepthRaysParams), C.POINTER(IsdfDepthRaysInfo)
    lib.isdf_depth_render_params_default.argtypes = [qp]
    lib.isdf_depth_render_params_default.restype = None
    lib.isdf_depth_render_sizes.argtypes = [ip]
    lib.isdf_depth_render_sizes.restype = None
    lib.isdf_depth_render.argtypes = [C.c_void_p, cp, dp, C.c_void_p, C.c_longlong, qp, C.c_void_p, qi]
    lib.isdf_depth_render_device.argtypes = [C.c_void_p, cp, dp, C.c_void_p, C.c_longlong, qp, C.c_void_p, qi, C.c_void_p]
    lib.isdf_depth_render_host.argtypes = [cp, dp, C.c_void_p, C.c_longlong, C.c_void_p, dp, C.c_double, C.POINTER(C.c_int32), qp, C.c_void_p, qi]
    lib.isdf_depth_rays_params_default.argtypes = [yp]
    lib.isdf_depth_rays_params_default.restype = None
    lib.isdf_depth_rays_sizes.argtypes = [ip]
    lib.isdf_depth_rays_sizes.restype = None
    lib.isdf_depth_rays_rows.argtypes = [cp, yp]
    lib.isdf_depth_rays_rows.restype = C.c_longlong
    lib.isdf_depth_rays.argtypes = [C.c_void_p, cp, dp, C.c_void_p, C.c_int, yp, C.c_void_p, C.c_void_p, yi]
    lib.isdf_depth_rays_device.argtypes = [C.c_void_p, cp, dp, C.c_void_p, C.c_int, yp, C.c_void_p, C.c_void_p, yi, C.c_void_p]
    lib.isdf_depth_rays_host.argtypes = [cp, dp, C.c_void_p, C.c_int, yp, dp, dp, C.c_double, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, yi]
    lib.isdf_depth_rays_host.restype = C.c_longlong
    lib.isdf_integrate_depth.argtypes = [C.c_void_p, cp, dp, C.c_void_p, C.c_int, yp, sp, yi, si]
    sz3 = (C.c_int * 3)()
    lib.isdf_depth_render_sizes(sz3)
    if list(sz3) != [C.sizeof(IsdfDepthCamera), C.sizeof(IsdfDepthRenderParams), C.sizeof(IsdfDepthRenderInfo)]:
        raise RuntimeError(f"isdf_depth_render structs: the library has {list(sz3)}, the mirror "
                           f"{[C.sizeof(IsdfDepthCamera), C.sizeof(IsdfDepthRenderParams), C.sizeof(IsdfDepthRenderInfo)]}")
    lib.isdf_depth_rays_sizes(sz3)
    if list(sz3)[:2] != [C.sizeof(IsdfDepthRaysParams), C.sizeof(IsdfDepthRaysInfo)]:
        raise RuntimeError(f"isdf_depth_rays structs: the library has {list(sz3)[:2]}, the mirror "
                           f"{[C.sizeof(IsdfDepthRaysParams), C.sizeof(IsdfDepthRaysInfo)]}")
    hp, hi, i3 = C.POINTER(IsdfMapShiftParams), C.POINTER(IsdfMapShiftInfo), C.POINTER(C.c_int32)
    lib.isdf_map_shift_params_default.argtypes = [hp]
    lib.isdf_map_shift_params_default.restype = None
    lib.isdf_map_shift_sizes.argtypes = [ip]
    lib.isdf_map_shift_sizes.restype = None
    lib.isdf_shift_map.argtypes = [C.c_void_p, i3, hp, hi]
    lib.isdf_map_follow.argtypes = [C.c_void_p, dp, C.c_int, hp, i3, hi]
    lib.isdf_shift_geometry_host.argtypes = [dp, dp, C.c_double, i3, i3, dp, dp]
    lib.isdf_shift_grid_host.argtypes = [C.c_void_p, C.c_int, i3, i3, C.c_void_p]
    lib.isdf_shift_bands_host.argtypes = [i3, i3, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
    lib.isdf_map_shift_sizes(sz)
    if list(sz) != [C.sizeof(IsdfMapShiftParams), C.sizeof(IsdfMapShiftInfo)]:
        raise RuntimeError(f"isdf_map_shift structs: the library has {list(sz)}, the mirror "
                           f"{[C.sizeof(IsdfMapShiftParams), C.sizeof(IsdfMapShiftInfo)]}")
    ki, fi = C.POINTER(IsdfMapKnownInfo), C.POINTER(IsdfMapFrontierInfo)
    lib.isdf_map_known_sizes.argtypes = [ip]
    lib.isdf_map_known_sizes.restype = None
    lib.isdf_map_known_enable.argtypes = [C.c_void_p, C.c_int]
    lib.isdf_map_known_fill.argtypes = [C.c_void_p, i3, C.c_int]
    lib.isdf_map_known_merge_ms.argtypes = [C.c_void_p, C.c_int, dp]
    lib.isdf_map_known_get.argtypes = [C.c_void_p, C.c_void_p, ki]
    lib.isdf_map_frontier.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, fi]
    lib.isdf_known_merge_host.argtypes = [C.c_void_p, i3, C.c_void_p, C.c_void_p]
    lib.isdf_known_merge_host.restype = C.c_longlong
    lib.isdf_known_shift_host.argtypes = [C.c_void_p, i3, i3, C.c_void_p]
    lib.isdf_known_fill_host.argtypes = [C.c_void_p, i3, i3, C.c_int]
    lib.isdf_known_fill_host.restype = C.c_longlong
    lib.isdf_known_frontier_host.argtypes = [C.c_void_p, C.c_void_p, i3, C.c_void_p, C.c_void_p, C.c_longlong, fi]
    hp2, hi2 = C.POINTER(IsdfTrajKnownParams), C.POINTER(IsdfTrajKnownInfo)
    lib.isdf_traj_known_params_default.argtypes = [hp2]
    lib.isdf_traj_known_params_default.restype = None
    lib.isdf_traj_known_horizon.argtypes = [C.c_void_p, C.c_int, dp, dp, hp2, hi2]
    lib.isdf_traj_known_horizon_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, hp2, hi2, C.c_void_p]
    sz4 = (C.c_int * 4)()
    lib.isdf_map_known_sizes(sz4)
    mirror = [C.sizeof(IsdfMapKnownInfo), C.sizeof(IsdfMapFrontierInfo), C.sizeof(IsdfTrajKnownParams), C.sizeof(IsdfTrajKnownInfo)]
    if list(sz4) != mirror:
        raise RuntimeError(f"isdf_map_known structs: the library has {list(sz4)}, the mirror {mirror}")
    vp, vi = C.POINTER(IsdfViewGainParams), C.POINTER(IsdfViewGainInfo)
    lib.isdf_view_gain_params_default.argtypes = [vp]
    lib.isdf_view_gain_params_default.restype = None
    lib.isdf_view_gain_sizes.argtypes = [ip]
    lib.isdf_view_gain_sizes.restype = None
    lib.isdf_view_gain.argtypes = [C.c_void_p, C.POINTER(IsdfDepthCamera), dp, C.c_longlong, vp, C.c_void_p, vi]
    lib.isdf_view_gain_device.argtypes = [C.c_void_p, C.POINTER(IsdfDepthCamera), C.c_void_p, C.c_longlong, vp, C.c_void_p, vi, C.c_void_p]
    lib.isdf_view_gain_host.argtypes = [C.c_void_p, C.c_void_p, dp, dp, C.c_double, i3, C.POINTER(IsdfDepthCamera), dp, C.c_longlong, vp, C.c_void_p, vi]
    lib.isdf_view_gain_host.restype = C.c_longlong
    lib.isdf_view_gain_sizes(sz)
    if list(sz) != [C.sizeof(IsdfViewGainParams), C.sizeof(IsdfViewGainInfo)]:
        raise RuntimeError(f"isdf_view_gain structs: the library has {list(sz)}, the mirror "
                           f"{[C.sizeof(IsdfViewGainParams), C.sizeof(IsdfViewGainInfo)]}")
    cp, ci = C.POINTER(IsdfFrontierClusterParams), C.POINTER(IsdfFrontierClusterInfo)
    lib.isdf_frontier_cluster_params_default.argtypes = [cp]
    lib.isdf_frontier_cluster_params_default.restype = None
    lib.isdf_frontier_cluster_sizes.argtypes = [ip]
    lib.isdf_frontier_cluster_sizes.restype = None
    lib.isdf_map_frontier_clusters.argtypes = [C.c_void_p, C.c_void_p, cp, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, ci]
    lib.isdf_known_clusters_host.argtypes = [C.c_void_p, i3, cp, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, ci]
    lib.isdf_frontier_cluster_sizes(sz)
    if list(sz) != [C.sizeof(IsdfFrontierClusterParams), C.sizeof(IsdfFrontierClusterInfo)]:
        raise RuntimeError(f"isdf_frontier_cluster structs: the library has {list(sz)}, the mirror "
                           f"{[C.sizeof(IsdfFrontierClusterParams), C.sizeof(IsdfFrontierClusterInfo)]}")
    kp, ki = C.POINTER(IsdfViewCandidatesParams), C.POINTER(IsdfViewCandidatesInfo)
    lib.isdf_view_candidates_params_default.argtypes = [kp]
    lib.isdf_view_candidates_params_default.restype = None
    lib.isdf_view_candidates_sizes.argtypes = [ip]
    lib.isdf_view_candidates_sizes.restype = None
    lib.isdf_view_candidates.argtypes = [C.c_void_p, C.POINTER(IsdfDepthCamera), C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, kp, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, ki]
    lib.isdf_view_candidates_host.argtypes = [C.c_void_p, C.c_void_p, dp, dp, C.c_double, i3, C.POINTER(IsdfDepthCamera), C.c_void_p, C.c_longlong, C.c_void_p,
                                              C.c_longlong, kp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, ki]
    lib.isdf_view_candidates_sizes(sz)
    if list(sz) != [C.sizeof(IsdfViewCandidatesParams), C.sizeof(IsdfViewCandidatesInfo)]:
        raise RuntimeError(f"isdf_view_candidates structs: the library has {list(sz)}, the mirror "
                           f"{[C.sizeof(IsdfViewCandidatesParams), C.sizeof(IsdfViewCandidatesInfo)]}")
    sp, si = C.POINTER(IsdfViewSelectParams), C.POINTER(IsdfViewSelectInfo)
    lib.isdf_view_select_params_default.argtypes = [sp]
    lib.isdf_view_select_params_default.restype = None
    lib.isdf_view_select_sizes.argtypes = [ip]
    lib.isdf_view_select_sizes.restype = None
    lib.isdf_view_select.argtypes = [C.c_void_p, C.POINTER(IsdfDepthCamera), C.c_void_p, C.c_longlong, sp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, si]
    lib.isdf_view_select_host.argtypes = [C.c_void_p, C.c_void_p, dp, dp, C.c_double, i3, C.POINTER(IsdfDepthCamera), C.c_void_p, C.c_longlong, sp, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, si]
    lib.isdf_view_select_sizes(sz)
    if list(sz) != [C.sizeof(IsdfViewSelectParams), C.sizeof(IsdfViewSelectInfo)]:
        raise RuntimeError(f"isdf_view_select structs: the library has {list(sz)}, the mirror "
                           f"{[C.sizeof(IsdfViewSelectParams), C.sizeof(IsdfViewSelectInfo)]}")
    rp, ri = C.POINTER(IsdfViewSelectRoutedParams), C.POINTER(IsdfViewSelectRoutedInfo)
    lib.isdf_view_select_routed_params_default.argtypes = [rp]
    lib.isdf_view_select_routed_params_default.restype = None
    lib.isdf_view_select_routed_sizes.argtypes = [ip]
    lib.isdf_view_select_routed_sizes.restype = None
    lib.isdf_view_select_routed.argtypes = [C.c_void_p, C.POINTER(IsdfDepthCamera), C.c_void_p, C.c_longlong, C.c_void_p, rp, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, ri]
    lib.isdf_view_select_routed_host.argtypes = [C.c_void_p, C.c_void_p, dp, dp, C.c_double, i3, C.POINTER(IsdfDepthCamera), C.c_void_p, C.c_longlong, C.c_void_p, rp,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, ri]
    lib.isdf_view_select_routed_sizes(sz)
    if list(sz) != [C.sizeof(IsdfViewSelectRoutedParams), C.sizeof(IsdfViewSelectRoutedInfo)]:
        raise RuntimeError(f"isdf_view_select_routed structs: the library has {list(sz)}, the mirror "
                           f"{[C.sizeof(IsdfViewSelectRoutedParams), C.sizeof(IsdfViewSelectRoutedInfo)]}")
    ep, ei = C.POINTER(IsdfKnownErodeParams), C.POINTER(IsdfKnownErodeInfo)
    lib.isdf_known_erode_params_default.argtypes = [ep]
    lib.isdf_known_erode_params_default.restype = None
    lib.isdf_known_erode_sizes.argtypes = [ip]
    lib.isdf_known_erode_sizes.restype = None
    lib.isdf_map_known_erode.argtypes = [C.c_void_p, ep, C.c_void_p, ei]
    lib.isdf_known_erode_host.argtypes = [C.c_void_p, i3, C.c_int, C.c_int, C.c_void_p]
    lib.isdf_frontend_field_build_known.argtypes = [C.c_void_p, dp, ep, C.POINTER(IsdfFrontendFieldParams), C.POINTER(IsdfFrontendFieldInfo), ei]
    lib.isdf_frontend_field_known_info.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    lib.isdf_known_erode_sizes(sz)
    if list(sz) != [C.sizeof(IsdfKnownErodeParams), C.sizeof(IsdfKnownErodeInfo)]:
        raise RuntimeError(f"isdf_known_erode structs: the library has {list(sz)}, the mirror "
                           f"{[C.sizeof(IsdfKnownErodeParams), C.sizeof(IsdfKnownErodeInfo)]}")
    lib.isdf_frontend_field_set_known_follow.argtypes = [C.c_void_p, C.c_int]
    lib.isdf_frontend_field_follow_info.argtypes = [C.c_void_p, C.POINTER(IsdfFieldFollowInfo)]
    lib.isdf_frontend_field_follow_sizes.argtypes = [ip]
    lib.isdf_frontend_field_follow_sizes.restype = None
    lib.isdf_frontend_field_follow_sizes(sz)
    if sz[0] != C.sizeof(IsdfFieldFollowInfo):
        raise RuntimeError(f"isdf_field_follow_info: the library has {sz[0]}, the mirror {C.sizeof(IsdfFieldFollowInfo)}")
    lib.isdf_frontend_field_set_repair.argtypes = [C.c_void_p, C.c_int]
    lib.isdf_frontend_field_repair_info.argtypes = [C.c_void_p, C.POINTER(IsdfFieldRepairInfo)]
    lib.isdf_frontend_field_repair_sizes.argtypes = [ip]
    lib.isdf_frontend_field_repair_sizes.restype = None
    lib.isdf_frontend_field_repair_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, dp, C.POINTER(IsdfFieldRepairInfo)]
    lib.isdf_frontend_field_repair_sizes(sz)
    if sz[0] != C.sizeof(IsdfFieldRepairInfo):
        raise RuntimeError(f"isdf_field_repair_info: the library has {sz[0]}, the mirror {C.sizeof(IsdfFieldRepairInfo)}")
    lib.isdf_frontend_field_set_reopen.argtypes = [C.c_void_p, C.c_int]
    lib.isdf_frontend_field_reopen_info.argtypes = [C.c_void_p, C.POINTER(IsdfFieldReopenInfo)]
    lib.isdf_frontend_field_reopen_sizes.argtypes = [ip]
    lib.isdf_frontend_field_reopen_sizes.restype = None
    lib.isdf_frontend_field_reopen_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, dp, C.POINTER(IsdfFieldReopenInfo)]
    lib.isdf_frontend_field_reopen_sizes(sz)
    if sz[0] != C.sizeof(IsdfFieldReopenInfo):
        raise RuntimeError(f"isdf_field_reopen_info: the library has {sz[0]}, the mirror {C.sizeof(IsdfFieldReopenInfo)}")
    lib.isdf_frontend_field_set_shift.argtypes = [C.c_void_p, C.c_int]
    lib.isdf_frontend_field_shift_info.argtypes = [C.c_void_p, C.POINTER(IsdfFieldShiftInfo)]
    lib.isdf_frontend_field_shift_sizes.argtypes = [ip]
    lib.isdf_frontend_field_shift_sizes.restype = None
    lib.isdf_frontend_field_shift_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, dp, C.POINTER(IsdfFieldShiftInfo)]
    lib.isdf_frontend_field_shift_sizes(sz)
    if sz[0] != C.sizeof(IsdfFieldShiftInfo):
        raise RuntimeError(f"isdf_field_shift_info: the library has {sz[0]}, the mirror {C.sizeof(IsdfFieldShiftInfo)}")
    if path is None:
        _lib = lib
    return lib
