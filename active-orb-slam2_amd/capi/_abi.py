"""The C ABI of include/aos2.h restated for ctypes: constants, record dtypes, structures and the prototype of every function.

Declarations only: nothing here loads the library or touches an array.  tests/test_capi_layout_cpu.py compiles a C program against
the header and compares every size, field offset, constant and prototype with this file, so a declaration that drifts fails there.
A structure names its C type in `_c_name_`; a Python field name equals the C one except `lam` for `lambda`.
"""
import ctypes as C

import numpy as np

# ---- status and mode constants
CONSTANTS = {}   # C macro -> the value mirrored here


def _mirror(prefix, names, values=None):
    """the values (default 0, 1, ..) of the macros prefix + name, noted in CONSTANTS for the layout test"""
    values = tuple(range(len(names))) if values is None else values
    CONSTANTS.update({prefix + n: v for n, v in zip(names, values)})
    return values


AOS2_OK, AOS2_ERR_ARG, AOS2_ERR_CAPACITY, AOS2_ERR_TOO_SMALL, AOS2_ERR_HIP, AOS2_ERR_NO_DEVICE, AOS2_ERR_STOPPED = _mirror(
    "AOS2_", ("OK", "ERR_ARG", "ERR_CAPACITY", "ERR_TOO_SMALL", "ERR_HIP", "ERR_NO_DEVICE", "ERR_STOPPED"), (0, -1, -2, -3, -4, -5, 1))
AOS2_INIT_OK, AOS2_INIT_NO_MODEL = _mirror("AOS2_INIT_", ("OK", "NO_MODEL"))
AOS2_EG_OK, AOS2_EG_NO_STEP, AOS2_ERR_EG_MEMORY = _mirror("AOS2_", ("EG_OK", "EG_NO_STEP", "ERR_EG_MEMORY"), (0, 1, -6))
KFC_KEPT, KFC_CULLED, KFC_DEFERRED, KFC_SKIPPED = _mirror("AOS2_KFC_", ("KEPT", "CULLED", "DEFERRED", "SKIPPED"))
(CONNECTIONS_TH,) = _mirror("AOS2_", ("CONNECTIONS_TH",), (15,))
ND_UPDATED, ND_BAD, ND_NO_OBS, ND_UNKNOWN, ND_REF_UNUSABLE = _mirror("AOS2_ND_", ("UPDATED", "BAD", "NO_OBS", "UNKNOWN", "REF_UNUSABLE"))
ND_ROWS_PLANNING, ND_ROWS_TRACKING = _mirror("AOS2_ND_ROWS_", ("PLANNING", "TRACKING"))
TRI_NO_MATCH, TRI_ACCEPTED, TRI_LOW_PARALLAX, TRI_W_ZERO, TRI_DEPTH1, TRI_DEPTH2, TRI_REPROJ1, TRI_REPROJ2, TRI_ZERO_DIST, TRI_SCALE, \
    TRI_SUPERSEDED = _mirror("AOS2_TRI_", ("NO_MATCH", "ACCEPTED", "LOW_PARALLAX", "W_ZERO", "DEPTH1", "DEPTH2", "REPROJ1", "REPROJ2",
                                           "ZERO_DIST", "SCALE", "SUPERSEDED"))
SIM3_OPT_LINEARISE, SIM3_OPT_TRIAL, SIM3_OPT_REJECT = _mirror("AOS2_SIM3_OPT_STEP_", ("LINEARISE", "TRIAL", "REJECT"), (1, 2, 4))
# class constants of the wrappers: KeyFrameDatabase.LOOP .., Visibility.CAMERA_MAP .., Matcher.TH_LOW .., Frames.MAP_POINTS ..
KFDB_MODES = _mirror("AOS2_KFDB_", ("LOOP", "RELOC"))
VIS_CAMERAS = _mirror("AOS2_VIS_CAMERA_", ("MAP", "PLAIN"))
MATCHER_THRESHOLDS = _mirror("AOS2_", ("TH_LOW", "TH_HIGH", "HISTO_LENGTH"), (50, 100, 30))
FRAMES_MEMBERS = _mirror("AOS2_FRAMES_", ("MAP_POINTS", "OUTLIER", "TCW", "U_RIGHT", "DEPTH", "GRID_OFF", "GRID_IDX", "KEYS_UN_X", "KEYS_UN_Y",
                                          "KEYS_ANGLE", "KEYS_OCTAVE"))
HIP_D2H, HIP_H2D = 2, 1   # hipMemcpyKind of the HIP runtime (not part of aos2.h)

# ---- records passed as numpy arrays: C type -> dtype
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
# aos2_triang_obs_t: mvKeysUn[i].pt, mvKeys[i].pt, mvuRight[i], mvDepth[i], mvKeysUn[i].octave
TRIANG_OBS = np.dtype([("ux", "<f4"), ("uy", "<f4"), ("kx", "<f4"), ("ky", "<f4"), ("u_right", "<f4"), ("depth", "<f4"), ("octave", "<i4")])
RECORD_DTYPES = {"aos2_keypoint_t": KP_DTYPE, "aos2_triang_obs_t": TRIANG_OBS}


# ---- structures, in the header's order of sections
def _struct(c_name, fields):
    """a ctypes.Structure that mirrors the C type `c_name` (None: a type that is not in the header)"""
    return type(c_name or "aos2_call_t", (C.Structure,), {"_c_name_": c_name, "_fields_": fields})


# aos2_call_t of csrc/host_runner.cpp (the recording harness; not part of aos2.h)
_Call = _struct(None,
    [("fn", C.c_void_p), ("n_int", C.c_int32), ("n_fp", C.c_int32), ("iargs", C.c_int64 * 24), ("fargs", C.c_uint64 * 8)])

_KfdbQuery = _struct("aos2_kfdb_query_t",
    [("mode", C.c_int32), ("slot", C.c_int32), ("words", C.c_void_p), ("values", C.c_void_p), ("n_words", C.c_int32),
    ("on_device", C.c_int32), ("min_score", C.c_float), ("n_excluded", C.c_int32), ("excluded", C.c_void_p)])

_KfdbResult = _struct("aos2_kfdb_result_t",
    [("candidates", C.c_void_p), ("cap_candidates", C.c_int32)] +
    [(k, C.c_int32) for k in ("n_candidates", "n_sharing", "max_common_words", "min_common_words", "n_scored", "n_matched")] +
    [("best_acc_score", C.c_float), ("scored_slot", C.c_void_p), ("scored_words", C.c_void_p), ("scored_score", C.c_void_p),
    ("cap_scored", C.c_int32), ("sharing_slot", C.c_void_p), ("sharing_words", C.c_void_p), ("cap_sharing", C.c_int32)])

VisCamera = _struct("aos2_vis_camera_t",
    [(k, C.c_float) for k in ("fx", "fy", "cx", "cy", "min_x", "max_x", "min_y", "max_y", "max_dist", "min_dist")] +
    [("feature_threshold", C.c_int32), ("T_sw", C.c_float * 16), ("T_bc", C.c_float * 16)])

SvcParams = _struct("aos2_svc_params_t",
    [(k, C.c_double) for k in ("turn_radius", "robot_r", "dt", "min_x", "max_x", "min_y", "max_y", "max_dist_heuristic")] +
    [("start", C.c_double * 3), ("heuristic", C.c_int32), ("feature_threshold", C.c_int32)])

_SvcMotionsOut = _struct("aos2_svc_motions_out_t",
    [(k, C.c_void_p) for k in ("path_valid", "type", "t", "m", "n_states", "valid", "first_invalid", "cost_length",
    "cost_camera", "offsets", "states")] +
    [("states_capacity", C.c_int64), ("states_needed", C.c_int64)])

_BowPair = _struct("aos2_bow_pair_t",
    [("n_kf", C.c_int32), ("n_f", C.c_int32), ("desc_kf", C.c_void_p), ("desc_f", C.c_void_p),
    ("kf_has_mp", C.c_void_p), ("angle_kf", C.c_void_p), ("angle_f", C.c_void_p),
    ("n_nodes_kf", C.c_int32), ("n_nodes_f", C.c_int32),
    ("node_id_kf", C.c_void_p), ("node_off_kf", C.c_void_p), ("node_idx_kf", C.c_void_p),
    ("node_id_f", C.c_void_p), ("node_off_f", C.c_void_p), ("node_idx_f", C.c_void_p)])

_BowFrames = _struct("aos2_bow_frames_t",
    [("n_frames", C.c_int32), ("cap", C.c_int32)] + [(k, C.c_void_p) for k in (
    "d_desc_kf", "d_kps_kf", "d_n_kf", "d_desc_f", "d_kps_f", "d_n_f", "kf_has_mp", "d_kf_fv_node", "d_kf_fv_off", "d_kf_fv_idx",
    "d_kf_n_fv", "d_f_fv_node", "d_f_fv_off", "d_f_fv_idx", "d_f_n_fv")])

_BowKfPair = _struct("aos2_bow_kf_pair_t",
    [("n1", C.c_int32), ("n2", C.c_int32), ("desc1", C.c_void_p), ("desc2", C.c_void_p),
    ("has_mp1", C.c_void_p), ("has_mp2", C.c_void_p), ("angle1", C.c_void_p), ("angle2", C.c_void_p),
    ("n_nodes1", C.c_int32), ("n_nodes2", C.c_int32),
    ("node_id1", C.c_void_p), ("node_off1", C.c_void_p), ("node_idx1", C.c_void_p),
    ("node_id2", C.c_void_p), ("node_off2", C.c_void_p), ("node_idx2", C.c_void_p)])

_TriangPair = _struct("aos2_triang_pair_t",
    [("n1", C.c_int32), ("n2", C.c_int32), ("desc1", C.c_void_p), ("desc2", C.c_void_p),
    ("has_mp1", C.c_void_p), ("has_mp2", C.c_void_p),
    ("x1", C.c_void_p), ("y1", C.c_void_p), ("angle1", C.c_void_p), ("u_right1", C.c_void_p),
    ("x2", C.c_void_p), ("y2", C.c_void_p), ("angle2", C.c_void_p), ("u_right2", C.c_void_p),
    ("octave2", C.c_void_p), ("scale_factors2", C.c_void_p), ("level_sigma2_2", C.c_void_p),
    ("n_levels2", C.c_int32), ("F12", C.c_float * 9), ("ex", C.c_float), ("ey", C.c_float),
    ("n_nodes1", C.c_int32), ("n_nodes2", C.c_int32),
    ("node_id1", C.c_void_p), ("node_off1", C.c_void_p), ("node_idx1", C.c_void_p),
    ("node_id2", C.c_void_p), ("node_off2", C.c_void_p), ("node_idx2", C.c_void_p)])

_FrameView = _struct("aos2_frame_view_t",
    [("n_f", C.c_int32), ("desc_f", C.c_void_p), ("kp_x", C.c_void_p), ("kp_y", C.c_void_p),
    ("kp_octave", C.c_void_p), ("kp_angle", C.c_void_p), ("u_right", C.c_void_p),
    ("scale_factors", C.c_void_p), ("n_levels", C.c_int32),
    ("min_x", C.c_float), ("min_y", C.c_float), ("max_x", C.c_float), ("max_y", C.c_float),
    ("grid_w_inv", C.c_float), ("grid_h_inv", C.c_float),
    ("grid_off", C.c_void_p), ("grid_idx", C.c_void_p), ("f_mp_state", C.c_void_p)])

_ProjMp = _struct("aos2_proj_mp_t",
    [("n_mp", C.c_int32), ("track_in_view", C.c_void_p), ("pred_level", C.c_void_p),
    ("view_cos", C.c_void_p), ("proj_x", C.c_void_p), ("proj_y", C.c_void_p),
    ("proj_xr", C.c_void_p), ("desc", C.c_void_p), ("has_obs", C.c_void_p)])

_ProjLast = _struct("aos2_proj_last_t",
    [("n_last", C.c_int32), ("last_valid", C.c_void_p), ("world_pos", C.c_void_p),
    ("desc", C.c_void_p), ("last_octave", C.c_void_p), ("last_angle", C.c_void_p),
    ("has_obs", C.c_void_p), ("Tcw", C.c_float * 16), ("Tlw", C.c_float * 16),
    ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
    ("mb", C.c_float), ("mbf", C.c_float)])

_ProjPoints = _struct("aos2_proj_points_t",
    [("n_pts", C.c_int32), ("valid", C.c_void_p), ("pos", C.c_void_p), ("max_dist", C.c_void_p),
    ("min_dist", C.c_void_p), ("normal", C.c_void_p), ("desc", C.c_void_p), ("q_angle", C.c_void_p),
    ("R", C.c_float * 9), ("t", C.c_float * 3), ("Ow", C.c_float * 3), ("R2", C.c_float * 9),
    ("t2", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
    ("bf", C.c_float), ("log_scale_factor", C.c_float), ("inv_level_sigma2", C.c_void_p), ("th", C.c_float)])

_Sim3Problem = _struct("aos2_sim3_problem_t",
    [("n", C.c_int32), ("X3Dc1", C.c_void_p), ("X3Dc2", C.c_void_p), ("max_err1", C.c_void_p), ("max_err2", C.c_void_p)] +
    [(k, C.c_float) for k in ("fx1", "fy1", "cx1", "cy1", "fx2", "fy2", "cx2", "cy2")] +
    [("fix_scale", C.c_int32), ("probability", C.c_double), ("min_inliers", C.c_int32), ("max_iterations", C.c_int32),
    ("draws", C.c_void_p)])

_Sim3Result = _struct("aos2_sim3_result_t",
    [("ransac_max_its", C.c_int32), ("first_success", C.c_int32), ("best_iteration", C.c_int32), ("best_inliers", C.c_int32),
    ("T12", C.c_float * 16), ("R12", C.c_float * 9), ("t12", C.c_float * 3), ("s12", C.c_float),
    ("inliers", C.c_void_p), ("counts", C.c_void_p)])

_PnpProblem = _struct("aos2_pnp_problem_t",
    [("n", C.c_int32), ("P3Dw", C.c_void_p), ("P2D", C.c_void_p), ("max_err", C.c_void_p)] +
    [(k, C.c_float) for k in ("fx", "fy", "cx", "cy")] +
    [("min_inliers", C.c_int32), ("min_set", C.c_int32), ("first_iteration", C.c_int32), ("n_iterations", C.c_int32),
    ("draws", C.c_void_p), ("best_inliers_in", C.c_int32), ("best_in", C.c_void_p)])

_PnpResult = _struct("aos2_pnp_result_t",
    [("returned_at", C.c_int32), ("Tcw", C.c_float * 16), ("n_inliers", C.c_int32), ("inliers", C.c_void_p),
    ("best_iteration", C.c_int32), ("best_inliers", C.c_int32), ("best_Tcw", C.c_float * 16), ("best", C.c_void_p),
    ("counts", C.c_void_p)])

_InitProblem = _struct("aos2_initializer_problem_t",
    [("n_keys1", C.c_int32), ("n_keys2", C.c_int32), ("keys1", C.c_void_p), ("keys2", C.c_void_p), ("n_matches", C.c_int32),
    ("matches", C.c_void_p), ("sigma", C.c_float), ("iterations", C.c_int32), ("sets", C.c_void_p)] +
    [(k, C.c_float) for k in ("fx", "fy", "cx", "cy", "min_parallax")] + [("min_triangulated", C.c_int32)])

_InitResult = _struct("aos2_initializer_result_t",
    [("status", C.c_int32), ("initialized", C.c_int32), ("used_homography", C.c_int32), ("SH", C.c_float), ("SF", C.c_float),
    ("H21", C.c_float * 9), ("F21", C.c_float * 9), ("best_iteration_h", C.c_int32), ("best_iteration_f", C.c_int32),
    ("inliers_h", C.c_void_p), ("inliers_f", C.c_void_p), ("R21", C.c_float * 9), ("t21", C.c_float * 3), ("P3D", C.c_void_p),
    ("triangulated", C.c_void_p), ("n_good", C.c_int32 * 8), ("parallax", C.c_float * 8), ("n_hypotheses", C.c_int32)])

_LbaProblem = _struct("aos2_lba_problem_t",
    [("n_poses", C.c_int32), ("n_points", C.c_int32), ("n_edges", C.c_int32),
    ("pose_Tcw", C.c_void_p), ("pose_fixed", C.c_void_p), ("pose_id", C.c_void_p),
    ("point_xyz", C.c_void_p), ("point_id", C.c_void_p), ("edge_pose", C.c_void_p),
    ("edge_point", C.c_void_p), ("edge_obs", C.c_void_p), ("edge_stereo", C.c_void_p),
    ("edge_inv_sigma2", C.c_void_p),
    ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("bf", C.c_float),
    ("stop_flag", C.c_void_p), ("iters_first", C.c_int32), ("iters_second", C.c_int32)])

_LbaResult = _struct("aos2_lba_result_t",
    [("pose_Tcw", C.c_void_p), ("point_xyz", C.c_void_p), ("edge_outlier", C.c_void_p),
    ("edge_chi2", C.c_void_p), ("iters_done_first", C.c_int32), ("iters_done_second", C.c_int32),
    ("final_chi2", C.c_double), ("final_lambda", C.c_double), ("ms_device", C.c_float),
    ("status", C.c_int32), ("trials_first", C.c_int32), ("trials_second", C.c_int32),
    ("polls", C.c_int32), ("stop_poll", C.c_int32)])

_GbaOptions = _struct("aos2_gba_options_t",
    [("iterations", C.c_int32), ("robust", C.c_int32), ("huber_mono", C.c_float), ("huber_stereo", C.c_float)])

_GbaResult = _struct("aos2_gba_result_t",
    [("pose_Tcw", C.c_void_p), ("point_xyz", C.c_void_p), ("point_included", C.c_void_p),
    ("iterations", C.c_int32), ("trials", C.c_int32), ("chi2_initial", C.c_double), ("chi2_final", C.c_double),
    ("final_lambda", C.c_double), ("polls", C.c_int32), ("stop_poll", C.c_int32), ("h_blocks", C.c_int32),
    ("l_blocks", C.c_int32), ("ms_device", C.c_float), ("status", C.c_int32)])

_PoseProblem = _struct("aos2_pose_problem_t",
    [("n", C.c_int32), ("Xw", C.c_void_p), ("obs", C.c_void_p), ("stereo", C.c_void_p),
    ("inv_sigma2", C.c_void_p), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
    ("cy", C.c_float), ("bf", C.c_float), ("Tcw", C.c_float * 16)])

_PoseResult = _struct("aos2_pose_result_t",
    [("Tcw", C.c_float * 16), ("outlier", C.c_void_p), ("n_bad", C.c_int32), ("n_inliers", C.c_int32)])

_Sim3OptProblem = _struct("aos2_sim3_opt_problem_t",
    [("n", C.c_int32)] + [(k, C.c_void_p) for k in ("X1c", "X2c", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2")] +
    [(k, C.c_float) for k in ("fx1", "fy1", "cx1", "cy1", "fx2", "fy2", "cx2", "cy2")] +
    [("q12", C.c_double * 4), ("t12", C.c_double * 3), ("s12", C.c_double), ("th2", C.c_float), ("fix_scale", C.c_int32)])

_Sim3OptResult = _struct("aos2_sim3_opt_result_t",
    [("q12", C.c_double * 4), ("t12", C.c_double * 3), ("s12", C.c_double), ("outlier", C.c_void_p),
    ("n_bad", C.c_int32), ("n_inliers", C.c_int32), ("iterations", C.c_int32 * 2), ("trials", C.c_int32 * 2)])

_EssentialGraphProblem = _struct("aos2_essential_graph_problem_t",
    [("n_vertices", C.c_int32), ("Scw", C.c_void_p), ("fixed", C.c_int32), ("n_edges", C.c_int32), ("v0", C.c_void_p),
    ("v1", C.c_void_p), ("Sji", C.c_void_p), ("fix_scale", C.c_int32), ("iterations", C.c_int32), ("n_points", C.c_int32),
    ("Xw", C.c_void_p), ("ref", C.c_void_p)])

_EssentialGraphResult = _struct("aos2_essential_graph_result_t",
    [("Scw", C.c_void_p), ("Tiw", C.c_void_p), ("Xw", C.c_void_p), ("chi2_initial", C.c_double), ("chi2_final", C.c_double),
    ("iterations", C.c_int32), ("trials", C.c_int32), ("rejected", C.c_int32), ("l_blocks", C.c_int32), ("status", C.c_int32)])

_MapPointsDev = _struct("aos2_map_points_dev_t",
    [("n", C.c_int32), ("pos", C.c_void_p), ("desc", C.c_void_p), ("has_obs", C.c_void_p),
    ("normal", C.c_void_p), ("min_dist", C.c_void_p), ("max_dist", C.c_void_p)])

_FramesTriang = _struct("aos2_frames_triang_t",
    [("n_pairs", C.c_int32)] + [(k, C.c_void_p) for k in ("kf1", "kf2", "F12", "epipole", "d_node_of1", "d_fv_node1", "d_fv_off1",
    "d_fv_idx1", "d_n_fv1", "d_fv_node2", "d_fv_off2", "d_fv_idx2", "d_n_fv2")])

_TriangGeom = _struct("aos2_triang_geom_t",
    [("Tcw1", C.c_float * 16), ("Tcw2", C.c_float * 16)] +
    [(k, C.c_float) for k in ("fx1", "fy1", "cx1", "cy1", "mb1", "mbf1", "fx2", "fy2", "cx2", "cy2", "mb2", "mbf2")] +
    [("n_levels", C.c_int32), ("scale_factors1", C.c_float * 8), ("scale_factors2", C.c_float * 8)])

_LocalMapGraph = _struct("aos2_local_map_graph_t",
    [("n_points", C.c_int32), ("point_bad", C.c_void_p), ("point_nobs", C.c_void_p), ("obs_off", C.c_void_p),
    ("obs_kf", C.c_void_p), ("n_keyframes", C.c_int32), ("kf_bad", C.c_void_p), ("kf_mp_off", C.c_void_p),
    ("kf_mp", C.c_void_p), ("kf_best", C.c_void_p), ("kf_child_off", C.c_void_p), ("kf_child", C.c_void_p),
    ("kf_parent", C.c_void_p)])


# the arrays of a culling view: field -> dtype
_KFC_FIELDS = (("obs_idx", np.int32), ("kf_octave", np.int8), ("kf_depth", np.float32), ("kf_stereo", np.uint8),
               ("kf_th_depth", np.float32), ("kf_flags", np.uint8))


_KfCullingView = _struct("aos2_kf_culling_view_t",
    [(k, C.c_void_p) for k, _ in _KFC_FIELDS])

_LocalMapDelta = _struct("aos2_local_map_delta_t",
    [("n_points", C.c_int32), ("n_keyframes", C.c_int32),
    ("n_point_rows", C.c_int32), ("point_row", C.c_void_p), ("point_bad", C.c_void_p), ("point_nobs", C.c_void_p),
    ("obs_off", C.c_void_p), ("obs_kf", C.c_void_p),
    ("n_kf_mp_rows", C.c_int32), ("kf_mp_row", C.c_void_p), ("kf_mp_off", C.c_void_p), ("kf_mp", C.c_void_p),
    ("n_kf_link_rows", C.c_int32), ("kf_link_row", C.c_void_p), ("kf_bad", C.c_void_p), ("kf_best", C.c_void_p),
    ("kf_child_off", C.c_void_p), ("kf_child", C.c_void_p), ("kf_parent", C.c_void_p), ("view", C.c_void_p)])

# the arrays of an aos2_normal_depth_t: field -> (dtype, elements per listed point; None: per observation slot)
_ND_INPUTS = (("point", np.int32), ("xyz", np.float32), ("ref_kf", np.int32), ("kf_center", np.float32), ("scale", np.float32),
              ("term_off", np.int32))
_ND_OUTPUTS = (("status", np.uint8, 1), ("normal", np.float32, 3), ("min_dist", np.float32, 1), ("max_dist", np.float32, 1),
               ("theta_mean", np.float32, 1), ("theta_std", np.float32, 1), ("n_terms", np.int32, 1), ("upper", np.float32, 1),
               ("lower", np.float32, 1), ("max_range", np.float32, 1), ("min_range", np.float32, 1), ("term_unit", np.float32, None),
               ("term_theta", np.float32, None))

_NormalDepth = _struct("aos2_normal_depth_t",
    [("n", C.c_int32), ("point", C.c_void_p), ("xyz", C.c_void_p), ("ref_kf", C.c_void_p), ("kf_center", C.c_void_p),
    ("n_levels", C.c_int32), ("scale", C.c_void_p), ("rows_form", C.c_int32), ("term_off", C.c_void_p)] +
    [(k, C.c_void_p) for k, _, _ in _ND_OUTPUTS])

_Sim3OptSteps = _struct("aos2_sim3_opt_steps_t",
    [("problem", _Sim3OptProblem), ("S_lin", C.c_double * 8), ("S_trial", C.c_double * 8)] +
    [(k, C.c_void_p) for k in ("act_in", "chi_in", "outlier_in")] + [(k, C.c_int32) for k in ("tail", "remove", "mask", "pad")] +
    [(k, C.c_void_p) for k in ("Hb", "pert", "chi_lin", "trial_sum", "chi_trial", "flagged", "chi", "act", "outlier")])

_PosePassCase = _struct("aos2_pose_pass_case_t",
    [("n", C.c_int32), ("form", C.c_int32), ("it", C.c_int32), ("Xw", C.c_void_p), ("obs", C.c_void_p), ("inv_sigma2", C.c_void_p),
    ("stereo", C.c_void_p), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("bf", C.c_float),
    ("pose", C.c_double * 7), ("level1", C.c_void_p), ("robust", C.c_void_p), ("outlier", C.c_void_p), ("chi2", C.c_void_p),
    ("sums", C.c_double * 28), ("pose_out", C.c_double * 7), ("Tcw", C.c_float * 16), ("n_bad", C.c_int32), ("n_inliers", C.c_int32)])

_LbaSystem = _struct("aos2_lba_system_t",
    [("np", C.c_int32), ("nl", C.c_int32), ("npad", C.c_int32), ("phase", C.c_int32), ("trials_first", C.c_int32),
    ("iters_done_first", C.c_int32), ("n_units", C.c_int32), ("lam", C.c_double), ("current_chi", C.c_double),
    ("hpose", C.c_void_p), ("hpoint", C.c_void_p), ("blk_off", C.c_void_p), ("units", C.c_void_p), ("pose", C.c_void_p),
    ("point", C.c_void_p), ("e_level1", C.c_void_p), ("e_robust", C.c_void_p), ("Hpp_init", C.c_void_p), ("b_init", C.c_void_p),
    ("b_p", C.c_void_p), ("Hll", C.c_void_p), ("b_l", C.c_void_p), ("Hs", C.c_void_p), ("bs", C.c_void_p)])

_LbaLmState = _struct("aos2_lba_lm_state_t",
    [(k, C.c_double) for k in ("lam", "ni", "currentChi", "iniChi", "final_chi2", "final_lambda")] +
    [(k, C.c_int32) for k in ("phase", "run", "lin", "initp", "xmark", "it", "qmax", "nBad")] +
    [("iters_done", C.c_int32 * 2), ("trials", C.c_int32 * 2)] +
    [(k, C.c_int32) for k in ("polls", "stop_poll", "n_active", "solver_failed", "err_at", "ntr")] +
    [(k, C.c_double * 48) for k in ("tr_rho", "tr_temp", "tr_cur", "tr_lambda")])


# arrays of a snapshot of aos2_debug_lba_trial_device: name -> (dtype, size from n_poses, n_points, n_edges)
_LBA_SNAP_ARRAYS = (("est", np.float64, lambda q, m, E: 7 * q + 3 * m), ("bk", np.float64, lambda q, m, E: 7 * q + 3 * m),
                    ("x", np.float64, lambda q, m, E: 6 * q + 3 * m), ("b", np.float64, lambda q, m, E: 6 * q + 3 * m),
                    ("Hll", np.float64, lambda q, m, E: 9 * m), ("Rl", np.float64, lambda q, m, E: 9 * q),
                    ("tmp", np.float64, lambda q, m, E: 6 * q), ("part", np.float64, lambda q, m, E: 2 * m),
                    ("e_level1", np.uint8, lambda q, m, E: E), ("e_robust", np.uint8, lambda q, m, E: E),
                    ("err", np.float64, lambda q, m, E: 3 * E), ("lrec", np.float64, lambda q, m, E: 4 * E),
                    ("erec_flags", np.uint32, lambda q, m, E: E), ("out_Tcw", np.float32, lambda q, m, E: 16 * q),
                    ("out_xyz", np.float32, lambda q, m, E: 3 * m), ("out_chi2", np.float64, lambda q, m, E: E),
                    ("out_outlier", np.uint8, lambda q, m, E: E))


_LbaTrialSnap = _struct("aos2_lba_trial_snap_t",
    [("taken", C.c_int32), ("pad_", C.c_int32), ("st", _LbaLmState), ("scal3", C.c_double)] +
    [(k, C.c_void_p) for k, _, _ in _LBA_SNAP_ARRAYS])

_LbaTrial = _struct("aos2_lba_trial_t",
    [("np", C.c_int32), ("nl", C.c_int32), ("n_pl", C.c_int32), ("n_part", C.c_int32), ("hpose", C.c_void_p), ("hpoint", C.c_void_p),
    ("pt_off", C.c_void_p), ("pt_k", C.c_void_p), ("pl_pos", C.c_void_p), ("snap", _LbaTrialSnap * 5)])


STRUCTS = [v for v in list(globals().values()) if isinstance(v, type) and issubclass(v, C.Structure) and getattr(v, "_c_name_", None)]
RENAMED_FIELDS = {"lam": "lambda"}   # Python field -> C field


# ---- prototypes: function -> (restype, argtypes), in the header's order.  An int-returning function returns an AOS2_* status or a count
vp, ci, cf, cd, sz, i32, i64, cs = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_size_t, C.c_int32, C.c_int64, C.c_char_p
pvp, pci, pcf, pi32 = C.POINTER(vp), C.POINTER(ci), C.POINTER(cf), C.POINTER(i32)


def _same(signature, *names):
    """functions that share one signature"""
    return {n: signature for n in names}


PROTOTYPES = {
    "aos2_last_error": (cs, []),
    "aos2_device_count": (ci, []),
    "aos2_version": (cs, []),
    "aos2_device_local_cpus": (ci, [ci, cs, ci]),
    # ORBextractor
    "aos2_extractor_create": (ci, [ci, cf, ci, ci, ci, ci, pvp]),
    "aos2_extractor_destroy": (None, [vp]),
    "aos2_extractor_levels": (ci, [vp]),
    "aos2_extractor_scale_factor": (cf, [vp]),
    **_same((pcf, [vp]), "aos2_extractor_scale_factors", "aos2_extractor_inv_scale_factors", "aos2_extractor_sigma2",
            "aos2_extractor_inv_sigma2"),
    **_same((pci, [vp]), "aos2_extractor_features_per_level", "aos2_extractor_umax"),
    "aos2_extractor_extract": (ci, [vp, vp, ci, ci, ci, vp, vp, ci, pci]),
    "aos2_extractor_max_keypoints": (ci, [vp]),
    "aos2_extractor_max_keypoints_for": (ci, [vp, ci, ci]),
    **_same((ci, [vp, vp, ci, ci, ci, ci, sz, vp, vp, ci, vp]), "aos2_extractor_extract_batch", "aos2_extractor_extract_batch_device",
            "aos2_extractor_extract_batch_device_async"),
    "aos2_host_alloc": (ci, [pvp, sz]),
    "aos2_host_free": (ci, [vp]),
    "aos2_extractor_wait": (ci, [vp]),
    "aos2_extractor_stream_wait": (ci, [vp, vp]),
    "aos2_extractor_wait_for_stream": (ci, [vp, vp]),
    "aos2_extractor_pack_slots": (ci, [vp, ci, vp, vp, vp, ci, vp, sz, vp]),
    "aos2_extractor_pyramid_level_size": (ci, [vp, ci, pci, pci]),
    "aos2_extractor_pyramid_level": (ci, [vp, ci, ci, ci, vp, ci]),
    "aos2_compute_stereo_matches": (ci, [vp, vp, ci, vp, vp, ci, vp, vp, ci, cf, cf, vp, vp]),
    **_same((ci, [vp, vp, ci, vp, vp, vp, vp, vp, vp, ci, cf, cf, vp, vp]), "aos2_compute_stereo_matches_device",
            "aos2_compute_stereo_matches_device_async"),
    "aos2_compute_stereo_matches_last_device_ms": (cf, [vp]),
    "aos2_extractor_debug_candidates": (ci, [vp, ci, ci, vp, vp, vp, ci, pci]),
    "aos2_extractor_last_timing": (ci, [vp, vp, ci]),
    "aos2_extractor_set_chunks": (ci, [vp, ci]),
    "aos2_extractor_bench_fast": (ci, [vp, ci, pcf]),
    "aos2_extractor_bench_describe": (ci, [vp, ci, pcf]),
    # ORBVocabulary
    "aos2_vocabulary_create": (ci, [ci, pvp]),
    "aos2_vocabulary_destroy": (None, [vp]),
    **_same((ci, [vp, cs]), "aos2_vocabulary_load_binary", "aos2_vocabulary_load_text", "aos2_vocabulary_save_binary"),
    "aos2_vocabulary_set_nodes": (ci, [vp, ci, ci, ci, ci, ci, vp, vp, vp, vp]),
    **_same((ci, [vp]), "aos2_vocabulary_k", "aos2_vocabulary_levels", "aos2_vocabulary_scoring", "aos2_vocabulary_weighting",
            "aos2_vocabulary_nodes", "aos2_vocabulary_empty"),
    "aos2_vocabulary_size": (C.c_uint, [vp]),
    "aos2_vocabulary_get_nodes": (ci, [vp] * 6),
    "aos2_vocabulary_transform": (ci, [vp, vp, ci, ci, vp, vp, pci, vp, vp, vp, pci, vp, vp]),
    "aos2_vocabulary_transform_device": (ci, [vp, ci, vp, vp, ci, ci] + [vp] * 9),
    "aos2_vocabulary_last_device_ms": (cf, [vp]),
    "aos2_vocabulary_stream": (vp, [vp]),
    "aos2_vocabulary_score": (ci, [vp, vp, vp, ci, vp, vp, ci, C.POINTER(cd)]),
    # KeyFrameDatabase
    "aos2_kfdb_create": (ci, [vp, ci, pvp]),
    "aos2_kfdb_destroy": (None, [vp]),
    "aos2_kfdb_put": (ci, [vp, vp, vp, ci, pi32]),
    "aos2_kfdb_put_device": (ci, [vp, vp, ci, vp, vp, vp, ci, vp]),
    **_same((ci, [vp, i32]), "aos2_kfdb_add", "aos2_kfdb_erase", "aos2_kfdb_drop"),
    "aos2_kfdb_clear": (ci, [vp]),
    "aos2_kfdb_size": (ci, [vp]),
    "aos2_kfdb_arena_capacity": (i64, [vp]),
    "aos2_kfdb_set_neighbours": (ci, [vp, ci, vp, vp]),
    "aos2_kfdb_last_device_ms": (cf, [vp]),
    **_same((ci, [vp, vp, vp, ci]), "aos2_kfdb_detect", "aos2_debug_kfdb_host"),
    **_same((ci, [vp, vp, vp, ci, vp, pcf]), "aos2_kfdb_scores", "aos2_debug_kfdb_scores_host"),
    # planner: visibility and motion checks
    "aos2_vis_camera_default": (ci, [ci, vp]),
    "aos2_vis_create": (ci, [ci, pvp]),
    "aos2_vis_destroy": (None, [vp]),
    "aos2_vis_set_camera": (ci, [vp, vp]),
    "aos2_vis_set_map": (ci, [vp, ci] + [vp] * 6),
    "aos2_vis_map_size": (ci, [vp]),
    "aos2_vis_gate_tile": (None, [pci, pci]),
    "aos2_vis_last_device_ms": (cf, [vp]),
    **_same((ci, [vp, ci, vp, vp, vp, vp]), "aos2_vis_count", "aos2_vis_count_poses", "aos2_debug_visibility_host",
            "aos2_debug_visibility_poses_host", "aos2_svc_valid", "aos2_debug_svc_valid_host"),
    **_same((ci, [vp, ci, vp, vp, ci, vp]), "aos2_vis_motion_costs", "aos2_debug_visibility_motion_costs_host"),
    **_same((ci, [vp, ci, vp, ci, pi32]), "aos2_vis_advance", "aos2_debug_visibility_advance_host"),
    "aos2_svc_params_default": (ci, [vp]),
    "aos2_svc_create": (ci, [ci, pvp]),
    "aos2_svc_destroy": (None, [vp]),
    "aos2_svc_vis": (vp, [vp]),
    "aos2_svc_set_params": (ci, [vp, vp]),
    "aos2_svc_set_obstacles": (ci, [vp, ci, vp, cd]),
    "aos2_svc_collide_tile": (None, [pci, pci]),
    "aos2_svc_last_device_ms": (cf, [vp]),
    **_same((ci, [vp, ci, vp, vp, vp]), "aos2_svc_motions", "aos2_debug_svc_motions_host"),
    "aos2_debug_tw_math": (ci, [ci, ci] + [vp] * 7),
    # ORBmatcher, Frame members, geometric solvers
    "aos2_matcher_create": (ci, [cf, ci, ci, pvp]),
    "aos2_matcher_destroy": (None, [vp]),
    "aos2_descriptor_distance": (ci, [vp, vp]),
    "aos2_matcher_last_device_ms": (cf, [vp]),
    "aos2_matcher_hamming_best2": (ci, [vp, vp, ci, vp, ci, vp, vp, vp]),
    "aos2_matcher_hamming_best2_device": (ci, [vp, vp, ci, vp, ci, vp, vp, vp, ci, pcf]),
    **_same((ci, [vp, vp, ci, vp, vp]), "aos2_matcher_search_by_bow", "aos2_matcher_search_by_bow_device", "aos2_matcher_search_by_bow_kf"),
    "aos2_matcher_search_by_bow_frames": (ci, [vp, vp, vp, vp]),
    "aos2_matcher_search_for_triangulation": (ci, [vp, vp, ci, ci, vp, vp]),
    "aos2_compute_distinctive_descriptors": (ci, [vp, ci, vp, vp, vp]),
    "aos2_matcher_search_by_projection": (ci, [vp, vp, vp, cf, vp, vp]),
    "aos2_matcher_search_by_projection_batch": (ci, [vp, vp, vp, ci, cf, vp, vp]),
    "aos2_matcher_search_by_projection_last": (ci, [vp, vp, vp, cf, ci, vp, vp]),
    "aos2_matcher_fuse": (ci, [vp, vp, vp, ci, vp, vp, vp]),
    "aos2_matcher_search_by_projection_kf": (ci, [vp, vp, vp, vp, vp]),
    "aos2_matcher_search_by_sim3": (ci, [vp, vp, vp, vp, vp, vp, vp]),
    "aos2_matcher_search_by_projection_reloc": (ci, [vp, vp, vp, ci, vp, vp]),
    "aos2_matcher_search_for_initialization": (ci, [vp, vp, ci, vp, vp, vp, vp, ci, vp, vp]),
    "aos2_frame_assign_features_to_grid": (ci, [vp, ci, vp, vp, cf, cf, cf, cf, vp, vp, pi32]),
    "aos2_frame_stereo_from_rgbd": (ci, [vp, ci, vp, vp, vp, vp, ci, ci, ci, cf, vp, vp]),
    "aos2_frame_is_in_frustum": (ci, [vp, vp, cf, cf, cf, cf, ci, cf, vp, vp, vp, vp, vp, vp]),
    "aos2_frame_image_bounds": (ci, [ci, ci, cf, cf, cf, cf, vp, vp]),
    **_same((ci, [vp, vp, ci]), "aos2_debug_sim3_host", "aos2_debug_pnp_host", "aos2_debug_initializer_host", "aos2_debug_sim3_opt_host",
            "aos2_debug_essential_graph_host", "aos2_debug_sim3_opt_steps_device"),
    **_same((ci, [vp, vp, vp, ci]), "aos2_sim3_ransac", "aos2_pnp_ransac", "aos2_initializer_initialize", "aos2_optimize_sim3",
            "aos2_optimize_essential_graph", "aos2_pose_optimization", "aos2_lba_solve_batch", "aos2_debug_global_ba_host"),
    "aos2_pnp_ransac_parameters": (ci, [ci, cd, ci, ci, ci, cf, vp, vp, vp]),
    "aos2_debug_pnp_set": (ci, [ci, vp, ci, vp]),
    "aos2_debug_pnp_scan": (ci, [ci, ci, vp, vp, ci, ci, ci, vp, vp, vp]),
    "aos2_debug_initializer_svd": (ci, [vp, ci, ci, vp, vp, vp]),
    "aos2_debug_initializer_rng": (ci, [ci, vp]),
    "aos2_debug_initializer_inv33": (ci, [vp, vp, C.POINTER(cd)]),
    "aos2_debug_triangulate_host": (ci, [vp, ci, vp, vp, vp, vp]),
    "aos2_triangulate_matches": (ci, [vp, vp, ci, vp, vp, vp, vp]),
    # Optimizer: LocalBA, global BA, pose, OptimizeSim3, essential graph
    "aos2_lba_create": (ci, [ci, pvp]),
    "aos2_lba_destroy": (None, [vp]),
    "aos2_lba_solve": (ci, [vp, vp, vp]),
    **_same((ci, [vp, ci]), "aos2_lba_debug_stop_at_poll", "aos2_lba_set_host_threads", "aos2_lba_set_window_groups",
            "aos2_debug_sim3_opt_steps_host", "aos2_local_map_debug_culling_rounds", "aos2_local_map_debug_connections_sort",
            "aos2_local_map_debug_normal_depth", "aos2_local_map_debug_apply_tile", "aos2_frames_set_async_keyframe_calls"),
    "aos2_lba_last_program": (ci, [vp, vp, vp]),
    "aos2_lba_last_window_slots": (ci, [vp, C.POINTER(i64)]),
    "aos2_lba_debug_host_phase": (ci, [vp, ci, ci, vp, vp]),
    "aos2_global_bundle_adjustment": (ci, [vp, vp, vp, vp]),
    **_same((ci, [vp, ci, ci, vp, vp, vp, vp, vp, cd, vp, vp, vp]), "aos2_debug_global_ba_solve_device",
            "aos2_debug_essential_graph_solve_device"),
    "aos2_debug_global_ba_reduced_device": (ci, [vp, vp, vp, cd, ci, vp, vp, vp]),
    **_same((ci, [vp, ci, vp]), "aos2_debug_global_ba_profile", "aos2_debug_essential_graph_profile"),
    **_same((cf, [vp]), "aos2_pose_optimization_last_device_ms", "aos2_optimize_sim3_last_device_ms",
            "aos2_optimize_essential_graph_last_device_ms"),
    "aos2_debug_essential_graph_arith_host": (ci, [ci, vp, ci, vp]),
    "aos2_debug_essential_graph_linearised_device": (ci, [vp] * 8),
    "aos2_debug_essential_graph_trial_device": (ci, [vp] * 10),
    # resident frame batches
    "aos2_frames_create": (ci, [ci, ci, ci, pvp]),
    "aos2_frames_destroy": (None, [vp]),
    "aos2_frames_stream": (vp, [vp]),
    "aos2_frames_wait": (ci, [vp]),
    "aos2_frames_wait_for_stream": (ci, [vp, vp]),
    "aos2_frames_device_ptr": (vp, [vp, ci]),
    "aos2_frames_build": (ci, [vp, vp, ci, vp, vp, vp, ci, ci, ci, vp, ci, sz, cf, cf, cf, cf, cf]),
    "aos2_frames_build_stereo": (ci, [vp, vp, ci, vp, vp, vp, ci, ci, ci, vp, vp, cf, cf, cf, cf, cf]),
    "aos2_frames_set_pose": (ci, [vp, vp]),
    "aos2_frames_set_distortion": (ci, [vp, cf, cf, cf, cf, cf]),
    "aos2_frames_set_map_points": (ci, [vp, vp, vp, vp]),
    "aos2_frames_get": (ci, [vp, ci, vp, sz]),
    "aos2_frames_search_by_projection_last": (ci, [vp, vp, vp, cf, ci, ci, vp]),
    "aos2_frames_pose_optimization": (ci, [vp, vp, vp]),
    "aos2_frames_discard_outliers": (ci, [vp]),
    "aos2_frames_search_local_points": (ci, [vp, vp, vp, ci, cf, cf, vp]),
    "aos2_frames_search_for_triangulation": (ci, [vp, vp, vp, ci, ci, vp, vp]),
    "aos2_frames_fuse": (ci, [vp, vp, ci, ci, vp, vp, cf, vp, vp]),
    "aos2_frames_triangulate_matches": (ci, [vp, vp, ci, vp, vp, vp, ci, vp, vp, vp]),
    # local map: UpdateLocalMap, KeyFrameCulling, UpdateConnections, apply
    "aos2_local_map_create": (ci, [ci, pvp]),
    "aos2_local_map_destroy": (None, [vp]),
    **_same((ci, [vp, vp]), "aos2_local_map_set", "aos2_local_map_get", "aos2_local_map_set_culling_view", "aos2_local_map_apply",
            "aos2_debug_local_map_apply_host"),
    "aos2_local_map_debug_limits": (ci, [vp, i64, ci]),
    **_same((ci, [vp]), "aos2_local_map_last_groups", "aos2_local_map_last_culling_rounds"),
    "aos2_frames_update_local_map": (ci, [vp, vp, vp, ci, vp, vp, ci, vp, vp]),
    "aos2_frames_track_local_map_stats": (ci, [vp, vp, ci, ci, vp, vp]),
    **_same((ci, [vp, ci, ci, vp, vp, vp, ci, vp, vp, ci, vp, vp]), "aos2_debug_local_map_host", "aos2_local_map_update"),
    "aos2_debug_local_map_stats_host": (ci, [vp, ci, ci, vp, vp, vp, ci, ci, vp, vp]),
    "aos2_local_map_keyframe_culling": (ci, [vp, ci, ci, vp, vp, vp, vp, vp, ci, vp]),
    "aos2_debug_keyframe_culling_host": (ci, [vp, vp, ci, ci, vp, vp, vp, vp, vp, ci, vp]),
    "aos2_local_map_get_culling_view": (ci, [vp, vp, vp]),
    **_same((cf, [vp]), "aos2_local_map_last_culling_device_ms", "aos2_local_map_last_connections_device_ms",
            "aos2_local_map_last_normal_depth_device_ms"),
    "aos2_local_map_update_normal_depth": (ci, [vp, vp]),
    "aos2_debug_update_normal_depth_host": (ci, [vp, vp, vp]),
    **_same((ci, [vp, ci, ci, vp, vp, vp, ci, vp, vp, vp, ci, vp, vp, vp, ci]), "aos2_local_map_update_connections",
            "aos2_debug_update_connections_host"),
    "aos2_local_map_last_apply": (ci, [vp, vp, vp, vp]),
    "aos2_local_map_last_apply_bytes": (i64, [vp]),
    # replay of a fixed call sequence, dataset helper
    "aos2_capture_begin": (ci, [vp]),
    "aos2_capture_end": (ci, [vp, pvp]),
    "aos2_graph_launch": (ci, [vp, vp]),
    "aos2_graph_nodes": (ci, [vp]),
    "aos2_graph_destroy": (None, [vp]),
    "aos2_png_unfilter": (ci, [vp, ci, ci, ci]),
    # test taps of single routines and kernels
    "aos2_debug_octree_host": (ci, [vp, vp, vp, ci, ci, ci, ci, ci, ci, vp, ci]),
    "aos2_debug_sincos_host": (None, [cf, pcf, pcf]),
    "aos2_debug_extractor_plan": (ci, [vp, ci, ci, vp, vp, ci, pci, vp]),
    "aos2_debug_sincos_device": (ci, [vp, ci, vp, vp, ci]),
    "aos2_debug_wave_ops_device": (ci, [vp, vp, ci, ci, vp, vp, ci]),
    "aos2_debug_row_sums_scatter_device": (ci, [vp, ci, vp, vp, ci]),
    "aos2_debug_pose_blocks_device": (ci, [vp, vp, vp, vp, vp, vp, vp, ci, ci]),
    "aos2_debug_pose_pass_device": (ci, [vp, ci, ci, ci]),
    "aos2_debug_lba_reduced_solve_device": (ci, [ci] + [vp] * 12 + [ci]),
    "aos2_debug_lba_assemble_device": (ci, [vp, vp, ci, ci, ci, vp, vp]),
    "aos2_debug_lba_trial_device": (ci, [vp, vp, ci, ci, ci, vp, vp, ci, vp]),
}
