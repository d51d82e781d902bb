"""ctypes binding of the C ABI declared in include/aos2.h (lib/libaos2.so, built by csrc/Makefile).

This is plumbing: numpy arrays in, numpy arrays out, every call goes through the extern "C" entry
points a C++/cgo/JNI caller would use.  There is no Python or CPU fallback: a missing library
raises LibraryMissing, a missing GPU surfaces as AosError(AOS2_ERR_NO_DEVICE).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

AOS2_OK = 0
AOS2_ERR_ARG, AOS2_ERR_CAPACITY, AOS2_ERR_TOO_SMALL, AOS2_ERR_HIP, AOS2_ERR_NO_DEVICE = -1, -2, -3, -4, -5
AOS2_ERR_STOPPED = 1

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])


class LibraryMissing(RuntimeError):
    pass


class AosError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"aos2 error {code}: {msg}")
        self.code = code


def lib_path():
    return os.environ.get("AOS2_LIB") or os.path.join(_HERE, "lib", "libaos2.so")


def lib():
    global _LIB
    if _LIB is None:
        p = lib_path()
        if not os.path.exists(p):
            raise LibraryMissing(f"{p} not found: build it with `make -C {_HERE}/csrc` "
                                 "(__graft_entry__.build()); there is no fallback path")
        L = C.CDLL(p)
        L.aos2_last_error.restype = C.c_char_p
        L.aos2_version.restype = C.c_char_p
        vp, ci, cf = C.c_void_p, C.c_int, C.c_float
        L.aos2_extractor_create.argtypes = [ci, cf, ci, ci, ci, ci, C.POINTER(vp)]
        L.aos2_extractor_destroy.argtypes = [vp]
        L.aos2_extractor_levels.argtypes = [vp]
        L.aos2_extractor_scale_factor.argtypes = [vp]
        L.aos2_extractor_scale_factor.restype = cf
        for n in ("scale_factors", "inv_scale_factors", "sigma2", "inv_sigma2"):
            f = getattr(L, "aos2_extractor_" + n)
            f.argtypes = [vp]
            f.restype = C.POINTER(cf)
        for n in ("features_per_level", "umax"):
            f = getattr(L, "aos2_extractor_" + n)
            f.argtypes = [vp]
            f.restype = C.POINTER(ci)
        L.aos2_extractor_max_keypoints.argtypes = [vp]
        L.aos2_extractor_max_keypoints_for.argtypes = [vp, ci, ci]
        L.aos2_extractor_extract.argtypes = [vp, vp, ci, ci, ci, vp, vp, ci, C.POINTER(ci)]
        L.aos2_extractor_extract_batch.argtypes = [vp, vp, ci, ci, ci, ci, C.c_size_t, vp, vp, ci, vp]
        L.aos2_host_alloc.argtypes = [C.POINTER(vp), C.c_size_t]
        L.aos2_host_free.argtypes = [vp]
        L.aos2_extractor_extract_batch_device.argtypes = [vp, vp, ci, ci, ci, ci, C.c_size_t, vp, vp, ci, vp]
        L.aos2_extractor_extract_batch_device_async.argtypes = [vp, vp, ci, ci, ci, ci, C.c_size_t, vp, vp, ci, vp]
        L.aos2_extractor_wait.argtypes = [vp]
        L.aos2_extractor_pyramid_level_size.argtypes = [vp, ci, C.POINTER(ci), C.POINTER(ci)]
        L.aos2_extractor_pyramid_level.argtypes = [vp, ci, ci, ci, vp, ci]
        L.aos2_extractor_debug_candidates.argtypes = [vp, ci, ci, vp, vp, vp, ci, C.POINTER(ci)]
        L.aos2_extractor_last_timing.argtypes = [vp, vp, ci]
        if hasattr(L, "aos2_extractor_set_chunks"):
            L.aos2_extractor_set_chunks.argtypes = [vp, ci]
        L.aos2_extractor_bench_fast.argtypes = [vp, ci, C.POINTER(cf)]
        L.aos2_extractor_bench_describe.argtypes = [vp, ci, C.POINTER(cf)]
        if hasattr(L, "aos2_compute_stereo_matches"):
            L.aos2_compute_stereo_matches.argtypes = [vp, vp, ci, vp, vp, ci, vp, vp, ci, cf, cf, vp, vp]
            L.aos2_compute_stereo_matches_device.argtypes = [vp, vp, ci, vp, vp, vp, vp, vp, vp, ci, cf, cf, vp, vp]
            L.aos2_compute_stereo_matches_device_async.argtypes = [vp, vp, ci, vp, vp, vp, vp, vp, vp, ci, cf, cf, vp, vp]
            L.aos2_compute_stereo_matches_last_device_ms.restype = cf
            L.aos2_compute_stereo_matches_last_device_ms.argtypes = [vp]
        if hasattr(L, "aos2_vocabulary_create"):
            L.aos2_vocabulary_create.argtypes = [ci, C.POINTER(vp)]
            L.aos2_vocabulary_destroy.argtypes = [vp]
            L.aos2_vocabulary_load_binary.argtypes = [vp, C.c_char_p]
            L.aos2_vocabulary_load_text.argtypes = [vp, C.c_char_p]
            L.aos2_vocabulary_save_binary.argtypes = [vp, C.c_char_p]
            L.aos2_vocabulary_set_nodes.argtypes = [vp, ci, ci, ci, ci, ci, vp, vp, vp, vp]
            for nm in ("k", "levels", "scoring", "weighting", "nodes", "empty"):
                getattr(L, "aos2_vocabulary_" + nm).argtypes = [vp]
            L.aos2_vocabulary_size.argtypes = [vp]
            L.aos2_vocabulary_get_nodes.argtypes = [vp] * 6
            L.aos2_vocabulary_size.restype = C.c_uint
            L.aos2_vocabulary_transform.argtypes = [vp, vp, ci, ci, vp, vp, C.POINTER(ci), vp, vp, vp, C.POINTER(ci), vp, vp]
            L.aos2_vocabulary_transform_device.argtypes = [vp, ci, vp, vp, ci, ci] + [vp] * 9
            L.aos2_vocabulary_last_device_ms.restype = cf
            L.aos2_vocabulary_last_device_ms.argtypes = [vp]
            L.aos2_vocabulary_score.argtypes = [vp, vp, vp, ci, vp, vp, ci, C.POINTER(C.c_double)]
        L.aos2_kfdb_create.argtypes = [vp, ci, C.POINTER(vp)]
        L.aos2_kfdb_destroy.argtypes = [vp]
        L.aos2_kfdb_put.argtypes = [vp, vp, vp, ci, C.POINTER(C.c_int32)]
        L.aos2_kfdb_put_device.argtypes = [vp, vp, ci, vp, vp, vp, ci, vp]
        for nm in ("add", "erase", "drop"):
            getattr(L, "aos2_kfdb_" + nm).argtypes = [vp, C.c_int32]
        L.aos2_kfdb_clear.argtypes = [vp]
        L.aos2_kfdb_size.argtypes = [vp]
        L.aos2_kfdb_arena_capacity.argtypes = [vp]
        L.aos2_kfdb_arena_capacity.restype = C.c_int64
        L.aos2_kfdb_set_neighbours.argtypes = [vp, ci, vp, vp]
        L.aos2_kfdb_last_device_ms.argtypes = [vp]
        L.aos2_kfdb_last_device_ms.restype = cf
        for nm in ("aos2_kfdb_detect", "aos2_debug_kfdb_host"):
            getattr(L, nm).argtypes = [vp, vp, vp, ci]
        for nm in ("aos2_kfdb_scores", "aos2_debug_kfdb_scores_host"):
            getattr(L, nm).argtypes = [vp, vp, vp, ci, vp, C.POINTER(cf)]
        L.aos2_vis_camera_default.argtypes = [ci, vp]
        L.aos2_vis_create.argtypes = [ci, C.POINTER(vp)]
        L.aos2_vis_destroy.argtypes = [vp]
        L.aos2_vis_destroy.restype = None
        L.aos2_vis_set_camera.argtypes = [vp, vp]
        L.aos2_vis_set_map.argtypes = [vp, ci] + [vp] * 6
        L.aos2_vis_map_size.argtypes = [vp]
        L.aos2_vis_gate_tile.argtypes = [C.POINTER(ci), C.POINTER(ci)]
        L.aos2_vis_gate_tile.restype = None
        L.aos2_vis_last_device_ms.argtypes = [vp]
        L.aos2_vis_last_device_ms.restype = cf
        for nm in ("aos2_vis_count", "aos2_vis_count_poses", "aos2_debug_visibility_host", "aos2_debug_visibility_poses_host"):
            getattr(L, nm).argtypes = [vp, ci, vp, vp, vp, vp]
        for nm in ("aos2_vis_motion_costs", "aos2_debug_visibility_motion_costs_host"):
            getattr(L, nm).argtypes = [vp, ci, vp, vp, ci, vp]
        for nm in ("aos2_vis_advance", "aos2_debug_visibility_advance_host"):
            getattr(L, nm).argtypes = [vp, ci, vp, ci, C.POINTER(C.c_int32)]
        L.aos2_svc_params_default.argtypes = [vp]
        L.aos2_svc_create.argtypes = [ci, C.POINTER(vp)]
        L.aos2_svc_destroy.argtypes = [vp]
        L.aos2_svc_destroy.restype = None
        L.aos2_svc_vis.argtypes = [vp]
        L.aos2_svc_vis.restype = vp
        L.aos2_svc_set_params.argtypes = [vp, vp]
        L.aos2_svc_set_obstacles.argtypes = [vp, ci, vp, C.c_double]
        L.aos2_svc_collide_tile.argtypes = [C.POINTER(ci), C.POINTER(ci)]
        L.aos2_svc_collide_tile.restype = None
        L.aos2_svc_last_device_ms.argtypes = [vp]
        L.aos2_svc_last_device_ms.restype = cf
        for nm in ("aos2_svc_valid", "aos2_debug_svc_valid_host"):
            getattr(L, nm).argtypes = [vp, ci, vp, vp, vp, vp]
        for nm in ("aos2_svc_motions", "aos2_debug_svc_motions_host"):
            getattr(L, nm).argtypes = [vp, ci, vp, vp, vp]
        L.aos2_debug_tw_math.argtypes = [ci, ci] + [vp] * 7
        L.aos2_local_map_create.argtypes = [ci, C.POINTER(vp)]
        L.aos2_local_map_destroy.argtypes = [vp]
        L.aos2_local_map_destroy.restype = None
        L.aos2_local_map_set.argtypes = [vp, vp]
        L.aos2_local_map_get.argtypes = [vp, vp]
        L.aos2_local_map_debug_limits.argtypes = [vp, C.c_int64, ci]
        L.aos2_local_map_last_groups.argtypes = [vp]
        L.aos2_frames_update_local_map.argtypes = [vp, vp, vp, ci, vp, vp, ci, vp, vp]
        L.aos2_frames_track_local_map_stats.argtypes = [vp, vp, ci, ci, vp, vp]
        L.aos2_debug_local_map_host.argtypes = [vp, ci, ci, vp, vp, vp, ci, vp, vp, ci, vp, vp]
        L.aos2_local_map_update.argtypes = [vp, ci, ci, vp, vp, vp, ci, vp, vp, ci, vp, vp]
        L.aos2_debug_local_map_stats_host.argtypes = [vp, ci, ci, vp, vp, vp, ci, ci, vp, vp]
        L.aos2_local_map_set_culling_view.argtypes = [vp, vp]
        L.aos2_local_map_keyframe_culling.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp, ci, vp]
        L.aos2_local_map_debug_culling_rounds.argtypes = [vp, ci]
        L.aos2_local_map_last_culling_rounds.argtypes = [vp]
        L.aos2_local_map_last_culling_device_ms.argtypes = [vp]
        L.aos2_local_map_last_culling_device_ms.restype = C.c_float
        L.aos2_debug_keyframe_culling_host.argtypes = [vp, vp, ci, ci, vp, vp, vp, vp, vp, ci, vp]
        L.aos2_local_map_get_culling_view.argtypes = [vp, vp, vp]
        L.aos2_local_map_update_connections.argtypes = [vp, ci, ci, vp, vp, vp, ci, vp, vp, vp, ci, vp, vp, vp, ci]
        L.aos2_debug_update_connections_host.argtypes = [vp, ci, ci, vp, vp, vp, ci, vp, vp, vp, ci, vp, vp, vp, ci]
        L.aos2_local_map_last_connections_device_ms.argtypes = [vp]
        L.aos2_local_map_last_connections_device_ms.restype = C.c_float
        L.aos2_local_map_debug_connections_sort.argtypes = [vp, ci]
        L.aos2_local_map_apply.argtypes = [vp, vp]
        L.aos2_debug_local_map_apply_host.argtypes = [vp, vp]
        L.aos2_local_map_last_apply.argtypes = [vp, vp, vp, vp]
        L.aos2_local_map_last_apply_bytes.argtypes = [vp]
        L.aos2_local_map_last_apply_bytes.restype = C.c_int64
        L.aos2_local_map_debug_apply_tile.argtypes = [vp, ci]
        L.aos2_debug_octree_host.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, ci, vp, ci]
        L.aos2_debug_sincos_host.argtypes = [cf, C.POINTER(cf), C.POINTER(cf)]
        L.aos2_debug_extractor_plan.argtypes = [vp, ci, ci, vp, vp, ci, C.POINTER(ci), vp]
        L.aos2_debug_sincos_device.argtypes = [vp, ci, vp, vp, ci]
        L.aos2_debug_wave_ops_device.argtypes = [vp, vp, ci, ci, vp, vp, ci]
        L.aos2_debug_row_sums_scatter_device.argtypes = [vp, ci, vp, vp, ci]
        L.aos2_debug_pose_blocks_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, ci, ci]
        if hasattr(L, "aos2_debug_pose_pass_device"):
            L.aos2_debug_pose_pass_device.argtypes = [vp, ci, ci, ci]
        L.aos2_debug_lba_reduced_solve_device.argtypes = [ci] + [vp] * 12 + [ci]
        L.aos2_debug_triangulate_host.argtypes = [vp, ci, vp, vp, vp, vp]
        L.aos2_triangulate_matches.argtypes = [vp, vp, ci, vp, vp, vp, vp]
        L.aos2_debug_sim3_host.argtypes = [vp, vp, ci]
        L.aos2_sim3_ransac.argtypes = [vp, vp, vp, ci]
        L.aos2_debug_pnp_host.argtypes = [vp, vp, ci]
        L.aos2_debug_pnp_set.argtypes = [ci, vp, ci, vp]
        L.aos2_debug_pnp_scan.argtypes = [ci, ci, vp, vp, ci, ci, ci, vp, vp, vp]
        L.aos2_pnp_ransac.argtypes = [vp, vp, vp, ci]
        L.aos2_pnp_ransac_parameters.argtypes = [ci, C.c_double, ci, ci, ci, cf, vp, vp, vp]
        L.aos2_debug_initializer_host.argtypes = [vp, vp, ci]
        L.aos2_debug_initializer_svd.argtypes = [vp, ci, ci, vp, vp, vp]
        L.aos2_debug_initializer_rng.argtypes = [ci, vp]
        L.aos2_debug_initializer_inv33.argtypes = [vp, vp, C.POINTER(C.c_double)]
        L.aos2_initializer_initialize.argtypes = [vp, vp, vp, ci]
        L.aos2_debug_sim3_opt_host.argtypes = [vp, vp, ci]
        L.aos2_debug_sim3_opt_steps_host.argtypes = [vp, ci]
        L.aos2_debug_sim3_opt_steps_device.argtypes = [vp, vp, ci]
        L.aos2_optimize_sim3.argtypes = [vp, vp, vp, ci]
        L.aos2_optimize_sim3_last_device_ms.argtypes = [vp]
        L.aos2_optimize_sim3_last_device_ms.restype = cf
        L.aos2_debug_essential_graph_host.argtypes = [vp, vp, ci]
        L.aos2_optimize_essential_graph.argtypes = [vp, vp, vp, ci]
        L.aos2_optimize_essential_graph_last_device_ms.argtypes = [vp]
        L.aos2_optimize_essential_graph_last_device_ms.restype = cf
        L.aos2_debug_essential_graph_profile.argtypes = [vp, ci, vp]
        L.aos2_debug_essential_graph_arith_host.argtypes = [ci, vp, ci, vp]
        L.aos2_debug_essential_graph_solve_device.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp, C.c_double, vp, vp, vp]
        L.aos2_debug_essential_graph_linearised_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
        L.aos2_debug_essential_graph_trial_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.aos2_global_bundle_adjustment.argtypes = [vp, vp, vp, vp]
        L.aos2_debug_global_ba_host.argtypes = [vp, vp, vp, ci]
        L.aos2_debug_global_ba_solve_device.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp, C.c_double, vp, vp, vp]
        L.aos2_debug_global_ba_reduced_device.argtypes = [vp, vp, vp, C.c_double, ci, vp, vp, vp]
        L.aos2_debug_global_ba_profile.argtypes = [vp, ci, vp]
        if hasattr(L, "aos2_matcher_create"):
            L.aos2_matcher_create.argtypes = [cf, ci, ci, C.POINTER(vp)]
            L.aos2_matcher_destroy.argtypes = [vp]
            L.aos2_descriptor_distance.argtypes = [vp, vp]
            if hasattr(L, "aos2_matcher_last_device_ms"):
                L.aos2_matcher_last_device_ms.argtypes = [vp]
                L.aos2_matcher_last_device_ms.restype = cf
            L.aos2_matcher_hamming_best2.argtypes = [vp, vp, ci, vp, ci, vp, vp, vp]
            L.aos2_matcher_hamming_best2_device.argtypes = [vp, vp, ci, vp, ci, vp, vp, vp, ci, C.POINTER(cf)]
            L.aos2_matcher_search_by_bow.argtypes = [vp, vp, ci, vp, vp]
            L.aos2_matcher_search_by_bow_device.argtypes = [vp, vp, ci, vp, vp]
            L.aos2_matcher_search_by_bow_frames.argtypes = [vp, vp, vp, vp]
            L.aos2_vocabulary_stream.argtypes = [vp]
            L.aos2_vocabulary_stream.restype = vp
            if hasattr(L, "aos2_matcher_search_by_bow_kf"):
                L.aos2_matcher_search_by_bow_kf.argtypes = [vp, vp, ci, vp, vp]
                L.aos2_matcher_search_for_triangulation.argtypes = [vp, vp, ci, ci, vp, vp]
                L.aos2_compute_distinctive_descriptors.argtypes = [vp, ci, vp, vp, vp]
            if hasattr(L, "aos2_matcher_fuse"):
                L.aos2_matcher_fuse.argtypes = [vp, vp, vp, ci, vp, vp, vp]
                L.aos2_matcher_search_by_projection_kf.argtypes = [vp, vp, vp, vp, vp]
                L.aos2_matcher_search_by_sim3.argtypes = [vp, vp, vp, vp, vp, vp, vp]
                L.aos2_matcher_search_by_projection_reloc.argtypes = [vp, vp, vp, ci, vp, vp]
            if hasattr(L, "aos2_frame_assign_features_to_grid"):
                L.aos2_frame_assign_features_to_grid.argtypes = [vp, ci, vp, vp, cf, cf, cf, cf, vp, vp, C.POINTER(C.c_int32)]
                L.aos2_frame_stereo_from_rgbd.argtypes = [vp, ci, vp, vp, vp, vp, ci, ci, ci, cf, vp, vp]
            if hasattr(L, "aos2_frame_is_in_frustum"):
                L.aos2_frame_is_in_frustum.argtypes = [vp, vp, cf, cf, cf, cf, ci, cf, vp, vp, vp, vp, vp, vp]
            if hasattr(L, "aos2_matcher_search_for_initialization"):
                L.aos2_matcher_search_for_initialization.argtypes = [vp, vp, ci, vp, vp, vp, vp, ci, vp, vp]
            if hasattr(L, "aos2_matcher_search_by_projection_batch"):
                L.aos2_matcher_search_by_projection_batch.argtypes = [vp, vp, vp, ci, cf, vp, vp]
            L.aos2_matcher_search_by_projection.argtypes = [vp, vp, vp, cf, vp, vp]
            L.aos2_matcher_search_by_projection_last.argtypes = [vp, vp, vp, cf, ci, vp, vp]
        if hasattr(L, "aos2_lba_create"):
            L.aos2_lba_create.argtypes = [ci, C.POINTER(vp)]
            L.aos2_lba_destroy.argtypes = [vp]
            L.aos2_lba_solve.argtypes = [vp, vp, vp]
            L.aos2_lba_solve_batch.argtypes = [vp, vp, vp, ci]
            L.aos2_lba_debug_stop_at_poll.argtypes = [vp, ci]
            L.aos2_lba_set_host_threads.argtypes = [vp, ci]
            L.aos2_lba_set_window_groups.argtypes = [vp, ci]
            L.aos2_lba_last_program.argtypes = [vp, vp, vp]
            L.aos2_lba_debug_host_phase.argtypes = [vp, ci, ci, vp, vp]
            L.aos2_debug_lba_assemble_device.argtypes = [vp, vp, ci, ci, ci, vp, vp]
            L.aos2_debug_lba_trial_device.argtypes = [vp, vp, ci, ci, ci, vp, vp, ci, vp]
            if hasattr(L, "aos2_pose_optimization"):
                L.aos2_pose_optimization.argtypes = [vp, vp, vp, ci]
                L.aos2_pose_optimization_last_device_ms.argtypes = [vp]
                L.aos2_pose_optimization_last_device_ms.restype = cf
        if hasattr(L, "aos2_frames_create"):
            L.aos2_frames_create.argtypes = [ci, ci, ci, C.POINTER(vp)]
            L.aos2_frames_destroy.argtypes = [vp]
            L.aos2_frames_stream.argtypes = [vp]
            L.aos2_frames_stream.restype = vp
            L.aos2_frames_wait.argtypes = [vp]
            L.aos2_frames_wait_for_stream.argtypes = [vp, vp]
            L.aos2_frames_device_ptr.argtypes = [vp, ci]
            L.aos2_frames_search_for_triangulation.argtypes = [vp, vp, vp, ci, ci, vp, vp]
            L.aos2_frames_fuse.argtypes = [vp, vp, ci, ci, vp, vp, cf, vp, vp]
            L.aos2_frames_triangulate_matches.argtypes = [vp, vp, ci, vp, vp, vp, ci, vp, vp, vp]
            L.aos2_frames_device_ptr.restype = vp
            L.aos2_frames_build.argtypes = [vp, vp, ci, vp, vp, vp, ci, ci, ci, vp, ci, C.c_size_t, cf, cf, cf, cf, cf]
            L.aos2_frames_build_stereo.argtypes = [vp, vp, ci, vp, vp, vp, ci, ci, ci, vp, vp, cf, cf, cf, cf, cf]
            L.aos2_frames_set_pose.argtypes = [vp, vp]
            L.aos2_frames_set_distortion.argtypes = [vp, cf, cf, cf, cf, cf]
            L.aos2_frame_image_bounds.argtypes = [ci, ci, cf, cf, cf, cf, vp, vp]
            L.aos2_frames_set_map_points.argtypes = [vp, vp, vp, vp]
            L.aos2_frames_get.argtypes = [vp, ci, vp, C.c_size_t]
            L.aos2_frames_search_by_projection_last.argtypes = [vp, vp, vp, cf, ci, ci, vp]
            L.aos2_frames_pose_optimization.argtypes = [vp, vp, vp]
            L.aos2_frames_discard_outliers.argtypes = [vp]
            L.aos2_frames_search_local_points.argtypes = [vp, vp, vp, ci, cf, cf, vp]
            L.aos2_extractor_stream_wait.argtypes = [vp, vp]
            L.aos2_extractor_wait_for_stream.argtypes = [vp, vp]
            L.aos2_lba_last_window_slots.argtypes = [vp, C.POINTER(C.c_int64)]
            L.aos2_extractor_pack_slots.argtypes = [vp, ci, vp, vp, vp, ci, vp, C.c_size_t, vp]
            L.aos2_capture_begin.argtypes = [vp]
            L.aos2_capture_end.argtypes = [vp, C.POINTER(vp)]
            L.aos2_graph_launch.argtypes = [vp, vp]
            L.aos2_graph_nodes.argtypes = [vp]
            L.aos2_graph_destroy.argtypes = [vp]
            L.aos2_graph_destroy.restype = None
        _LIB = _RecLib(L)
    return _LIB


# ---- recording (bench harness): the calls of a job captured instead of executed, for the native step runner (csrc/host_runner.cpp)
class _Call(C.Structure):
    _fields_ = [("fn", C.c_void_p), ("n_int", C.c_int32), ("n_fp", C.c_int32), ("iargs", C.c_int64 * 24), ("fargs", C.c_uint64 * 8)]


# the functions a recorded job may consist of: work that is enqueued / solved / waited for.  Everything else (getters, stream handles,
# setters) executes at once even while a recording is open
_RECORDABLE = {
    "aos2_frames_set_pose", "aos2_extractor_extract_batch_device_async", "aos2_frames_build", "aos2_frames_build_stereo",
    "aos2_compute_stereo_matches_device_async", "aos2_frames_search_by_projection_last", "aos2_frames_pose_optimization",
    "aos2_frames_discard_outliers", "aos2_frames_search_local_points", "aos2_frames_wait", "aos2_extractor_wait",
    "aos2_extractor_stream_wait", "aos2_extractor_wait_for_stream", "aos2_vocabulary_transform_device", "aos2_matcher_search_by_bow_frames",
    "aos2_frames_search_for_triangulation", "aos2_frames_fuse", "aos2_lba_solve_batch", "aos2_extractor_pack_slots",
    "hipMemcpyAsync", "hipStreamSynchronize", "hipStreamWaitEvent", "hipEventRecord", "hipMemcpy",
}
_REC = None   # the open recording (a list), or None


class recording:
    """with capi.recording() as calls: ...   -- the recordable C calls made inside are appended to `calls` (not executed; they
    "return" AOS2_OK); calls.keep holds every argument object alive; calls.array() is the aos2_call_t array for the runner"""

    class _List(list):
        def __init__(self):
            super().__init__()
            self.keep = []
            self.names = []   # function name per call (diagnostics)

        def array(self):
            a = (_Call * max(1, len(self)))()
            for i, c in enumerate(self):
                a[i] = c
            return a

    def __enter__(self):
        global _REC
        assert _REC is None, "recordings do not nest"
        _REC = recording._List()
        return _REC

    def __exit__(self, *exc):
        global _REC
        _REC = None
        return False


def _record(fn, name, args):
    import struct
    at = fn.argtypes
    if at is None or len(at) != len(args):
        raise TypeError(f"recording {name}: the function needs argtypes for every argument")
    c = _Call()
    c.fn = C.cast(fn, C.c_void_p).value
    ni = nf = 0
    for a, t in zip(args, at):
        if t is C.c_float or t is C.c_double:
            v = float(a.value if isinstance(a, C._SimpleCData) else a)
            bits = struct.unpack("<I", struct.pack("<f", v))[0] if t is C.c_float else struct.unpack("<Q", struct.pack("<d", v))[0]
            if nf >= 8:
                raise TypeError(f"recording {name}: more than 8 floating-point arguments")
            c.fargs[nf] = bits
            nf += 1
            continue
        if a is None:
            v = 0
        elif isinstance(a, (int, np.integer)):
            v = int(a)
        elif isinstance(a, C._SimpleCData):
            v = a.value or 0
        else:
            v = C.cast(a, C.c_void_p).value or 0   # pointers, arrays, byref()
        if ni >= 24:
            raise TypeError(f"recording {name}: more than 24 integer arguments")
        if v >= 1 << 63:
            v -= 1 << 64
        c.iargs[ni] = v
        ni += 1
    c.n_int, c.n_fp = ni, nf
    _REC.append(c)
    _REC.keep.append(args)
    _REC.names.append(name)
    return AOS2_OK


class _RecLib:
    """the loaded library; a recordable function called while a recording is open is captured instead of executed"""

    def __init__(self, L):
        object.__setattr__(self, "_L", L)
        object.__setattr__(self, "_w", {})
        object.__setattr__(self, "_names", frozenset(_RECORDABLE))   # (kept here: module globals are gone when handles close at exit)

    def __getattr__(self, name):
        w = self._w.get(name)
        if w is None:
            fn = getattr(self._L, name)
            if name in self._names:
                def w(*args, _fn=fn, _name=name):
                    if _REC is None:
                        return _fn(*args)
                    return _record(_fn, _name, args)
                w.argtypes_of = fn
            else:
                w = fn
            self._w[name] = w
        return w


class Graph:
    """include/aos2.h "Replay of a fixed call sequence": the calls made inside `with Graph.capture(stream) as g:` are recorded
    (nothing runs); g.launch() enqueues them all with one call"""

    def __init__(self, stream):
        self.L, self.stream, self.h = lib(), stream, None

    @classmethod
    def capture(cls, stream):
        return cls(stream)

    def __enter__(self):
        _check(self.L.aos2_capture_begin(self.stream))
        return self

    def __exit__(self, et, ev, tb):
        h = C.c_void_p()
        st = self.L.aos2_capture_end(self.stream, C.byref(h))
        if et is None:
            _check(st)
            self.h = h
        elif st == AOS2_OK and h:
            self.L.aos2_graph_destroy(h)   # (the body failed: what was recorded until then is dropped)
        return False

    def nodes(self):
        return int(self.L.aos2_graph_nodes(self.h))

    def launch(self, stream=None):
        _check(self.L.aos2_graph_launch(self.h, self.stream if stream is None else stream))

    def close(self):
        if self.h:
            self.L.aos2_graph_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_HIP = None


def hip_runtime():
    """libamdhip64 (the runtime the library itself links) for the harness's own copies: hipMemcpyAsync & co, recordable"""
    global _HIP
    if _HIP is None:
        H = C.CDLL("libamdhip64.so")
        vp = C.c_void_p
        H.hipMemcpyAsync.argtypes = [vp, vp, C.c_size_t, C.c_int, vp]
        H.hipMemcpy.argtypes = [vp, vp, C.c_size_t, C.c_int]
        H.hipStreamSynchronize.argtypes = [vp]
        H.hipStreamWaitEvent.argtypes = [vp, vp, C.c_uint]
        H.hipEventRecord.argtypes = [vp, vp]
        H.hipStreamCreateWithFlags.argtypes = [C.POINTER(vp), C.c_uint]
        H.hipEventCreateWithFlags.argtypes = [C.POINTER(vp), C.c_uint]
        H.hipHostMalloc.argtypes = [C.POINTER(vp), C.c_size_t, C.c_uint]
        _HIP = _RecLib(H)
    return _HIP


HIP_D2H, HIP_H2D = 2, 1


class Runner:
    """csrc/host_runner.cpp: the step schedule of bench.py on native threads over recorded call lists"""
    PIPE_WAIT, PIPE_STEP, KF_JOB, LBA_JOB = 0, 1, 2, 3

    def __init__(self, n_pipes, n_lba):
        p = os.path.join(os.path.dirname(lib_path()), "libaos2_runner.so")
        if not os.path.exists(p):
            raise LibraryMissing(f"{p} not found: build it with `make -C {_HERE}/csrc`")
        R = C.CDLL(p)
        vp = C.c_void_p
        R.aos2_runner_create.restype = vp
        R.aos2_runner_create.argtypes = [C.c_int, C.c_int]
        R.aos2_runner_destroy.argtypes = [vp]
        R.aos2_runner_set_list.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int]
        R.aos2_runner_step.argtypes = [vp, C.c_int]
        R.aos2_runner_run.argtypes = [vp, C.c_int, C.c_int]
        R.aos2_runner_sync.argtypes = [vp]
        R.aos2_runner_error.argtypes = [vp]
        R.aos2_runner_error.restype = C.c_char_p
        R.aos2_runner_reset_stats.argtypes = [vp]
        R.aos2_runner_stats.argtypes = [vp, C.c_int, vp, C.c_int]
        R.aos2_runner_set_lba_every.argtypes = [vp, C.c_int]
        R.aos2_runner_last_lba.argtypes = [vp]
        self.R = R
        self.h = R.aos2_runner_create(int(n_pipes), int(n_lba))
        if not self.h:
            raise ValueError("aos2_runner_create")
        self._keep = {}

    def __del__(self):
        if getattr(self, "h", None):
            self.R.aos2_runner_destroy(self.h)
            self.h = None

    def set_list(self, kind, index, calls):
        """calls: a recording (or None / empty: the job is skipped)"""
        n = len(calls) if calls else 0
        arr = calls.array() if n else None
        if self.R.aos2_runner_set_list(self.h, kind, index, C.cast(arr, C.c_void_p) if n else None, n) != 0:
            raise ValueError("aos2_runner_set_list")
        self._keep[(kind, index)] = (calls, arr)

    def _st(self, st):
        if st != 0:
            raise AosError(st, self.R.aos2_runner_error(self.h).decode() + ": " + lib().aos2_last_error().decode(errors="replace"))

    def set_lba_every(self, n):
        """a LocalBA job every n steps (its list then solves the windows of n steps in one call)"""
        if self.R.aos2_runner_set_lba_every(self.h, int(n)) != 0:
            raise ValueError("aos2_runner_set_lba_every")

    def last_lba(self):
        return int(self.R.aos2_runner_last_lba(self.h))

    def step(self, s):
        self._st(self.R.aos2_runner_step(self.h, int(s)))

    def run(self, s0, n):
        self._st(self.R.aos2_runner_run(self.h, int(s0), int(n)))

    def sync(self):
        self._st(self.R.aos2_runner_sync(self.h))

    def reset_stats(self):
        self.R.aos2_runner_reset_stats(self.h)

    def stats(self, which):
        n = self.R.aos2_runner_stats(self.h, which, None, 0)
        a = np.zeros(max(n, 1), np.float64)
        self.R.aos2_runner_stats(self.h, which, _p(a), n)
        return a[:n]


def _check(st, ok=(AOS2_OK,)):
    if st not in ok:
        raise AosError(st, lib().aos2_last_error().decode(errors="replace"))
    return st


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class _HostBlock:
    """page-locked host allocation (aos2_host_alloc), released with the last array that views it"""

    def __init__(self, nbytes):
        self.L = lib()
        p = C.c_void_p()
        _check(self.L.aos2_host_alloc(C.byref(p), max(int(nbytes), 1)))
        self.p = p.value

    def __del__(self):
        if getattr(self, "p", None) and C is not None:   # (at interpreter shutdown the module globals may already be gone)
            self.L.aos2_host_free(C.c_void_p(self.p))
            self.p = None


def host_empty(shape, dtype=np.uint8):
    """uninitialised numpy array in page-locked host memory (for Extractor.extract_batch inputs / outputs)"""
    dt = np.dtype(dtype)
    n = int(np.prod(shape)) * dt.itemsize
    blk = _HostBlock(n)
    buf = (C.c_uint8 * max(n, 1)).from_address(blk.p)
    buf._block = blk   # the ctypes view keeps the allocation alive; numpy keeps the view alive (.base)
    return np.frombuffer(buf, dtype=dt, count=int(np.prod(shape))).reshape(shape)


def device_count():
    return lib().aos2_device_count()


def device_local_cpus(device=0):
    """set of host CPUs on the device's NUMA node (aos2_device_local_cpus; empty when the platform does not say)"""
    L = lib()
    L.aos2_device_local_cpus.argtypes = [C.c_int, C.c_char_p, C.c_int]
    buf = C.create_string_buffer(8192)
    _check(L.aos2_device_local_cpus(int(device), buf, len(buf)))
    cpus = set()
    for part in buf.value.decode().split(","):
        part = part.strip()
        if not part:
            continue
        a, _, b = part.partition("-")
        cpus.update(range(int(a), int(b or a) + 1))
    return cpus


def bind_to_device_node(device=0):
    """sched_setaffinity of the calling thread (and the threads it creates from now on) to the device's local CPUs, intersected with
    the CPUs the process may use; returns the CPU count bound to, 0 when nothing was changed"""
    import os
    try:
        cpus = device_local_cpus(device) & os.sched_getaffinity(0)
    except (AosError, OSError):
        return 0
    if not cpus:
        return 0
    os.sched_setaffinity(0, cpus)
    return len(cpus)


class Extractor:
    """Mirror of ORBextractor (include/ORBextractor.h:45-111): ctor args, operator(), getters."""

    def __init__(self, nfeatures=1000, scale_factor=1.2, nlevels=8, ini_th=20, min_th=7, device=0):
        self.L = lib()
        h = C.c_void_p()
        _check(self.L.aos2_extractor_create(nfeatures, scale_factor, nlevels, ini_th, min_th, device, C.byref(h)))
        self.h = h
        self.nlevels = nlevels
        self.nfeatures = nfeatures

    def close(self):
        if getattr(self, "h", None):
            self.L.aos2_extractor_destroy(self.h)
            self.h = None

    __del__ = close

    def _arr(self, name, n, dt):
        ptr = getattr(self.L, "aos2_extractor_" + name)(self.h)
        return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dt).copy()

    # GetLevels / GetScaleFactor(s) / ... (include/ORBextractor.h:58-83)
    def GetLevels(self):
        return self.L.aos2_extractor_levels(self.h)

    def GetScaleFactor(self):
        return self.L.aos2_extractor_scale_factor(self.h)

    def GetScaleFactors(self):
        return self._arr("scale_factors", self.nlevels, np.float32)

    def GetInverseScaleFactors(self):
        return self._arr("inv_scale_factors", self.nlevels, np.float32)

    def GetScaleSigmaSquares(self):
        return self._arr("sigma2", self.nlevels, np.float32)

    def GetInverseScaleSigmaSquares(self):
        return self._arr("inv_sigma2", self.nlevels, np.float32)

    @property
    def features_per_level(self):
        return self._arr("features_per_level", self.nlevels, np.int32)

    @property
    def umax(self):
        return self._arr("umax", 16, np.int32)

    @property
    def max_keypoints(self):
        return self.L.aos2_extractor_max_keypoints(self.h)

    def max_keypoints_for(self, w, h):
        """capacity that always suffices for w x h images (wide images can exceed nfeatures + 3 per level)"""
        return self.L.aos2_extractor_max_keypoints_for(self.h, int(w), int(h))

    def __call__(self, image, mask=None):
        """operator()(image, mask, keypoints, descriptors): returns (keypoints[KP_DTYPE], desc[n,32])."""
        if image is None or image.size == 0:
            n = C.c_int(-1)
            _check(self.L.aos2_extractor_extract(self.h, None, 0, 0, 0, None, None, 0, C.byref(n)))
            return np.zeros(0, KP_DTYPE), np.zeros((0, 32), np.uint8)
        if image.dtype != np.uint8 or image.ndim != 2:
            raise AssertionError("image.type() == CV_8UC1")  # src/ORBextractor.cc:1050
        if image.strides[1] != 1:
            image = np.ascontiguousarray(image)
        h, w = image.shape
        cap = self.max_keypoints_for(w, h)
        kps = np.zeros(cap, KP_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        n = C.c_int(0)
        _check(self.L.aos2_extractor_extract(self.h, _p(image), w, h, image.strides[0], _p(kps), _p(desc), cap, C.byref(n)))
        return kps[: n.value].copy(), desc[: n.value].copy()

    def extract_batch(self, images):
        """host images [B, h, w] (any host memory; host_empty() arrays are uploaded by DMA) -> [(kps, desc)] * B"""
        images = np.ascontiguousarray(images, dtype=np.uint8)
        B, h, w = images.shape
        cap = self.max_keypoints_for(w, h)
        if getattr(self, "_out_key", None) != (B, cap):   # page-locked result buffers, reused between calls
            self._out_key, self._out = None, None
            self._out = (host_empty((B, cap), KP_DTYPE), host_empty((B, cap, 32), np.uint8))
            self._out_key = (B, cap)
        kps, desc = self._out
        n = np.zeros(B, np.int32)
        _check(self.L.aos2_extractor_extract_batch(self.h, _p(images), B, w, h, w, w * h, _p(kps), _p(desc), cap, _p(n)))
        return [(kps[b, : n[b]].copy(), desc[b, : n[b]].copy()) for b in range(B)]

    def extract_batch_device(self, d_imgs, batch, w, h, stride, image_stride, d_kps, d_desc, cap, d_nout):
        """raw device pointers (ints)"""
        _check(self.L.aos2_extractor_extract_batch_device(self.h, C.c_void_p(d_imgs), batch, w, h, stride, image_stride,
                                                          C.c_void_p(d_kps), C.c_void_p(d_desc), cap, C.c_void_p(d_nout)))

    def extract_batch_device_async(self, d_imgs, batch, w, h, stride, image_stride, d_kps, d_desc, cap, d_nout):
        """enqueue only (raw device pointers); results and errors are complete after wait()"""
        _check(self.L.aos2_extractor_extract_batch_device_async(self.h, C.c_void_p(d_imgs), batch, w, h, stride, image_stride,
                                                                C.c_void_p(d_kps), C.c_void_p(d_desc), cap, C.c_void_p(d_nout)))

    def pack_slots(self, batch, d_kps, d_desc, d_n, cap, d_slots, slot_bytes, stream=None):
        """aos2_extractor_pack_slots: device outputs -> fixed-size per-frame slots (sharding.slot_bytes layout)"""
        _check(self.L.aos2_extractor_pack_slots(self.h, batch, d_kps, d_desc, d_n, cap, d_slots, slot_bytes, stream))

    def stream_wait(self, stream):
        _check(self.L.aos2_extractor_stream_wait(self.h, stream))

    def wait_for_stream(self, stream):
        """the batches enqueued from now on run behind what `stream` holds so far (device-side)"""
        _check(self.L.aos2_extractor_wait_for_stream(self.h, stream))

    def wait(self):
        """complete every batch enqueued with extract_batch_device_async"""
        _check(self.L.aos2_extractor_wait(self.h))

    def pyramid_level(self, level, image=0, border=0):
        """mvImagePyramid[level] (include/ORBextractor.h:85)"""
        w, h = C.c_int(), C.c_int()
        _check(self.L.aos2_extractor_pyramid_level_size(self.h, level, C.byref(w), C.byref(h)))
        out = np.zeros((h.value + 2 * border, w.value + 2 * border), np.uint8)
        _check(self.L.aos2_extractor_pyramid_level(self.h, image, level, border, _p(out), out.strides[0]))
        return out

    def debug_candidates(self, level, image=0):
        n = C.c_int(0)
        _check(self.L.aos2_extractor_debug_candidates(self.h, image, level, None, None, None, 0, C.byref(n)))
        xs = np.zeros(max(n.value, 1), np.int16)
        ys = np.zeros(max(n.value, 1), np.int16)
        sc = np.zeros(max(n.value, 1), np.uint8)
        _check(self.L.aos2_extractor_debug_candidates(self.h, image, level, _p(xs), _p(ys), _p(sc), len(xs), C.byref(n)))
        return xs[: n.value], ys[: n.value], sc[: n.value]

    def debug_plan(self, w, h):
        """aos2_debug_extractor_plan: the plan for w x h images, computed on the host (no device) -> dict(levels int64 [nlevels][4] =
        w, h, pitch, off; cells int32 [n][6] = level, vx0, vy0, cw, ch, slot_off; pyr_bytes; slot_total)"""
        levels, totals, n = np.zeros((self.nlevels, 4), np.int64), np.zeros(2, np.int64), C.c_int(0)
        _check(self.L.aos2_debug_extractor_plan(self.h, int(w), int(h), _p(levels), None, 0, C.byref(n), _p(totals)))
        cells = np.zeros((max(n.value, 1), 6), np.int32)
        _check(self.L.aos2_debug_extractor_plan(self.h, int(w), int(h), _p(levels), _p(cells), len(cells), C.byref(n), _p(totals)))
        return dict(levels=levels, cells=cells[: n.value], pyr_bytes=int(totals[0]), slot_total=int(totals[1]))

    def set_chunks(self, n):
        _check(self.L.aos2_extractor_set_chunks(self.h, n))

    def last_timing(self):
        t = np.zeros(8, np.float32)
        _check(self.L.aos2_extractor_last_timing(self.h, _p(t), 8))
        return dict(pyramid=float(t[0]), fast=float(t[1]), compact=float(t[2]), octree=float(t[3]),
                    describe=float(t[4]), total_wall=float(t[5]), chunks=int(t[6]))

    def bench_fast(self, iters=20):
        ms = C.c_float(0)
        _check(self.L.aos2_extractor_bench_fast(self.h, iters, C.byref(ms)))
        return ms.value

    def bench_describe(self, iters=20):
        ms = C.c_float(0)
        _check(self.L.aos2_extractor_bench_describe(self.h, iters, C.byref(ms)))
        return ms.value


class Vocabulary:
    """ORBVocabulary (include/ORBVocabulary.h:31-32): loaders, transform(), score()."""

    def __init__(self, device=0):
        self.L = lib()
        h = C.c_void_p()
        _check(self.L.aos2_vocabulary_create(device, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.aos2_vocabulary_destroy(self.h)
            self.h = None

    __del__ = close

    def loadFromBinaryFile(self, path):
        return self.L.aos2_vocabulary_load_binary(self.h, str(path).encode()) == AOS2_OK

    def loadFromTextFile(self, path):
        return self.L.aos2_vocabulary_load_text(self.h, str(path).encode()) == AOS2_OK

    def saveToBinaryFile(self, path):
        _check(self.L.aos2_vocabulary_save_binary(self.h, str(path).encode()))

    def set_nodes(self, k, L, scoring, weighting, parent, desc, weight, is_leaf):
        parent = np.ascontiguousarray(parent, np.int32)
        desc = np.ascontiguousarray(desc, np.uint8)
        weight = np.ascontiguousarray(weight, np.float64)
        is_leaf = np.ascontiguousarray(is_leaf, np.uint8)
        _check(self.L.aos2_vocabulary_set_nodes(self.h, k, L, scoring, weighting, len(parent), _p(parent), _p(desc),
                                                _p(weight), _p(is_leaf)))

    def info(self):
        g = lambda n: getattr(self.L, "aos2_vocabulary_" + n)(self.h)  # noqa: E731
        return dict(k=g("k"), L=g("levels"), scoring=g("scoring"), weighting=g("weighting"), nodes=g("nodes"),
                    words=int(g("size")))

    def nodes(self):
        """m_nodes, root included -> dict(parent, is_leaf (= no children), word_id, weight, desc)"""
        n = self.L.aos2_vocabulary_nodes(self.h)
        r = dict(parent=np.zeros(n, np.int32), is_leaf=np.zeros(n, np.uint8), word_id=np.zeros(n, np.uint32),
                 weight=np.zeros(n, np.float64), desc=np.zeros((n, 32), np.uint8))
        _check(self.L.aos2_vocabulary_get_nodes(self.h, *[_p(r[k]) for k in ("parent", "is_leaf", "word_id", "weight", "desc")]))
        return r

    def empty(self):
        return bool(self.L.aos2_vocabulary_empty(self.h))

    def transform(self, desc, levelsup=4):
        """-> dict(bow_word, bow_value, fv_node, fv_off, fv_idx, word_of, node_of)"""
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n = len(desc)
        m = max(n, 1)
        bw, bv = np.zeros(m, np.uint32), np.zeros(m, np.float64)
        fn, fo, fi = np.zeros(m, np.int32), np.zeros(n + 2, np.int32), np.zeros(m, np.int32)
        wo, no = np.zeros(m, np.uint32), np.zeros(m, np.uint32)
        nb, nf = C.c_int(0), C.c_int(0)
        _check(self.L.aos2_vocabulary_transform(self.h, _p(desc), n, levelsup, _p(bw), _p(bv), C.byref(nb), _p(fn), _p(fo),
                                                _p(fi), C.byref(nf), _p(wo), _p(no)))
        nb, nf = nb.value, nf.value
        return dict(bow_word=bw[:nb].copy(), bow_value=bv[:nb].copy(), fv_node=fn[:nf].copy(), fv_off=fo[: nf + 1].copy(),
                    fv_idx=fi[: fo[nf]].copy(), word_of=wo[:n].copy(), node_of=no[:n].copy())

    def transform_device(self, batch, d_desc, d_n, cap, levelsup, d_bw, d_bv, d_nb, d_fn, d_fo, d_fi, d_nf, d_wo=0, d_no=0):
        """raw device pointers (ints); returns the device time in ms"""
        V = C.c_void_p
        _check(self.L.aos2_vocabulary_transform_device(self.h, batch, V(d_desc), V(d_n), cap, levelsup, V(d_bw), V(d_bv),
                                                       V(d_nb), V(d_fn), V(d_fo), V(d_fi), V(d_nf), V(d_wo or None),
                                                       V(d_no or None)))
        return float(self.L.aos2_vocabulary_last_device_ms(self.h))

    def stream(self):
        return self.L.aos2_vocabulary_stream(self.h)

    def score(self, a, b):
        w1, v1 = np.ascontiguousarray(a["bow_word"], np.uint32), np.ascontiguousarray(a["bow_value"], np.float64)
        w2, v2 = np.ascontiguousarray(b["bow_word"], np.uint32), np.ascontiguousarray(b["bow_value"], np.float64)
        s = C.c_double(0)
        _check(self.L.aos2_vocabulary_score(self.h, _p(w1), _p(v1), len(w1), _p(w2), _p(v2), len(w2), C.byref(s)))
        return s.value


# ---- KeyFrameDatabase (include/aos2.h: aos2_kfdb_*, aos2_debug_kfdb_host)
class _KfdbQuery(C.Structure):
    _fields_ = [("mode", C.c_int32), ("slot", C.c_int32), ("words", C.c_void_p), ("values", C.c_void_p), ("n_words", C.c_int32),
                ("on_device", C.c_int32), ("min_score", C.c_float), ("n_excluded", C.c_int32), ("excluded", C.c_void_p)]


class _KfdbResult(C.Structure):
    _fields_ = [("candidates", C.c_void_p), ("cap_candidates", C.c_int32)] + \
               [(k, C.c_int32) for k in ("n_candidates", "n_sharing", "max_common_words", "min_common_words", "n_scored", "n_matched")] + \
               [("best_acc_score", C.c_float), ("scored_slot", C.c_void_p), ("scored_words", C.c_void_p), ("scored_score", C.c_void_p),
                ("cap_scored", C.c_int32), ("sharing_slot", C.c_void_p), ("sharing_words", C.c_void_p), ("cap_sharing", C.c_int32)]


_KFDB_SCALARS = ("n_candidates", "n_sharing", "max_common_words", "min_common_words", "n_scored", "n_matched")
_KFDB_LISTS = (("candidates", "candidates", np.int32, "n_candidates"), ("scored_slot", "scored", np.int32, "n_scored"),
               ("scored_words", "scored", np.int32, "n_scored"), ("scored_score", "scored", np.float32, "n_scored"),
               ("sharing_slot", "sharing", np.int32, "n_sharing"), ("sharing_words", "sharing", np.int32, "n_sharing"))


class KeyFrameDatabase:
    """KeyFrameDatabase (include/KeyFrameDatabase.h:42-70) over slots: the BowVectors resident on the device, the candidates of
    DetectLoopCandidates / DetectRelocalizationCandidates for a batch of queries in one call."""
    LOOP, RELOC = 0, 1

    def __init__(self, voc: Vocabulary, device=0):
        self.L = lib()
        h = C.c_void_p()
        _check(self.L.aos2_kfdb_create(voc.h, device, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.aos2_kfdb_destroy(self.h)
            self.h = None

    __del__ = close

    def put(self, words, values):
        w, v = np.ascontiguousarray(words, np.uint32), np.ascontiguousarray(values, np.float64)
        if len(w) != len(v):
            raise ValueError("words and values differ in length")
        s = C.c_int32(-1)
        _check(self.L.aos2_kfdb_put(self.h, _p(w), _p(v), len(w), C.byref(s)))
        return s.value

    def put_device(self, voc, batch, d_words, d_values, d_n_bow, cap):
        """rows as Vocabulary.transform_device wrote them (raw device pointers) -> the slots"""
        slots = np.full(max(batch, 1), -1, np.int32)
        V = C.c_void_p
        _check(self.L.aos2_kfdb_put_device(self.h, voc.h if voc is not None else None, batch, V(d_words), V(d_values), V(d_n_bow),
                                           cap, _p(slots)))
        return slots[:batch]

    def add(self, slot):
        _check(self.L.aos2_kfdb_add(self.h, slot))

    def erase(self, slot):
        _check(self.L.aos2_kfdb_erase(self.h, slot))

    def drop(self, slot):
        _check(self.L.aos2_kfdb_drop(self.h, slot))

    def clear(self):
        _check(self.L.aos2_kfdb_clear(self.h))

    def size(self):
        return self.L.aos2_kfdb_size(self.h)

    def arena_capacity(self):
        return int(self.L.aos2_kfdb_arena_capacity(self.h))

    def last_device_ms(self):
        return float(self.L.aos2_kfdb_last_device_ms(self.h))

    def set_neighbours(self, slots, neigh):
        s = np.ascontiguousarray(slots, np.int32)
        n = np.ascontiguousarray(neigh, np.int32).reshape(len(s), 10)
        _check(self.L.aos2_kfdb_set_neighbours(self.h, len(s), _p(s), _p(n)))

    @staticmethod
    def _query(Q, q, keep):
        """q: dict(mode, min_score, excluded) with slot=, or words= / values= (host), or d_words= / d_values= / n_words= (device)"""
        Q.mode, Q.min_score, Q.slot = int(q.get("mode", 0)), float(q.get("min_score", 0.0)), int(q.get("slot", -1))
        if "d_words" in q:
            Q.words, Q.values, Q.n_words, Q.on_device = q["d_words"], q["d_values"], int(q["n_words"]), 1
        elif "words" in q:
            w, v = np.ascontiguousarray(q["words"], np.uint32), np.ascontiguousarray(q["values"], np.float64)
            keep += [w, v]
            Q.words, Q.values, Q.n_words = w.ctypes.data, v.ctypes.data, int(q.get("n_words", len(w)))
        ex = q.get("excluded")
        if ex is not None:
            ex = np.ascontiguousarray(ex, np.int32)
            keep.append(ex)
            Q.excluded, Q.n_excluded = ex.ctypes.data, int(q.get("n_excluded", len(ex)))

    def detect_args(self, queries, lists=("scored", "sharing"), caps=None, sentinel=None):
        """the aos2_kfdb_query_t / aos2_kfdb_result_t arrays of a detect call -> (Q, R, what they point to, the result arrays per query).
        caps: dict(candidates=, scored=, sharing=), default the number of added slots; `sentinel` pre-fills structs and buffers."""
        nq = len(queries)
        Q, R, keep, outs = (_KfdbQuery * max(nq, 1))(), (_KfdbResult * max(nq, 1))(), [], []
        n_added = self.size()
        caps = dict(caps or {})
        if sentinel is not None:
            C.memset(R, sentinel, C.sizeof(R))
        for i, q in enumerate(queries):
            self._query(Q[i], q, keep)
            o = {}
            for name, group, dt, _ in _KFDB_LISTS:
                if group != "candidates" and group not in lists:
                    setattr(R[i], name, None)
                    continue
                cap = int(caps.get(group, n_added))
                o[name] = np.zeros(max(cap, 1), dt) if sentinel is None else np.frombuffer(bytes([sentinel]) * (max(cap, 1) * 4), dt).copy()
                setattr(R[i], name, o[name].ctypes.data)
                setattr(R[i], "cap_" + group, cap)
            outs.append(o)
        return Q, R, keep, outs

    def detect(self, queries, host=False, lists=("scored", "sharing"), caps=None, sentinel=None):
        """aos2_kfdb_detect (host=True: aos2_debug_kfdb_host) -> one dict per query: the fields of aos2_kfdb_result_t, lists cut to
        their counts.  The result structs and buffers are kept in self.last (structs, arrays, the structs' bytes before the call) for a
        caller that expects a refusal."""
        nq = len(queries)
        Q, R, keep, outs = self.detect_args(queries, lists, caps, sentinel)
        self.last = (R, outs, bytes(R))
        _check((self.L.aos2_debug_kfdb_host if host else self.L.aos2_kfdb_detect)(self.h, Q, R, nq))
        res = []
        for i in range(nq):
            d = {k: int(getattr(R[i], k)) for k in _KFDB_SCALARS}
            d["best_acc_score"] = np.float32(R[i].best_acc_score)
            for name, group, dt, cnt in _KFDB_LISTS:
                if name in outs[i]:
                    d[name] = outs[i][name][: d[cnt]].copy()
            res.append(d)
        return res

    def scores(self, query, slots, host=False):
        """aos2_kfdb_scores (host=True: its host tap): the loop of LoopClosing::DetectLoop -> (float32 scores, their minimum from 1)"""
        Q, keep = _KfdbQuery(), []
        self._query(Q, query, keep)
        s = np.ascontiguousarray(slots, np.int32)
        out, mn = np.zeros(max(len(s), 1), np.float32), C.c_float(-1.0)
        f = self.L.aos2_debug_kfdb_scores_host if host else self.L.aos2_kfdb_scores
        _check(f(self.h, C.byref(Q), _p(s), len(s), _p(out), C.byref(mn)))
        return out[: len(s)], np.float32(mn.value)


# ---- planner visibility (include/aos2.h: aos2_vis_*, aos2_debug_visibility_*host)
class VisCamera(C.Structure):
    """aos2_vis_camera_t"""
    _fields_ = [(k, C.c_float) for k in ("fx", "fy", "cx", "cy", "min_x", "max_x", "min_y", "max_y", "max_dist", "min_dist")] + \
               [("feature_threshold", C.c_int32), ("T_sw", C.c_float * 16), ("T_bc", C.c_float * 16)]


class Visibility:
    """camera (include/camera.h:51-129) for batches of states: the planner's map resident on the device, countVisible for ns
    states in one call, MotionCostCamera for many motions and AdvanceStepCamera for a trajectory.  host=True runs the library's
    own serial routine (aos2_debug_visibility_*host) instead."""
    CAMERA_MAP, CAMERA_PLAIN = 0, 1

    def __init__(self, device=0):
        self.L = lib()
        h = C.c_void_p()
        _check(self.L.aos2_vis_create(device, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.aos2_vis_destroy(self.h)
            self.h = None

    __del__ = close

    @staticmethod
    def camera_default(which=0):
        cam = VisCamera()
        _check(lib().aos2_vis_camera_default(which, C.byref(cam)))
        return cam

    @staticmethod
    def gate_tile():
        """(points a workgroup of the gate kernel takes, states of its tile)"""
        p, s = C.c_int(0), C.c_int(0)
        lib().aos2_vis_gate_tile(C.byref(p), C.byref(s))
        return p.value, s.value

    def set_camera(self, cam: VisCamera):
        _check(self.L.aos2_vis_set_camera(self.h, C.byref(cam)))

    def set_map(self, xyz, upper, lower, max_range, min_range, found_ratio):
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        rest = [np.ascontiguousarray(a, np.float32).reshape(-1) for a in (upper, lower, max_range, min_range, found_ratio)]
        if any(len(a) != len(xyz) for a in rest):
            raise ValueError("the map's arrays differ in length")
        _check(self.L.aos2_vis_set_map(self.h, len(xyz), _p(xyz), *[_p(a) for a in rest]))

    def map_size(self):
        return self.L.aos2_vis_map_size(self.h)

    def last_device_ms(self):
        return float(self.L.aos2_vis_last_device_ms(self.h))

    def _count(self, f, arr, ns, want_sum, want_mask):
        words = (self.map_size() + 63) // 64
        count = np.zeros(ns, np.int32)
        s = np.zeros(ns, np.float32) if want_sum else None
        m = np.zeros((ns, words), np.uint64) if want_mask else None
        _check(f(self.h, ns, _p(arr), _p(count), _p(s) if want_sum else None, _p(m) if want_mask else None))
        return dict(count=count, sum=s, mask=m)

    def count(self, states, sum=True, mask=True, host=False):
        """aos2_vis_count: states [ns][3] = x, y, theta -> dict(count int32 [ns], sum float32 [ns] | None, mask uint64 [ns][words] | None)"""
        st = np.ascontiguousarray(states, np.float32).reshape(-1, 3)
        return self._count(self.L.aos2_debug_visibility_host if host else self.L.aos2_vis_count, st, len(st), sum, mask)

    def count_poses(self, T_wb, sum=True, mask=True, host=False):
        """aos2_vis_count_poses: T_wb [ns][4][4]"""
        T = np.ascontiguousarray(T_wb, np.float32).reshape(-1, 16)
        return self._count(self.L.aos2_debug_visibility_poses_host if host else self.L.aos2_vis_count_poses, T, len(T), sum, mask)

    def motion_costs(self, motions, thres=-1, host=False):
        """aos2_vis_motion_costs: motions = a list of [size][3] state arrays -> float64 [nm]"""
        ms = [np.asarray(m, np.float32).reshape(-1, 3) for m in motions]
        off = np.cumsum([0] + [len(m) for m in ms]).astype(np.int32)
        st = np.ascontiguousarray(np.concatenate(ms) if ms else np.zeros((0, 3)), np.float32)
        return self.motion_costs_raw(off, st, thres, host)

    def motion_costs_raw(self, offsets, states, thres=-1, host=False):
        off, st = np.ascontiguousarray(offsets, np.int32), np.ascontiguousarray(states, np.float32)
        cost = np.zeros(max(len(off) - 1, 0), np.float64)
        f = self.L.aos2_debug_visibility_motion_costs_host if host else self.L.aos2_vis_motion_costs
        _check(f(self.h, len(off) - 1, _p(off), _p(st), int(thres), _p(cost)))
        return cost

    def advance(self, states, thres=-1, host=False):
        """aos2_vis_advance: the last index of the leading run of states with count > thres, -1 if the first one fails"""
        st = np.ascontiguousarray(states, np.float32).reshape(-1, 3)
        idx = C.c_int32(-2)
        f = self.L.aos2_debug_visibility_advance_host if host else self.L.aos2_vis_advance
        _check(f(self.h, len(st), _p(st), int(thres), C.byref(idx)))
        return idx.value


# ---- planner motion checks (include/aos2.h: aos2_svc_*, aos2_debug_svc_*host, aos2_debug_tw_math)
class SvcParams(C.Structure):
    """aos2_svc_params_t"""
    _fields_ = [(k, C.c_double) for k in ("turn_radius", "robot_r", "dt", "min_x", "max_x", "min_y", "max_y", "max_dist_heuristic")] + \
               [("start", C.c_double * 3), ("heuristic", C.c_int32), ("feature_threshold", C.c_int32)]


class _SvcMotionsOut(C.Structure):
    """aos2_svc_motions_out_t"""
    _fields_ = [(k, C.c_void_p) for k in ("path_valid", "type", "t", "m", "n_states", "valid", "first_invalid", "cost_length",
                                          "cost_camera", "offsets", "states")] + \
               [("states_capacity", C.c_int64), ("states_needed", C.c_int64)]


class _OwnedVisibility(Visibility):
    """the visibility handle a StateValidChecker owns: it dies with its owner"""

    def __init__(self, owner, h):
        self.L, self.h, self.owner = lib(), C.c_void_p(h), owner

    def close(self):
        self.h = None

    __del__ = close


class StateValidChecker:
    """StateValidChecker (include/StateValidChecker.h:47-150) for batches: the obstacles and the camera's map resident on the
    device, isValid for ns states and checkMotionTW / reconstructMotionTW / MotionCost for nm pairs of states in one call.
    host=True runs the library's own serial routine (aos2_debug_svc_*host) instead.  `vis` is the camera base: set_camera and
    set_map go there."""
    MOTION_FIELDS = (("path_valid", np.uint8, 1), ("type", np.int32, 1), ("t", np.float64, 3), ("m", np.int32, 3), ("n_states", np.int32, 1),
                     ("valid", np.uint8, 1), ("first_invalid", np.int32, 1), ("cost_length", np.float64, 1), ("cost_camera", np.float64, 1))

    def __init__(self, device=0):
        self.L = lib()
        h = C.c_void_p()
        _check(self.L.aos2_svc_create(device, C.byref(h)))
        self.h = h
        self.vis = _OwnedVisibility(self, self.L.aos2_svc_vis(h))

    def close(self):
        if getattr(self, "h", None):
            self.vis.close()
            self.L.aos2_svc_destroy(self.h)
            self.h = None

    __del__ = close

    @staticmethod
    def params_default():
        p = SvcParams()
        _check(lib().aos2_svc_params_default(C.byref(p)))
        return p

    @staticmethod
    def collide_tile():
        """(obstacles a workgroup of the collision kernel stages at a time, states of its tile)"""
        o, s = C.c_int(0), C.c_int(0)
        lib().aos2_svc_collide_tile(C.byref(o), C.byref(s))
        return o.value, s.value

    def set_params(self, p: SvcParams):
        _check(self.L.aos2_svc_set_params(self.h, C.byref(p)))

    def set_obstacles(self, xy, obs_r=0.1):
        xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
        _check(self.L.aos2_svc_set_obstacles(self.h, len(xy), _p(xy), float(obs_r)))

    def last_device_ms(self):
        return float(self.L.aos2_svc_last_device_ms(self.h))

    def valid(self, states, host=False):
        """aos2_svc_valid: states [ns][3] float64 -> dict(valid uint8 [ns], collision_free uint8 [ns], count int32 [ns])"""
        st = np.ascontiguousarray(states, np.float64).reshape(-1, 3)
        out = dict(valid=np.zeros(len(st), np.uint8), collision_free=np.zeros(len(st), np.uint8), count=np.zeros(len(st), np.int32))
        f = self.L.aos2_debug_svc_valid_host if host else self.L.aos2_svc_valid
        _check(f(self.h, len(st), _p(st), _p(out["valid"]), _p(out["collision_free"]), _p(out["count"])))
        return out

    def motions(self, q1, q2, states=True, capacity=None, host=False):
        """aos2_svc_motions: q1, q2 [nm][3] float64 -> a dict of the per-motion arrays (MOTION_FIELDS) and, with states, offsets
        int32 [nm + 1] and states float64 [total][3].  capacity: the rows of the states buffer (default: asked for with a first
        call).  A buffer too small raises AosError(AOS2_ERR_CAPACITY) with .needed = the rows needed."""
        a = np.ascontiguousarray(q1, np.float64).reshape(-1, 3)
        b = np.ascontiguousarray(q2, np.float64).reshape(-1, 3)
        if len(a) != len(b):
            raise ValueError("q1 and q2 differ in length")
        nm = len(a)
        f = self.L.aos2_debug_svc_motions_host if host else self.L.aos2_svc_motions
        out = {k: np.zeros((nm, w) if w > 1 else nm, dt) for k, dt, w in self.MOTION_FIELDS}
        O = _SvcMotionsOut()
        for k in out:
            setattr(O, k, out[k].ctypes.data)
        if states:
            if capacity is None:      # the size first: a call that asks for no states reports the rows needed
                probe = _SvcMotionsOut()
                _check(f(self.h, nm, _p(a), _p(b), C.byref(probe)))
                capacity = probe.states_needed
            out["offsets"] = np.zeros(nm + 1, np.int32)
            buf = np.zeros((max(int(capacity), 1), 3), np.float64)
            O.offsets, O.states, O.states_capacity = out["offsets"].ctypes.data, buf.ctypes.data, int(capacity)
        st = f(self.h, nm, _p(a), _p(b), C.byref(O))
        if st == AOS2_ERR_CAPACITY:
            e = AosError(st, lib().aos2_last_error().decode(errors="replace"))
            e.needed = int(O.states_needed)
            raise e
        _check(st)
        if states:
            out["states"] = buf[: int(O.states_needed)]
        return out


# ---- Tracking::UpdateLocalMap for frame batches (include/aos2.h: aos2_local_map_*, aos2_frames_update_local_map)
_LM_I32 = ("point_nobs", "obs_off", "obs_kf", "kf_mp_off", "kf_mp", "kf_best", "kf_child_off", "kf_child", "kf_parent")
_LM_U8 = ("point_bad", "kf_bad")


class _LocalMapGraph(C.Structure):
    """aos2_local_map_graph_t"""
    _fields_ = [("n_points", C.c_int32), ("point_bad", C.c_void_p), ("point_nobs", C.c_void_p), ("obs_off", C.c_void_p),
                ("obs_kf", C.c_void_p), ("n_keyframes", C.c_int32), ("kf_bad", C.c_void_p), ("kf_mp_off", C.c_void_p),
                ("kf_mp", C.c_void_p), ("kf_best", C.c_void_p), ("kf_child_off", C.c_void_p), ("kf_child", C.c_void_p),
                ("kf_parent", C.c_void_p)]


def _local_map_graph(g, keep):
    """a graph dict (the fields of aos2_local_map_graph_t; an array may be None = NULL) -> the struct; `keep` holds the arrays"""
    s = _LocalMapGraph()
    s.n_points, s.n_keyframes = int(g["n_points"]), int(g["n_keyframes"])
    for k in _LM_I32 + _LM_U8:
        a = g.get(k)
        if a is None:
            setattr(s, k, None)
            continue
        a = np.ascontiguousarray(a, np.uint8 if k in _LM_U8 else np.int32).reshape(-1)
        keep.append(a)
        setattr(s, k, a.ctypes.data if a.size else keep[0].ctypes.data)   # (an empty array is not NULL)
    return s


# ---- LocalMapping::KeyFrameCulling over the resident graph (include/aos2.h: aos2_local_map_set_culling_view and friends)
KFC_KEPT, KFC_CULLED, KFC_DEFERRED, KFC_SKIPPED = range(4)
_KFC_FIELDS = (("obs_idx", np.int32), ("kf_octave", np.int8), ("kf_depth", np.float32), ("kf_stereo", np.uint8),
               ("kf_th_depth", np.float32), ("kf_flags", np.uint8))


class _KfCullingView(C.Structure):
    """aos2_kf_culling_view_t"""
    _fields_ = [(k, C.c_void_p) for k, _ in _KFC_FIELDS]


def _kf_culling_view(v, keep):
    """a view dict (the fields of aos2_kf_culling_view_t; an array may be None = NULL) -> the struct; `keep` holds the arrays"""
    s = _KfCullingView()
    for k, dt in _KFC_FIELDS:
        a = v.get(k)
        if a is None:
            setattr(s, k, None)
            continue
        a = np.ascontiguousarray(a, dt).reshape(-1)
        keep.append(a)
        setattr(s, k, a.ctypes.data if a.size else keep[0].ctypes.data)   # (an empty array is not NULL)
    return s


_LMD_I32 = ("point_row", "point_nobs", "obs_off", "obs_kf", "kf_mp_row", "kf_mp_off", "kf_mp", "kf_link_row", "kf_best", "kf_child_off",
            "kf_child", "kf_parent")
_LMD_U8 = ("point_bad", "kf_bad")


class _LocalMapDelta(C.Structure):
    """aos2_local_map_delta_t"""
    _fields_ = [("n_points", C.c_int32), ("n_keyframes", C.c_int32),
                ("n_point_rows", C.c_int32), ("point_row", C.c_void_p), ("point_bad", C.c_void_p), ("point_nobs", C.c_void_p),
                ("obs_off", C.c_void_p), ("obs_kf", C.c_void_p),
                ("n_kf_mp_rows", C.c_int32), ("kf_mp_row", C.c_void_p), ("kf_mp_off", C.c_void_p), ("kf_mp", C.c_void_p),
                ("n_kf_link_rows", C.c_int32), ("kf_link_row", C.c_void_p), ("kf_bad", C.c_void_p), ("kf_best", C.c_void_p),
                ("kf_child_off", C.c_void_p), ("kf_child", C.c_void_p), ("kf_parent", C.c_void_p), ("view", C.c_void_p)]


def _local_map_delta(d, keep):
    """a delta dict (the fields of aos2_local_map_delta_t; an array may be None = NULL, `view` a view dict or None; the three row
    counts default to the lengths of their row lists) -> the struct; `keep` holds the arrays and the view struct"""
    s = _LocalMapDelta()
    s.n_points, s.n_keyframes = int(d["n_points"]), int(d["n_keyframes"])
    for k in _LMD_I32 + _LMD_U8:
        a = d.get(k)
        if a is None:
            setattr(s, k, None)
            continue
        a = np.ascontiguousarray(a, np.uint8 if k in _LMD_U8 else np.int32).reshape(-1)
        keep.append(a)
        setattr(s, k, a.ctypes.data if a.size else keep[0].ctypes.data)   # (an empty array is not NULL)
    for n, rows in (("n_point_rows", "point_row"), ("n_kf_mp_rows", "kf_mp_row"), ("n_kf_link_rows", "kf_link_row")):
        setattr(s, n, int(d[n]) if n in d else (0 if d.get(rows) is None else len(d[rows])))
    if d.get("view") is not None:
        v = _kf_culling_view(d["view"], keep)
        keep.append(v)
        s.view = C.addressof(v)
    return s


def _kf_culling_call(fn, first, monocular, cand, bad_cap):
    """the arguments that aos2_local_map_keyframe_culling and its host tap share -> dict(status uint8 [n], n_mps, n_redundant int32
    [n], n_bad_points int, bad_points int32 [bad_cap + 1]: one element more than the call may write, preset to -7)"""
    cand = np.ascontiguousarray(cand, np.int32).reshape(-1)
    n = len(cand)
    status = np.full(max(n, 1), 255, np.uint8)
    n_mps, n_red = np.full(max(n, 1), -7, np.int32), np.full(max(n, 1), -7, np.int32)
    bad = np.full(int(bad_cap) + 1, -7, np.int32)
    nb = C.c_int32(-7)
    _check(fn(*first, int(bool(monocular)), n, _p(cand), _p(status), _p(n_mps), _p(n_red), _p(bad), int(bad_cap), C.byref(nb)))
    return dict(status=status[:n], n_mps=n_mps[:n], n_redundant=n_red[:n], n_bad_points=int(nb.value), bad_points=bad)


CONNECTIONS_TH = 15


def _update_connections_call(fn, first, th, kf, mp, conn_cap, ordered_cap, mp_cap=None):
    """the arguments that aos2_local_map_update_connections and its host tap share.  kf: the rows; mp: None (the resident matches)
    or one sequence of point rows per keyframe -> dict(n_conn, n_ordered int32 [n], conn_kf, conn_w int32 [n][conn_cap], ordered_kf,
    ordered_w int32 [n][ordered_cap], guard: the word behind each of the six arrays, preset to -7).  A capacity of 0 passes NULL."""
    kf = np.ascontiguousarray(kf, np.int32).reshape(-1)
    n = len(kf)
    n_mp = mp2 = None
    if mp is not None:
        if len(mp) != n:
            raise ValueError("one list of matches per keyframe")
        n_mp = np.array([len(x) for x in mp] + [0], np.int32)
        mp_cap = max(1, int(n_mp.max())) if mp_cap is None else int(mp_cap)
        mp2 = np.full((max(n, 1), mp_cap), -1, np.int32)
        for k, x in enumerate(mp):
            mp2[k, :min(len(x), mp_cap)] = np.asarray(x, np.int32)[:mp_cap]
    else:
        mp_cap = 0
    conn_cap, ordered_cap = int(conn_cap), int(ordered_cap)
    flat = {k: np.full(n * c + 1, -7, np.int32) for k, c in (("n_conn", 1), ("n_ordered", 1), ("conn_kf", conn_cap), ("conn_w", conn_cap),
                                                             ("ordered_kf", ordered_cap), ("ordered_w", ordered_cap))}

    def arg(k, c):
        return _p(flat[k]) if c > 0 else None
    _check(fn(*first, int(th), n, _p(kf), None if mp is None else _p(n_mp), None if mp is None else _p(mp2), mp_cap,
              _p(flat["n_conn"]), arg("conn_kf", conn_cap), arg("conn_w", conn_cap), conn_cap,
              _p(flat["n_ordered"]), arg("ordered_kf", ordered_cap), arg("ordered_w", ordered_cap), ordered_cap))
    out = dict(n_conn=flat["n_conn"][:n], n_ordered=flat["n_ordered"][:n], guard={k: int(a[-1]) for k, a in flat.items()})
    for k, c in (("conn_kf", conn_cap), ("conn_w", conn_cap), ("ordered_kf", ordered_cap), ("ordered_w", ordered_cap)):
        out[k] = flat[k][:n * c].reshape(n, c)
    return out


class LocalMap:
    """The covisibility graph resident on the device and Tracking::UpdateLocalMap (src/Tracking.cc:1375-1519) for the frames of a
    capi.Frames batch.  A graph is a dict with the fields of aos2_local_map_graph_t (numpy arrays, CSR offsets)."""

    def __init__(self, device=0):
        self.L = lib()
        h = C.c_void_p()
        _check(self.L.aos2_local_map_create(device, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.aos2_local_map_destroy(self.h)
            self.h = None

    __del__ = close

    def set(self, graph, ok=(AOS2_OK,)):
        """aos2_local_map_set; `ok`: the return values that do not raise (a machine without a device keeps a checked graph and
        returns AOS2_ERR_NO_DEVICE)"""
        keep = [np.zeros(1, np.int32)]
        s = _local_map_graph(graph, keep)
        return _check(self.L.aos2_local_map_set(self.h, C.byref(s)), ok)

    def graph(self):
        """the handle's snapshot as a graph dict (copies)"""
        s = _LocalMapGraph()
        _check(self.L.aos2_local_map_get(self.h, C.byref(s)))
        npnt, nk = s.n_points, s.n_keyframes
        g = dict(n_points=npnt, n_keyframes=nk)

        def arr(p, n, dt):
            if not n:
                return np.zeros(0, dt)
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8 if dt == np.uint8 else C.c_int32)), (n,)).astype(dt, copy=True)

        for k, n in (("obs_off", npnt + 1), ("kf_mp_off", nk + 1), ("kf_child_off", nk + 1), ("point_nobs", npnt), ("kf_parent", nk),
                     ("kf_best", nk * 10)):
            g[k] = arr(getattr(s, k), n, np.int32)
        g["point_bad"], g["kf_bad"] = arr(s.point_bad, npnt, np.uint8), arr(s.kf_bad, nk, np.uint8)
        for k, off in (("obs_kf", "obs_off"), ("kf_mp", "kf_mp_off"), ("kf_child", "kf_child_off")):
            g[k] = arr(getattr(s, k), int(g[off][-1]), np.int32)
        return g

    def view(self):
        """the handle's culling view as a view dict (copies, parallel to graph()), None if it holds none"""
        s, v = _LocalMapGraph(), _KfCullingView()
        _check(self.L.aos2_local_map_get(self.h, C.byref(s)))
        has = C.c_int32(0)
        _check(self.L.aos2_local_map_get_culling_view(self.h, C.byref(v), C.byref(has)))
        if not has.value:
            return None
        nk = s.n_keyframes
        n_obs = int(np.ctypeslib.as_array(C.cast(s.obs_off, C.POINTER(C.c_int32)), (s.n_points + 1,))[-1])
        n_mp = int(np.ctypeslib.as_array(C.cast(s.kf_mp_off, C.POINTER(C.c_int32)), (nk + 1,))[-1])
        lens = dict(obs_idx=n_obs, kf_octave=n_mp, kf_depth=n_mp, kf_stereo=n_mp, kf_th_depth=nk, kf_flags=nk)
        out = {}
        for k, dt in _KFC_FIELDS:
            n, nbytes = lens[k], lens[k] * np.dtype(dt).itemsize
            out[k] = np.frombuffer(C.string_at(getattr(v, k), nbytes), dt).copy() if n else np.zeros(0, dt)
        return out

    def apply(self, delta, ok=(AOS2_OK,)):
        """aos2_local_map_apply: a delta is a dict with the fields of aos2_local_map_delta_t (`view`: a view dict or None); `ok` as in
        set()"""
        keep = [np.zeros(1, np.int32)]
        s = _local_map_delta(delta, keep)
        return _check(self.L.aos2_local_map_apply(self.h, C.byref(s)), ok)

    def apply_host(self, delta, ok=(AOS2_OK,)):
        """aos2_debug_local_map_apply_host: the rebuild forced onto the host, the device copy marked dirty"""
        keep = [np.zeros(1, np.int32)]
        s = _local_map_delta(delta, keep)
        return _check(self.L.aos2_debug_local_map_apply_host(self.h, C.byref(s)), ok)

    def last_apply(self):
        """aos2_local_map_last_apply -> dict(path 0 host / 1 device, reallocated, device_ms, bytes uploaded)"""
        path, re, ms = C.c_int32(-1), C.c_int32(0), C.c_float(-1)
        _check(self.L.aos2_local_map_last_apply(self.h, C.byref(path), C.byref(re), C.byref(ms)))
        return dict(path=path.value, reallocated=re.value, device_ms=float(ms.value),
                    bytes=int(self.L.aos2_local_map_last_apply_bytes(self.h)))

    def debug_apply_tile(self, rows=0):
        _check(self.L.aos2_local_map_debug_apply_tile(self.h, int(rows)))

    def update(self, frames, d_local, local_cap, d_n_local, d_local_kfs, kf_cap, d_n_local_kfs, d_ref_kf):
        """aos2_frames_update_local_map: device addresses (ints); enqueued on the batch's stream"""
        _check(self.L.aos2_frames_update_local_map(frames.h, self.h, d_local, int(local_cap), d_n_local, d_local_kfs, int(kf_cap),
                                                   d_n_local_kfs, d_ref_kf))

    def stats(self, frames, d_stats, d_found_inc=0, stereo=False, only_tracking=False):
        """aos2_frames_track_local_map_stats: d_stats int32 [batch][3], d_found_inc int32 [n_points] or 0"""
        _check(self.L.aos2_frames_track_local_map_stats(frames.h, self.h, int(bool(stereo)), int(bool(only_tracking)), d_stats,
                                                        d_found_inc or None))

    def debug_limits(self, scratch_bytes=0, lds_keyframes=-1):
        _check(self.L.aos2_local_map_debug_limits(self.h, int(scratch_bytes), int(lds_keyframes)))

    def last_groups(self):
        return self.L.aos2_local_map_last_groups(self.h)

    def set_culling_view(self, view, ok=(AOS2_OK,)):
        """aos2_local_map_set_culling_view: a view is a dict with the fields of aos2_kf_culling_view_t; `ok` as in set()"""
        keep = [np.zeros(1, np.int32)]
        s = _kf_culling_view(view, keep)
        return _check(self.L.aos2_local_map_set_culling_view(self.h, C.byref(s)), ok)

    def keyframe_culling(self, cand, monocular=False, bad_cap=None):
        """aos2_local_map_keyframe_culling (LocalMapping::KeyFrameCulling, src/LocalMapping.cc:636-700) on the device; bad_cap
        defaults to the number of points of the handle's graph -> the dict of _kf_culling_call"""
        if bad_cap is None:
            s = _LocalMapGraph()
            _check(self.L.aos2_local_map_get(self.h, C.byref(s)))
            bad_cap = s.n_points
        return _kf_culling_call(self.L.aos2_local_map_keyframe_culling, (self.h,), monocular, cand, bad_cap)

    def debug_culling_rounds(self, rounds=0):
        _check(self.L.aos2_local_map_debug_culling_rounds(self.h, int(rounds)))

    def last_culling_rounds(self):
        return self.L.aos2_local_map_last_culling_rounds(self.h)

    def last_culling_device_ms(self):
        return float(self.L.aos2_local_map_last_culling_device_ms(self.h))

    @staticmethod
    def keyframe_culling_host(graph, view, cand, monocular=False, bad_cap=None):
        """aos2_debug_keyframe_culling_host: the same loop on one core, no device"""
        keep = [np.zeros(1, np.int32)]
        g, v = _local_map_graph(graph, keep), _kf_culling_view(view, keep)
        bad_cap = int(graph["n_points"]) if bad_cap is None else bad_cap
        return _kf_culling_call(lib().aos2_debug_keyframe_culling_host, (C.byref(g), C.byref(v)), monocular, cand, bad_cap)

    def update_connections(self, kf, mp=None, th=CONNECTIONS_TH, conn_cap=256, ordered_cap=256, mp_cap=None):
        """aos2_local_map_update_connections (KeyFrame::UpdateConnections, src/KeyFrame.cc:350-440) on the device -> the dict of
        _update_connections_call"""
        return _update_connections_call(self.L.aos2_local_map_update_connections, (self.h,), th, kf, mp, conn_cap, ordered_cap, mp_cap)

    @staticmethod
    def update_connections_host(graph, kf, mp=None, th=CONNECTIONS_TH, conn_cap=256, ordered_cap=256, mp_cap=None):
        """aos2_debug_update_connections_host: the same function on one core, no device"""
        keep = [np.zeros(1, np.int32)]
        g = _local_map_graph(graph, keep)
        return _update_connections_call(lib().aos2_debug_update_connections_host, (C.byref(g),), th, kf, mp, conn_cap, ordered_cap, mp_cap)

    def debug_connections_sort(self, lds_entries=0):
        _check(self.L.aos2_local_map_debug_connections_sort(self.h, int(lds_entries)))

    def last_connections_device_ms(self):
        return float(self.L.aos2_local_map_last_connections_device_ms(self.h))

    def update_host(self, n, mp, local_cap, kf_cap, local_kfs=None, n_local_kfs=None, ref_kf=None):
        """aos2_local_map_update: the device kernels on host arrays, arguments and result as host()"""
        return self._on_host_arrays(self.L.aos2_local_map_update, self.h, n, mp, local_cap, kf_cap, local_kfs, n_local_kfs, ref_kf)

    @staticmethod
    def host(graph, n, mp, local_cap, kf_cap, local_kfs=None, n_local_kfs=None, ref_kf=None):
        """aos2_debug_local_map_host: n int32 [B], mp int32 [B][cap]; the previous lists default to empty and ref_kf to -1 ->
        dict(mp, local, n_local, local_kfs, n_local_kfs, ref_kf), new arrays"""
        keep = [np.zeros(1, np.int32)]
        s = _local_map_graph(graph, keep)
        return LocalMap._on_host_arrays(lib().aos2_debug_local_map_host, C.byref(s), n, mp, local_cap, kf_cap, local_kfs, n_local_kfs, ref_kf)

    @staticmethod
    def _on_host_arrays(fn, first, n, mp, local_cap, kf_cap, local_kfs, n_local_kfs, ref_kf):
        mp = np.array(mp, np.int32, ndmin=2)
        B, cap = mp.shape
        n = np.ascontiguousarray(n, np.int32).reshape(B)
        lk = np.full((B, kf_cap), -1, np.int32) if local_kfs is None else np.array(local_kfs, np.int32).reshape(B, kf_cap)
        nlk = np.zeros(B, np.int32) if n_local_kfs is None else np.array(n_local_kfs, np.int32).reshape(B)
        ref = np.full(B, -1, np.int32) if ref_kf is None else np.array(ref_kf, np.int32).reshape(B)
        local, n_local = np.full((B, local_cap), -7, np.int32), np.full(B, -7, np.int32)
        _check(fn(first, B, cap, _p(n), _p(mp), _p(local), int(local_cap), _p(n_local), _p(lk), int(kf_cap), _p(nlk), _p(ref)))
        return dict(mp=mp, local=local, n_local=n_local, local_kfs=lk, n_local_kfs=nlk, ref_kf=ref)

    @staticmethod
    def stats_host(graph, n, mp, outlier, stereo=False, only_tracking=False, found_inc=True):
        """aos2_debug_local_map_stats_host -> dict(stats int32 [B][3], mp, found_inc int32 [n_points] | None)"""
        mp = np.array(mp, np.int32, ndmin=2)
        B, cap = mp.shape
        n = np.ascontiguousarray(n, np.int32).reshape(B)
        outlier = np.ascontiguousarray(outlier, np.uint8).reshape(B, cap)
        stats = np.zeros((B, 3), np.int32)
        inc = np.zeros(max(int(graph["n_points"]), 1), np.int32) if found_inc else None
        keep = [np.zeros(1, np.int32)]
        s = _local_map_graph(graph, keep)
        _check(lib().aos2_debug_local_map_stats_host(C.byref(s), B, cap, _p(n), _p(mp), _p(outlier), int(bool(stereo)),
                                                     int(bool(only_tracking)), _p(stats), _p(inc) if found_inc else None))
        return dict(stats=stats, mp=mp, found_inc=None if inc is None else inc[:int(graph["n_points"])])


def debug_tw_math(x, y, device=-1):
    """aos2_debug_tw_math: tw_sin(x), tw_cos(x), tw_atan2(y, x), sqrt(x), y / x of csrc/motion_tw.h on the host (device -1) or in a
    kernel -> dict of float64 arrays"""
    x, y = np.ascontiguousarray(x, np.float64).reshape(-1), np.ascontiguousarray(y, np.float64).reshape(-1)
    if len(x) != len(y):
        raise ValueError("x and y differ in length")
    out = {k: np.zeros(len(x), np.float64) for k in ("sin", "cos", "atan2", "sqrt", "quot")}
    _check(lib().aos2_debug_tw_math(int(device), len(x), _p(x), _p(y), *[_p(out[k]) for k in ("sin", "cos", "atan2", "sqrt", "quot")]))
    return out


def ComputeStereoMatches(left: Extractor, right: Extractor, kps_l, desc_l, kps_r, desc_r, mb, mbf, image=0):
    """Frame::ComputeStereoMatches (src/Frame.cc:495-669) on the pyramids `left` / `right` hold from their
    last extract.  Returns (mvuRight, mvDepth) float32 arrays, -1 = no match."""
    kps_l = np.ascontiguousarray(kps_l, KP_DTYPE)
    kps_r = np.ascontiguousarray(kps_r, KP_DTYPE)
    desc_l = np.ascontiguousarray(desc_l, np.uint8)
    desc_r = np.ascontiguousarray(desc_r, np.uint8)
    ur = np.full(len(kps_l), -1.0, np.float32)
    dp = np.full(len(kps_l), -1.0, np.float32)
    _check(left.L.aos2_compute_stereo_matches(left.h, right.h, image, _p(kps_l), _p(desc_l), len(kps_l), _p(kps_r),
                                              _p(desc_r), len(kps_r), mb, mbf, _p(ur), _p(dp)))
    return ur, dp


def compute_stereo_matches_device(left: Extractor, right: Extractor, batch, d_kpl, d_dl, d_nl, d_kpr, d_dr, d_nr, cap,
                                  mb, mbf, d_ur, d_depth):
    """raw device pointers (ints); arrays as written by extract_batch_device for the two eyes"""
    V = C.c_void_p
    _check(left.L.aos2_compute_stereo_matches_device(left.h, right.h, batch, V(d_kpl), V(d_dl), V(d_nl), V(d_kpr),
                                                     V(d_dr), V(d_nr), cap, mb, mbf, V(d_ur), V(d_depth)))
    return float(left.L.aos2_compute_stereo_matches_last_device_ms(left.h))


def compute_stereo_matches_device_async(left: Extractor, right: Extractor, batch, d_kpl, d_dl, d_nl, d_kpr, d_dr, d_nr, cap,
                                        mb, mbf, d_ur, d_depth):
    """the same, enqueued behind both extractors' batches in flight (no host wait)"""
    V = C.c_void_p
    _check(left.L.aos2_compute_stereo_matches_device_async(left.h, right.h, batch, V(d_kpl), V(d_dl), V(d_nl), V(d_kpr),
                                                           V(d_dr), V(d_nr), cap, mb, mbf, V(d_ur), V(d_depth)))


def debug_octree_host(xs, ys, score, minX, maxX, minY, maxY, N):
    xs = np.ascontiguousarray(xs, np.int16)
    ys = np.ascontiguousarray(ys, np.int16)
    score = np.ascontiguousarray(score, np.uint8)
    out = np.zeros(max(len(xs), 1), np.int32)
    k = lib().aos2_debug_octree_host(_p(xs), _p(ys), _p(score), len(xs), minX, maxX, minY, maxY, N, _p(out), len(out))
    if k < 0:
        raise AosError(k, "octree scratch exhausted")
    return out[:k].copy()


def debug_sincos_host(angle_rad):
    s, c = C.c_float(), C.c_float()
    lib().aos2_debug_sincos_host(float(angle_rad), C.byref(s), C.byref(c))
    return s.value, c.value


# ---- the loop body of LocalMapping::CreateNewMapPoints (include/aos2.h: aos2_triangulate_matches and friends)
TRI_NO_MATCH, TRI_ACCEPTED, TRI_LOW_PARALLAX, TRI_W_ZERO, TRI_DEPTH1, TRI_DEPTH2, TRI_REPROJ1, TRI_REPROJ2, TRI_ZERO_DIST, TRI_SCALE, \
    TRI_SUPERSEDED = range(11)


class _TriangGeom(C.Structure):
    _fields_ = [("Tcw1", C.c_float * 16), ("Tcw2", C.c_float * 16)] + \
               [(k, C.c_float) for k in ("fx1", "fy1", "cx1", "cy1", "mb1", "mbf1", "fx2", "fy2", "cx2", "cy2", "mb2", "mbf2")] + \
               [("n_levels", C.c_int32), ("scale_factors1", C.c_float * 8), ("scale_factors2", C.c_float * 8)]


# aos2_triang_obs_t: mvKeysUn[i].pt, mvKeys[i].pt, mvuRight[i], mvDepth[i], mvKeysUn[i].octave
TRIANG_OBS = np.dtype([("ux", "<f4"), ("uy", "<f4"), ("kx", "<f4"), ("ky", "<f4"), ("u_right", "<f4"), ("depth", "<f4"), ("octave", "<i4")])


def _triang_args(kf1, kf2, obs1, obs2):
    """kf1 / kf2: dicts with Tcw (4x4), fx fy cx cy mb mbf, scale_factors; obs1 / obs2: TRIANG_OBS arrays of the n matches"""
    g = _TriangGeom()
    sf1, sf2 = (np.asarray(k["scale_factors"], np.float32) for k in (kf1, kf2))
    if len(sf1) != len(sf2) or len(sf1) > 8:
        raise ValueError("both keyframes carry the same (at most 8) pyramid levels")
    g.n_levels = len(sf1)
    for tag, k, sf in (("1", kf1, sf1), ("2", kf2, sf2)):
        setattr(g, "Tcw" + tag, (C.c_float * 16)(*[float(v) for v in np.asarray(k["Tcw"], np.float32).reshape(16)]))
        for name in ("fx", "fy", "cx", "cy", "mb", "mbf"):
            setattr(g, name + tag, float(np.float32(k[name])))
        setattr(g, "scale_factors" + tag, (C.c_float * 8)(*[float(v) for v in sf]))
    obs1, obs2 = np.ascontiguousarray(obs1, TRIANG_OBS), np.ascontiguousarray(obs2, TRIANG_OBS)
    if obs1.shape != obs2.shape or obs1.ndim != 1:
        raise ValueError("one observation of each keyframe per match")
    n = len(obs1)
    return g, n, obs1, obs2, np.zeros((n, 3), np.float32), np.zeros(n, np.uint8)


def debug_triangulate_host(kf1, kf2, obs1, obs2):
    """aos2_debug_triangulate_host: the routine of the device kernels on the CPU -> (status uint8 [n], x3D float32 [n][3])"""
    g, n, obs1, obs2, x3D, status = _triang_args(kf1, kf2, obs1, obs2)
    _check(lib().aos2_debug_triangulate_host(C.byref(g), n, _p(obs1), _p(obs2), _p(x3D), _p(status)))
    return status, x3D


# ---- the RANSAC of Sim3Solver (include/aos2.h: aos2_sim3_ransac, aos2_debug_sim3_host)
class _Sim3Problem(C.Structure):
    _fields_ = [("n", C.c_int32), ("X3Dc1", C.c_void_p), ("X3Dc2", C.c_void_p), ("max_err1", C.c_void_p), ("max_err2", C.c_void_p)] + \
               [(k, C.c_float) for k in ("fx1", "fy1", "cx1", "cy1", "fx2", "fy2", "cx2", "cy2")] + \
               [("fix_scale", C.c_int32), ("probability", C.c_double), ("min_inliers", C.c_int32), ("max_iterations", C.c_int32),
                ("draws", C.c_void_p)]


class _Sim3Result(C.Structure):
    _fields_ = [("ransac_max_its", C.c_int32), ("first_success", C.c_int32), ("best_iteration", C.c_int32), ("best_inliers", C.c_int32),
                ("T12", C.c_float * 16), ("R12", C.c_float * 9), ("t12", C.c_float * 3), ("s12", C.c_float),
                ("inliers", C.c_void_p), ("counts", C.c_void_p)]


def sim3_random_int(rng, lo, hi):
    """DUtils::Random::RandomInt(min, max) (Thirdparty/DBoW2/DUtils/Random.cpp:47-50): d = max - min + 1,
    int(((double)rand() / ((double)RAND_MAX + 1.0)) * d) + min, with rand() taken from `rng` (a numpy Generator)"""
    d = hi - lo + 1
    return int((float(rng.integers(0, 2 ** 31)) / (2147483647.0 + 1.0)) * d) + lo


def sim3_draws(rng, n, max_iterations):
    """the draws of max_iterations iterations of Sim3Solver::iterate (:166-177) over n correspondences, in iteration order:
    int32 [max_iterations][3], draw i of an iteration = RandomInt(0, n - 1 - i); zeros when n < 3 (nothing to draw from)"""
    d = np.zeros((max_iterations, 3), np.int32)
    if n >= 3:
        for k in range(max_iterations):
            for i in range(3):
                d[k, i] = sim3_random_int(rng, 0, n - 1 - i)
    return d


def _sim3_args(problems, sentinel=None):
    """problems: dicts with X3Dc1 / X3Dc2 [n][3], max_err1 / max_err2 [n], K1 / K2 = (fx, fy, cx, cy), fix_scale, probability,
    min_inliers, max_iterations, draws [max_iterations][3]"""
    P, R, keep, outs = (_Sim3Problem * max(1, len(problems)))(), (_Sim3Result * max(1, len(problems)))(), [], []
    for i, q in enumerate(problems):
        arr = [np.ascontiguousarray(q[k], np.float32) for k in ("X3Dc1", "X3Dc2", "max_err1", "max_err2")]
        draws = np.ascontiguousarray(q["draws"], np.int32)
        n, its = len(arr[0]), int(q["max_iterations"])
        if arr[0].shape != (n, 3) or arr[1].shape != (n, 3) or arr[2].shape != (n,) or arr[3].shape != (n,) or draws.shape != (max(its, 0), 3):
            raise ValueError("problem %d: X3Dc [n][3], max_err [n], draws [max_iterations][3]" % i)
        inl = np.full(n, 0 if sentinel is None else sentinel, np.uint8)
        counts = np.full(max(its, 0), -1 if sentinel is None else sentinel, np.int32)
        keep += arr + [draws]
        outs.append((inl, counts))
        P[i].n = n
        P[i].X3Dc1, P[i].X3Dc2, P[i].max_err1, P[i].max_err2, P[i].draws = (a.ctypes.data for a in arr + [draws])
        for tag, K in (("1", q["K1"]), ("2", q["K2"])):
            for name, v in zip(("fx", "fy", "cx", "cy"), K):
                setattr(P[i], name + tag, float(np.float32(v)))
        P[i].fix_scale, P[i].probability = int(bool(q["fix_scale"])), float(q["probability"])
        P[i].min_inliers, P[i].max_iterations = int(q["min_inliers"]), its
        R[i].inliers, R[i].counts = inl.ctypes.data, counts.ctypes.data
        if sentinel is not None:
            R[i].ransac_max_its = R[i].first_success = R[i].best_iteration = R[i].best_inliers = sentinel
    return P, R, keep, outs


def _sim3_results(R, outs):
    return [dict(ransac_max_its=R[i].ransac_max_its, first_success=R[i].first_success, best_iteration=R[i].best_iteration,
                 best_inliers=R[i].best_inliers, T12=np.array(R[i].T12, np.float32).reshape(4, 4), R12=np.array(R[i].R12, np.float32).reshape(3, 3),
                 t12=np.array(R[i].t12, np.float32), s12=np.float32(R[i].s12), inliers=inl, counts=counts)
            for i, (inl, counts) in enumerate(outs)]


def debug_sim3_host(problems):
    """aos2_debug_sim3_host: the routine of the device kernels on the CPU -> one dict per problem (the fields of aos2_sim3_result_t)"""
    P, R, keep, outs = _sim3_args(problems)
    _check(lib().aos2_debug_sim3_host(P, R, len(problems)))
    return _sim3_results(R, outs)


# ---- the RANSAC of PnPsolver (include/aos2.h: aos2_pnp_ransac, aos2_debug_pnp_host, aos2_pnp_ransac_parameters)
class _PnpProblem(C.Structure):
    _fields_ = [("n", C.c_int32), ("P3Dw", C.c_void_p), ("P2D", C.c_void_p), ("max_err", C.c_void_p)] + \
               [(k, C.c_float) for k in ("fx", "fy", "cx", "cy")] + \
               [("min_inliers", C.c_int32), ("min_set", C.c_int32), ("first_iteration", C.c_int32), ("n_iterations", C.c_int32),
                ("draws", C.c_void_p), ("best_inliers_in", C.c_int32), ("best_in", C.c_void_p)]


class _PnpResult(C.Structure):
    _fields_ = [("returned_at", C.c_int32), ("Tcw", C.c_float * 16), ("n_inliers", C.c_int32), ("inliers", C.c_void_p),
                ("best_iteration", C.c_int32), ("best_inliers", C.c_int32), ("best_Tcw", C.c_float * 16), ("best", C.c_void_p),
                ("counts", C.c_void_p)]


def pnp_ransac_parameters(n, probability=0.99, min_inliers=8, max_iterations=300, min_set=4, epsilon=0.4):
    """aos2_pnp_ransac_parameters: SetRansacParameters (src/PnPsolver.cc:121-157; the defaults of include/PnPsolver.h:63) ->
    (mRansacMinInliers, mRansacEpsilon, mRansacMaxIts) as adjusted for n correspondences"""
    mi, eps, its = C.c_int32(), C.c_float(), C.c_int32()
    _check(lib().aos2_pnp_ransac_parameters(int(n), float(probability), int(min_inliers), int(max_iterations), int(min_set), float(np.float32(epsilon)),
                                            C.byref(mi), C.byref(eps), C.byref(its)))
    return mi.value, np.float32(eps.value), its.value


def pnp_draws(rng, n, n_iterations, min_set):
    """the draws of n_iterations iterations of PnPsolver::iterate (:191-201) over n correspondences, in iteration order:
    int32 [n_iterations][min_set], draw i of an iteration = RandomInt(0, n - 1 - i); zeros when n < min_set (nothing to draw from)"""
    d = np.zeros((n_iterations, min_set), np.int32)
    if n >= min_set:
        for k in range(n_iterations):
            for i in range(min_set):
                d[k, i] = sim3_random_int(rng, 0, n - 1 - i)
    return d


def _pnp_args(problems, sentinel=None, with_counts=True):
    """problems: dicts with P3Dw [n][3], P2D [n][2], max_err [n], K = (fx, fy, cx, cy), min_inliers (adjusted), min_set, n_iterations,
    draws [n_iterations][min_set], and optionally the carried state first_iteration, best_inliers_in, best_in [n]"""
    P, R, keep, outs = (_PnpProblem * max(1, len(problems)))(), (_PnpResult * max(1, len(problems)))(), [], []
    for i, q in enumerate(problems):
        arr = [np.ascontiguousarray(q[k], np.float32) for k in ("P3Dw", "P2D", "max_err")]
        n, its, ms = len(arr[0]), int(q["n_iterations"]), int(q["min_set"])
        draws = np.ascontiguousarray(q["draws"], np.int32)
        if arr[0].shape != (n, 3) or arr[1].shape != (n, 2) or arr[2].shape != (n,) or draws.shape != (max(its, 0), ms):
            raise ValueError("problem %d: P3Dw [n][3], P2D [n][2], max_err [n], draws [n_iterations][min_set]" % i)
        fill = 0 if sentinel is None else sentinel
        inl, best = np.full(n, fill, np.uint8), np.full(n, fill, np.uint8)
        counts = np.full(max(its, 0), -1 if sentinel is None else sentinel, np.int32) if with_counts else None
        keep += arr + [draws]
        outs.append((inl, best, counts))
        P[i].n = n
        P[i].P3Dw, P[i].P2D, P[i].max_err, P[i].draws = (a.ctypes.data for a in arr + [draws])
        for name, v in zip(("fx", "fy", "cx", "cy"), q["K"]):
            setattr(P[i], name, float(np.float32(v)))
        P[i].min_inliers, P[i].min_set, P[i].n_iterations = int(q["min_inliers"]), ms, its
        P[i].first_iteration, P[i].best_inliers_in = int(q.get("first_iteration", 0)), int(q.get("best_inliers_in", 0))
        if q.get("best_in") is not None:
            bi = np.ascontiguousarray(q["best_in"], np.uint8)
            if bi.shape != (n,):
                raise ValueError("problem %d: best_in [n]" % i)
            keep.append(bi)
            P[i].best_in = bi.ctypes.data
        R[i].inliers, R[i].best = inl.ctypes.data, best.ctypes.data
        R[i].counts = counts.ctypes.data if with_counts else None
        if sentinel is not None:
            C.memset(C.byref(R[i]), sentinel, _PnpResult.inliers.offset)
            C.memset(C.byref(R[i], _PnpResult.best_iteration.offset), sentinel, _PnpResult.best.offset - _PnpResult.best_iteration.offset)
    return P, R, keep, outs


def _pnp_results(R, outs):
    return [dict(returned_at=R[i].returned_at, Tcw=np.array(R[i].Tcw, np.float32).reshape(4, 4), n_inliers=R[i].n_inliers, inliers=inl,
                 best_iteration=R[i].best_iteration, best_inliers=R[i].best_inliers, best_Tcw=np.array(R[i].best_Tcw, np.float32).reshape(4, 4),
                 best=best, counts=counts)
            for i, (inl, best, counts) in enumerate(outs)]


def debug_pnp_set(n, row):
    """aos2_debug_pnp_set: the indices the draws of one iteration select, as csrc/pnp.h forms them"""
    row = np.ascontiguousarray(row, np.int32)
    out = np.zeros(len(row), np.int32)
    _check(lib().aos2_debug_pnp_set(int(n), _p(row), len(row), _p(out)))
    return [int(i) for i in out]


def debug_pnp_scan(first_iteration, counts, refined, refined_carried, min_inliers, best_inliers_in=0):
    """aos2_debug_pnp_scan: the loop of iterate() over tables -> (returned_at, best_iteration, best_inliers)"""
    counts, refined = np.ascontiguousarray(counts, np.int32), np.ascontiguousarray(refined, np.int32)
    r = [C.c_int32() for _ in range(3)]
    _check(lib().aos2_debug_pnp_scan(int(first_iteration), len(counts), _p(counts), _p(refined), int(refined_carried), int(min_inliers),
                                     int(best_inliers_in), *[C.byref(x) for x in r]))
    return tuple(x.value for x in r)


def debug_pnp_host(problems, with_counts=True):
    """aos2_debug_pnp_host: the routine of the device kernels on the CPU -> one dict per problem (the fields of aos2_pnp_result_t)"""
    P, R, keep, outs = _pnp_args(problems, None, with_counts)
    _check(lib().aos2_debug_pnp_host(P, R, len(problems)))
    return _pnp_results(R, outs)


# ---- Initializer::Initialize (include/aos2.h: aos2_initializer_initialize, aos2_debug_initializer_host)
AOS2_INIT_OK, AOS2_INIT_NO_MODEL = 0, 1


class _InitProblem(C.Structure):
    _fields_ = [("n_keys1", C.c_int32), ("n_keys2", C.c_int32), ("keys1", C.c_void_p), ("keys2", C.c_void_p), ("n_matches", C.c_int32),
                ("matches", C.c_void_p), ("sigma", C.c_float), ("iterations", C.c_int32), ("sets", C.c_void_p)] + \
               [(k, C.c_float) for k in ("fx", "fy", "cx", "cy", "min_parallax")] + [("min_triangulated", C.c_int32)]


class _InitResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("initialized", C.c_int32), ("used_homography", C.c_int32), ("SH", C.c_float), ("SF", C.c_float),
                ("H21", C.c_float * 9), ("F21", C.c_float * 9), ("best_iteration_h", C.c_int32), ("best_iteration_f", C.c_int32),
                ("inliers_h", C.c_void_p), ("inliers_f", C.c_void_p), ("R21", C.c_float * 9), ("t21", C.c_float * 3), ("P3D", C.c_void_p),
                ("triangulated", C.c_void_p), ("n_good", C.c_int32 * 8), ("parallax", C.c_float * 8), ("n_hypotheses", C.c_int32)]


_INIT_SCALARS = ("status", "initialized", "used_homography", "SH", "SF", "best_iteration_h", "best_iteration_f", "n_hypotheses")
_INIT_ARRAYS = (("H21", np.float32), ("F21", np.float32), ("R21", np.float32), ("t21", np.float32), ("n_good", np.int32),
                ("parallax", np.float32))


def initializer_sets(rng, n_matches, iterations):
    """mvSets (src/Initializer.cc:78-97): per iteration 8 indices drawn without replacement by RandomInt(0, size - 1) and the
    swap-with-back removal; int32 [iterations][8]"""
    sets = np.zeros((iterations, 8), np.int32)
    for it in range(iterations):
        avail = list(range(n_matches))
        for j in range(8):
            r = sim3_random_int(rng, 0, len(avail) - 1)
            sets[it, j] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return sets


def _init_args(problems, sentinel=None):
    """problems: dicts with keys1 [n1][2], keys2 [n2][2], matches [n][2], sets [iterations][8], K = (fx, fy, cx, cy) and optionally
    sigma (1.0), min_parallax (1.0), min_triangulated (50)"""
    P, R, keep, outs = (_InitProblem * max(1, len(problems)))(), (_InitResult * max(1, len(problems)))(), [], []
    for i, q in enumerate(problems):
        k1, k2 = np.ascontiguousarray(q["keys1"], np.float32), np.ascontiguousarray(q["keys2"], np.float32)
        mt, sets = np.ascontiguousarray(q["matches"], np.int32), np.ascontiguousarray(q["sets"], np.int32)
        if k1.ndim != 2 or k1.shape[1] != 2 or k2.ndim != 2 or k2.shape[1] != 2 or mt.ndim != 2 or mt.shape[1] != 2 or sets.ndim != 2 or sets.shape[1] != 8:
            raise ValueError("problem %d: keys1 [n1][2], keys2 [n2][2], matches [n][2], sets [iterations][8]" % i)
        fill = 0 if sentinel is None else sentinel
        out = (np.full(len(mt), fill, np.uint8), np.full(len(mt), fill, np.uint8), np.full((len(k1), 3), 0, np.float32), np.full(len(k1), fill, np.uint8))
        if sentinel is not None:
            out[2].view(np.uint8)[...] = sentinel
        keep += [k1, k2, mt, sets]
        outs.append(out)
        P[i].n_keys1, P[i].n_keys2, P[i].n_matches = len(k1), len(k2), int(q.get("n_matches", len(mt)))
        P[i].iterations = int(q.get("iterations", len(sets)))
        P[i].keys1, P[i].keys2, P[i].matches, P[i].sets = (a.ctypes.data if a.size else None for a in (k1, k2, mt, sets))
        P[i].sigma, P[i].min_parallax = float(np.float32(q.get("sigma", 1.0))), float(np.float32(q.get("min_parallax", 1.0)))
        P[i].min_triangulated = int(q.get("min_triangulated", 50))
        for name, v in zip(("fx", "fy", "cx", "cy"), q["K"]):
            setattr(P[i], name, float(np.float32(v)))
        if sentinel is not None:
            C.memset(C.byref(R[i]), sentinel, C.sizeof(_InitResult))
        R[i].inliers_h, R[i].inliers_f, R[i].P3D, R[i].triangulated = (a.ctypes.data for a in out)
        for name in q.get("null", ()):   # (tests: a missing array)
            setattr(R[i] if name in ("inliers_h", "inliers_f", "P3D", "triangulated") else P[i], name, None)
    return P, R, keep, outs


def _init_results(R, outs):
    res = []
    for i, (ih, jf, p3d, tri) in enumerate(outs):
        d = {k: getattr(R[i], k) for k in _INIT_SCALARS}
        d.update({k: np.array(getattr(R[i], k), t).reshape((3, 3) if k in ("H21", "F21", "R21") else -1) for k, t in _INIT_ARRAYS})
        d["SH"], d["SF"] = np.float32(d["SH"]), np.float32(d["SF"])
        d.update(inliers_h=ih, inliers_f=jf, P3D=p3d, triangulated=tri)
        res.append(d)
    return res


init_last = None   # (result structs, result arrays, the structs' bytes before the call) of the last initializer call


def debug_initializer_host(problems, sentinel=None):
    """aos2_debug_initializer_host: the routines of the device kernels on the CPU -> one dict per problem (aos2_initializer_result_t).
    `sentinel` pre-fills the result buffers; they stay in capi.init_last for a caller that expects an error"""
    global init_last
    P, R, keep, outs = _init_args(problems, sentinel)
    init_last = (R, outs, [bytes(R[i]) for i in range(len(problems))])
    _check(lib().aos2_debug_initializer_host(P, R, len(problems)))
    return _init_results(R, outs)


def debug_initializer_svd(A):
    """aos2_debug_initializer_svd: cv::SVDecomp of a float matrix as csrc/initializer.h runs it -> (left [n1][m], w [n], right [n][n])"""
    A = np.ascontiguousarray(A, np.float32)
    rows, cols = A.shape
    wide = rows < cols
    n, m = (rows, cols) if wide else (cols, rows)
    left, w, right = np.zeros((cols if wide else n, m), np.float32), np.zeros(n, np.float32), np.zeros((n, n), np.float32)
    _check(lib().aos2_debug_initializer_svd(_p(A), rows, cols, _p(left), _p(w), _p(right)))
    return left, w, right


def debug_initializer_rng(n):
    """the first n values of cv::RNG(0x12345678).next() as csrc/initializer.h generates them"""
    out = np.zeros(n, np.uint32)
    _check(lib().aos2_debug_initializer_rng(int(n), _p(out)))
    return out


def debug_initializer_inv33(S):
    """cv::Mat::inv() and cv::determinant of a float 3x3 -> (inverse, determinant)"""
    S, inv, det = np.ascontiguousarray(S, np.float32), np.zeros((3, 3), np.float32), C.c_double()
    _check(lib().aos2_debug_initializer_inv33(_p(S), _p(inv), C.byref(det)))
    return inv, det.value


# ---- Optimizer::OptimizeSim3 (include/aos2.h: aos2_optimize_sim3, aos2_debug_sim3_opt_host)
class _Sim3OptProblem(C.Structure):
    _fields_ = [("n", C.c_int32)] + [(k, C.c_void_p) for k in ("X1c", "X2c", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2")] + \
               [(k, C.c_float) for k in ("fx1", "fy1", "cx1", "cy1", "fx2", "fy2", "cx2", "cy2")] + \
               [("q12", C.c_double * 4), ("t12", C.c_double * 3), ("s12", C.c_double), ("th2", C.c_float), ("fix_scale", C.c_int32)]


class _Sim3OptResult(C.Structure):
    _fields_ = [("q12", C.c_double * 4), ("t12", C.c_double * 3), ("s12", C.c_double), ("outlier", C.c_void_p),
                ("n_bad", C.c_int32), ("n_inliers", C.c_int32), ("iterations", C.c_int32 * 2), ("trials", C.c_int32 * 2)]


def _sim3_opt_args(problems, sentinel=None):
    """problems: dicts with X1c / X2c [n][3], obs1 / obs2 [n][2], inv_sigma2_1 / inv_sigma2_2 [n], K1 / K2 = (fx, fy, cx, cy),
    q12 (x, y, z, w), t12, s12 (float64), th2, fix_scale"""
    P, R, keep, outs = (_Sim3OptProblem * max(1, len(problems)))(), (_Sim3OptResult * max(1, len(problems)))(), [], []
    names = ("X1c", "X2c", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2")
    for i, q in enumerate(problems):
        arr = [np.ascontiguousarray(q[k], np.float32) for k in names]
        n = len(arr[0])
        if [a.shape for a in arr] != [(n, 3), (n, 3), (n, 2), (n, 2), (n,), (n,)]:
            raise ValueError("problem %d: X [n][3], obs [n][2], inv_sigma2 [n]" % i)
        out = np.full(n, 0 if sentinel is None else sentinel, np.uint8)
        keep += arr
        outs.append(out)
        P[i].n = n
        for k, a in zip(names, arr):
            setattr(P[i], k, a.ctypes.data)
        for tag, K in (("1", q["K1"]), ("2", q["K2"])):
            for name, v in zip(("fx", "fy", "cx", "cy"), K):
                setattr(P[i], name + tag, float(np.float32(v)))
        P[i].q12 = (C.c_double * 4)(*[float(v) for v in q["q12"]])
        P[i].t12 = (C.c_double * 3)(*[float(v) for v in q["t12"]])
        P[i].s12, P[i].th2, P[i].fix_scale = float(q["s12"]), float(np.float32(q["th2"])), int(bool(q["fix_scale"]))
        R[i].outlier = out.ctypes.data
        if sentinel is not None:
            C.memset(C.byref(R[i]), sentinel, _Sim3OptResult.outlier.offset)
            R[i].n_bad = R[i].n_inliers = sentinel
    return P, R, keep, outs


def _sim3_opt_results(R, outs):
    return [dict(q12=np.array(R[i].q12, np.float64), t12=np.array(R[i].t12, np.float64), s12=np.float64(R[i].s12), outlier=out,
                 n_bad=R[i].n_bad, n_inliers=R[i].n_inliers, iterations=tuple(R[i].iterations), trials=tuple(R[i].trials))
            for i, out in enumerate(outs)]


def debug_sim3_opt_host(problems):
    """aos2_debug_sim3_opt_host: the routine of the device kernel on the CPU -> one dict per problem (the fields of aos2_sim3_opt_result_t)"""
    P, R, keep, outs = _sim3_opt_args(problems)
    _check(lib().aos2_debug_sim3_opt_host(P, R, len(problems)))
    return _sim3_opt_results(R, outs)


SIM3_OPT_LINEARISE, SIM3_OPT_TRIAL, SIM3_OPT_REJECT = 1, 2, 4
SIM3_OPT_STEPS_TAIL = 16   # elements the wrappers put behind act / chi / outlier


class _Sim3OptSteps(C.Structure):
    _fields_ = [("problem", _Sim3OptProblem), ("S_lin", C.c_double * 8), ("S_trial", C.c_double * 8)] + \
               [(k, C.c_void_p) for k in ("act_in", "chi_in", "outlier_in")] + [(k, C.c_int32) for k in ("tail", "remove", "mask", "pad")] + \
               [(k, C.c_void_p) for k in ("Hb", "pert", "chi_lin", "trial_sum", "chi_trial", "flagged", "chi", "act", "outlier")]


def _sim3_opt_steps_args(items, sentinel=0x5A, tail_byte=0xA5):
    """items: dicts with problem (as _sim3_opt_args takes it), S_lin / S_trial = (q, t, s), act_in [2n], chi_in [2n], outlier_in [n],
    remove, mask.  Every output buffer is filled with the byte `sentinel`; the SIM3_OPT_STEPS_TAIL elements behind the three planted
    arrays hold the byte `tail_byte` -> (the C items, what has to stay alive, the output arrays per item)"""
    I, keep, outs, tail = (_Sim3OptSteps * max(1, len(items)))(), [], [], SIM3_OPT_STEPS_TAIL
    for i, it in enumerate(items):
        P, _, arrays, _ = _sim3_opt_args([it["problem"]])
        n = P[0].n
        I[i].problem = P[0]
        for name in ("S_lin", "S_trial"):
            q, t, s = it[name]
            setattr(I[i], name, (C.c_double * 8)(*([float(v) for v in q] + [float(v) for v in t] + [float(s)])))
        planted = {}
        for name, count, dtype in (("act_in", 2 * n, np.uint8), ("chi_in", 2 * n, np.float64), ("outlier_in", n, np.uint8)):
            a = np.ascontiguousarray(it[name], dtype)
            if a.shape != (count,):
                raise ValueError("item %d: %s [%d]" % (i, name, count))
            full = np.empty(count + tail, dtype)
            full.view(np.uint8)[:] = tail_byte
            full[:count] = a
            planted[name] = full
            setattr(I[i], name, full.ctypes.data)
        I[i].tail, I[i].remove, I[i].mask = tail, int(bool(it["remove"])), int(it["mask"])
        out = {}
        for name, count, dtype in (("Hb", 36, np.float64), ("pert", 28 * 8, np.float64), ("chi_lin", 2 * n, np.float64), ("trial_sum", 1, np.float64),
                                   ("chi_trial", 2 * n, np.float64), ("flagged", 1, np.int32), ("chi", 2 * n + tail, np.float64),
                                   ("act", 2 * n + tail, np.uint8), ("outlier", n + tail, np.uint8)):
            a = np.empty(count, dtype)
            a.view(np.uint8)[:] = sentinel
            out[name] = a
            setattr(I[i], name, a.ctypes.data)
        out["pert"] = out["pert"].reshape(28, 8)
        keep += [arrays, planted]
        outs.append(out)
    return I, keep, outs


def debug_sim3_opt_steps_host(items, sentinel=0x5A):
    """aos2_debug_sim3_opt_steps_host: linearise / trial / reject of the host tap's edges alone -> the output arrays per item"""
    I, keep, outs = _sim3_opt_steps_args(items, sentinel)
    _check(lib().aos2_debug_sim3_opt_steps_host(I, len(items)))
    return outs


# ---- Optimizer::OptimizeEssentialGraph (include/aos2.h: aos2_optimize_essential_graph, aos2_debug_essential_graph_host)
AOS2_EG_OK, AOS2_EG_NO_STEP, AOS2_ERR_EG_MEMORY = 0, 1, -6


class _EssentialGraphProblem(C.Structure):
    _fields_ = [("n_vertices", C.c_int32), ("Scw", C.c_void_p), ("fixed", C.c_int32), ("n_edges", C.c_int32), ("v0", C.c_void_p),
                ("v1", C.c_void_p), ("Sji", C.c_void_p), ("fix_scale", C.c_int32), ("iterations", C.c_int32), ("n_points", C.c_int32),
                ("Xw", C.c_void_p), ("ref", C.c_void_p)]


class _EssentialGraphResult(C.Structure):
    _fields_ = [("Scw", C.c_void_p), ("Tiw", C.c_void_p), ("Xw", C.c_void_p), ("chi2_initial", C.c_double), ("chi2_final", C.c_double),
                ("iterations", C.c_int32), ("trials", C.c_int32), ("rejected", C.c_int32), ("l_blocks", C.c_int32), ("status", C.c_int32)]


def _essential_graph_args(problems, sentinel=None):
    """problems: dicts with Scw [n_vertices][8] (q (x, y, z, w), t, s; float64), fixed, v0 / v1 [n_edges], Sji [n_edges][8], fix_scale,
    iterations (20 when absent), Xw [n_points][3] (float32), ref [n_points].  A count may be forced apart from its arrays with
    n_vertices / n_edges / n_points, an array left out with None (what the argument checks are tried with).  `sentinel` pre-fills
    every result byte."""
    n = max(1, len(problems))
    P, R, keep, outs = (_EssentialGraphProblem * n)(), (_EssentialGraphResult * n)(), [], []
    for i, q in enumerate(problems):
        def arr(k, dt, cols):
            if q.get(k) is None:
                return None
            a = np.ascontiguousarray(q[k], dt).reshape((-1, cols) if cols else (-1,))
            keep.append(a)
            return a
        Scw, Sji, v0, v1 = arr("Scw", np.float64, 8), arr("Sji", np.float64, 8), arr("v0", np.int32, 0), arr("v1", np.int32, 0)
        Xw, ref = arr("Xw", np.float32, 3), arr("ref", np.int32, 0)
        if v0 is not None and v1 is not None and Sji is not None and not len(v0) == len(v1) == len(Sji):
            raise ValueError("problem %d: v0, v1 [n_edges], Sji [n_edges][8]" % i)
        if Xw is not None and ref is not None and len(Xw) != len(ref):
            raise ValueError("problem %d: Xw [n_points][3], ref [n_points]" % i)
        P[i].n_vertices = int(q.get("n_vertices", 0 if Scw is None else len(Scw)))
        P[i].n_edges = int(q.get("n_edges", 0 if v0 is None else len(v0)))
        P[i].n_points = int(q.get("n_points", 0 if Xw is None else len(Xw)))
        P[i].fixed, P[i].fix_scale, P[i].iterations = int(q["fixed"]), int(bool(q["fix_scale"])), int(q.get("iterations", 20))
        for k, a in (("Scw", Scw), ("Sji", Sji), ("v0", v0), ("v1", v1), ("Xw", Xw), ("ref", ref)):
            setattr(P[i], k, a.ctypes.data if a is not None and a.size else None)
        nv, npt = max(P[i].n_vertices, 0), max(P[i].n_points, 0)
        fill = 0 if sentinel is None else sentinel
        out = dict(Scw=np.frombuffer(bytes([fill]) * (64 * nv), np.float64).reshape(nv, 8).copy(),
                   Tiw=np.frombuffer(bytes([fill]) * (64 * nv), np.float32).reshape(nv, 4, 4).copy(),
                   Xw=np.frombuffer(bytes([fill]) * (12 * npt), np.float32).reshape(npt, 3).copy())
        outs.append(out)
        R[i].Scw, R[i].Tiw, R[i].Xw = out["Scw"].ctypes.data, out["Tiw"].ctypes.data, out["Xw"].ctypes.data
        if q.get("null_result"):
            setattr(R[i], q["null_result"], None)
        if sentinel is not None:
            off = _EssentialGraphResult.chi2_initial.offset
            C.memset(C.byref(R[i], off), sentinel, C.sizeof(_EssentialGraphResult) - off)
    return P, R, keep, outs


def _essential_graph_results(R, outs):
    return [dict(Scw=o["Scw"], Tiw=o["Tiw"], Xw=o["Xw"], chi2_initial=R[i].chi2_initial, chi2_final=R[i].chi2_final, iterations=R[i].iterations,
                 trials=R[i].trials, rejected=R[i].rejected, l_blocks=R[i].l_blocks, status=R[i].status) for i, o in enumerate(outs)]


def debug_essential_graph_host(problems, sentinel=None):
    """aos2_debug_essential_graph_host: the arithmetic of the device path on the CPU with a skyline solve -> one dict per problem (the
    fields of aos2_essential_graph_result_t)"""
    P, R, keep, outs = _essential_graph_args(problems, sentinel)
    debug_essential_graph_host.last = (R, outs)
    _check(lib().aos2_debug_essential_graph_host(P, R, len(problems)))
    return _essential_graph_results(R, outs)


def debug_essential_graph_arith_host(what, values):
    """aos2_debug_essential_graph_arith_host: "log" of Sim3s [n][8] -> [n][7]; "residual" of (C, S_v0, S_v1) [n][3][8] -> [n][7];
    "lu3" of (W, t) [n][12] -> [n][3]"""
    code, width, out_w = {"log": (0, 8, 7), "residual": (1, 24, 7), "lu3": (2, 12, 3)}[what]
    a = np.ascontiguousarray(values, np.float64).reshape(-1, width)
    out = np.zeros((len(a), out_w))
    _check(lib().aos2_debug_essential_graph_arith_host(code, _p(a), len(a), _p(out)))
    return out


def debug_sincos_device(angles, device=0):
    a = np.ascontiguousarray(angles, np.float32)
    s = np.zeros_like(a)
    c = np.zeros_like(a)
    _check(lib().aos2_debug_sincos_device(_p(a), len(a), _p(s), _p(c), device))
    return s, c


WAVE_OPS_I = ("dpp_u32_B1", "dpp_u32_4E", "dpp_u32_141", "dpp_u32_140", "dpp_i32_B1", "dpp_i32_4E", "dpp_i32_141", "dpp_i32_140",
              "row_sum", "sum", "max", "row_min", "min", "incl_scan", "block_excl_scan", "block_total", "block_sum")
WAVE_OPS_D = ("dpp_f64_B1", "dpp_f64_4E", "dpp_f64_141", "dpp_f64_140", "row_sum_f64", "readlane_0", "readlane_63")


def debug_wave_ops_device(vi, vd, device=0):
    """test tap: every primitive of csrc/wave_ops.h; vi (int32), vd (float64) [cases][nt], nt = 128 or 256 threads per workgroup
    -> dict name -> [cases][nt] (WAVE_OPS_I as int32, the row / wave min as uint32; WAVE_OPS_D as float64)"""
    vi = np.ascontiguousarray(vi, np.int32); vd = np.ascontiguousarray(vd, np.float64)
    assert vi.ndim == 2 and vi.shape == vd.shape
    oi = np.zeros(vi.shape + (len(WAVE_OPS_I),), np.int32)
    od = np.zeros(vi.shape + (len(WAVE_OPS_D),), np.float64)
    _check(lib().aos2_debug_wave_ops_device(_p(vi), _p(vd), vi.shape[0], vi.shape[1], _p(oi), _p(od), device))
    out = {k: oi[..., j].copy() for j, k in enumerate(WAVE_OPS_I)}
    out.update({k: od[..., j].copy() for j, k in enumerate(WAVE_OPS_D)})
    for k in ("row_min", "min"):
        out[k] = out[k].view(np.uint32)
    return out


def debug_row_sums_scatter_device(v, device=0):
    """test tap: row_sums_scatter_f64<K> of csrc/wave_ops.h by one wave; v (float64) [64][K], K = 7, 36 or 42
    -> (every lane's slots [64][ceil(K / 16)], owner [K][2] = (lane of a row, slot) of the total of value i)"""
    v = np.ascontiguousarray(v, np.float64)
    assert v.ndim == 2 and v.shape[0] == 64
    K = v.shape[1]
    out = np.zeros((64, (K + 15) // 16), np.float64)
    owner = np.zeros((K, 2), np.int32)
    _check(lib().aos2_debug_row_sums_scatter_device(_p(v), K, _p(out), _p(owner), device))
    return out, owner


def debug_pose_blocks_device(upd, T, Hb, lam, x0, device=0):
    """test tap: the pose solver's exp-map update and 6x6 solve on the device, n independent cases"""
    upd = np.ascontiguousarray(upd, np.float64); T = np.ascontiguousarray(T, np.float64)
    Hb = np.ascontiguousarray(Hb, np.float64); lam = np.ascontiguousarray(lam, np.float64)
    x = np.ascontiguousarray(x0, np.float64).copy()
    n = len(lam)
    To = np.zeros((n, 7)); ok = np.zeros(n, np.uint8)
    _check(lib().aos2_debug_pose_blocks_device(_p(upd), _p(T), _p(To), _p(Hb), _p(lam), _p(x), _p(ok), n, device))
    return To, x, ok


class _PosePassCase(C.Structure):
    _fields_ = [("n", C.c_int32), ("form", C.c_int32), ("it", C.c_int32), ("Xw", C.c_void_p), ("obs", C.c_void_p), ("inv_sigma2", C.c_void_p),
                ("stereo", C.c_void_p), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("bf", C.c_float),
                ("pose", C.c_double * 7), ("level1", C.c_void_p), ("robust", C.c_void_p), ("outlier", C.c_void_p), ("chi2", C.c_void_p),
                ("sums", C.c_double * 28), ("pose_out", C.c_double * 7), ("Tcw", C.c_float * 16), ("n_bad", C.c_int32), ("n_inliers", C.c_int32)]


POSE_PASS_FORMS = ((4, 256, 1024), (8, 256, 2048), (9, 128, 1152), (0, 256, None))   # form -> (kEpt, NT, largest n)


def debug_pose_pass_device(cases, mode, device=0):
    """test tap: pose_optimization_body of csrc/pose_opt.h, one workgroup per case in the instantiation POSE_PASS_FORMS[case["form"]].
    cases: synth_pose_problem()-style dicts (n, Xw, obs, stereo, inv_sigma2, fx .. bf) with form, pose (7 doubles qx qy qz qw tx ty tz) and,
    optional, it (0), level1 (zeros), robust (ones), outlier (zeros), chi2 (zeros), [n] each.  mode 1: one edge pass -> sums (28: H upper
    triangle, b, robust chi2), chi2 [n]; mode 2: the reclassification of round it -> outlier, level1, robust, chi2, n_bad; mode 0: the
    whole procedure -> outlier, n_bad, n_inliers, pose_out, Tcw.  -> one dict per case with all of them"""
    n_cases = len(cases)
    S = (_PosePassCase * max(n_cases, 1))()
    keep = []
    for s, c in zip(S, cases):
        n = int(c["n"])
        s.n, s.form, s.it = n, int(c["form"]), int(c.get("it", 0))
        arrs = {}
        for name, dt, fill in (("Xw", np.float32, None), ("obs", np.float32, None), ("inv_sigma2", np.float32, None), ("stereo", np.uint8, None),
                               ("level1", np.uint8, 0), ("robust", np.uint8, 1), ("outlier", np.uint8, 0), ("chi2", np.float64, 0)):
            a = np.full(n, fill, dt) if c.get(name) is None else np.array(c[name], dt, order="C").reshape(-1)
            assert a.size == n * (3 if name in ("Xw", "obs") else 1), name
            a = np.concatenate([a, np.zeros(1, dt)])   # (never an empty array)
            arrs[name] = a
            setattr(s, name, a.ctypes.data)
        keep.append(arrs)
        s.fx, s.fy, s.cx, s.cy, s.bf = (float(np.float32(c[k])) for k in ("fx", "fy", "cx", "cy", "bf"))
        s.pose = (C.c_double * 7)(*[float(x) for x in np.asarray(c["pose"], np.float64).reshape(7)])
    _check(lib().aos2_debug_pose_pass_device(C.byref(S) if n_cases else None, n_cases, int(mode), device))
    return [dict(sums=np.array(list(s.sums), np.float64), pose_out=np.array(list(s.pose_out), np.float64), Tcw=np.array(list(s.Tcw), np.float32),
                 n_bad=int(s.n_bad), n_inliers=int(s.n_inliers), **{k: a[k][:s.n].copy() for k in ("level1", "robust", "outlier", "chi2")})
            for s, a in zip(S, keep)]


def debug_lba_reduced_solve_device(cases, device=0):
    """test tap: LocalBA's reduced-system kernels alone, all cases in one launch of each.  cases: dicts with form (0 = k_ldlt_dev,
    2 = k_ldlt_reg), H (n x n, n = 6 np), bs, b_pose, x0, scale0 (n each: what x / scale_terms hold on entry), lam, T (np x 7)
    -> one dict per case: ok, x, scale_terms (n), T_out, T_backup (np x 7)"""
    cat = lambda k, dt=np.float64: np.ascontiguousarray(np.concatenate([np.asarray(c[k], dt).ravel() for c in cases]))
    nps = np.array([np.asarray(c["bs"]).size // 6 for c in cases], np.int32)
    for c, q in zip(cases, nps):
        assert np.asarray(c["H"]).shape == (6 * q, 6 * q) and np.asarray(c["T"]).shape == (q, 7)
        assert all(np.asarray(c[k]).shape == (6 * q,) for k in ("bs", "b_pose", "x0", "scale0"))
    form = np.array([c["form"] for c in cases], np.int32)
    H, bs, bp, T, x, sc = cat("H"), cat("bs"), cat("b_pose"), cat("T"), cat("x0"), cat("scale0")
    lam = np.array([c["lam"] for c in cases], np.float64)
    To, Tb, ok = np.zeros_like(T), np.zeros_like(T), np.zeros(len(cases), np.uint8)
    _check(lib().aos2_debug_lba_reduced_solve_device(len(cases), _p(nps), _p(form), _p(H), _p(bs), _p(bp), _p(lam), _p(T), _p(x), _p(To), _p(Tb),
                                                     _p(sc), _p(ok), device))
    out, o6, o7 = [], 0, 0
    for q, k in zip(nps, ok):
        out.append(dict(ok=int(k), x=x[o6:o6 + 6 * q].copy(), scale_terms=sc[o6:o6 + 6 * q].copy(),
                        T_out=To[o7:o7 + 7 * q].reshape(q, 7).copy(), T_backup=Tb[o7:o7 + 7 * q].reshape(q, 7).copy()))
        o6 += 6 * q; o7 += 7 * q
    return out


# ------------------------------------------------------------------------------------------ matcher
class _BowPair(C.Structure):
    _fields_ = [("n_kf", C.c_int32), ("n_f", C.c_int32), ("desc_kf", C.c_void_p), ("desc_f", C.c_void_p),
                ("kf_has_mp", C.c_void_p), ("angle_kf", C.c_void_p), ("angle_f", C.c_void_p),
                ("n_nodes_kf", C.c_int32), ("n_nodes_f", C.c_int32),
                ("node_id_kf", C.c_void_p), ("node_off_kf", C.c_void_p), ("node_idx_kf", C.c_void_p),
                ("node_id_f", C.c_void_p), ("node_off_f", C.c_void_p), ("node_idx_f", C.c_void_p)]


class _BowFrames(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("cap", C.c_int32)] + [(k, C.c_void_p) for k in (
        "d_desc_kf", "d_kps_kf", "d_n_kf", "d_desc_f", "d_kps_f", "d_n_f", "kf_has_mp", "d_kf_fv_node", "d_kf_fv_off", "d_kf_fv_idx",
        "d_kf_n_fv", "d_f_fv_node", "d_f_fv_off", "d_f_fv_idx", "d_f_n_fv")]


class _BowKfPair(C.Structure):
    _fields_ = [("n1", C.c_int32), ("n2", C.c_int32), ("desc1", C.c_void_p), ("desc2", C.c_void_p),
                ("has_mp1", C.c_void_p), ("has_mp2", C.c_void_p), ("angle1", C.c_void_p), ("angle2", C.c_void_p),
                ("n_nodes1", C.c_int32), ("n_nodes2", C.c_int32),
                ("node_id1", C.c_void_p), ("node_off1", C.c_void_p), ("node_idx1", C.c_void_p),
                ("node_id2", C.c_void_p), ("node_off2", C.c_void_p), ("node_idx2", C.c_void_p)]


class _TriangPair(C.Structure):
    _fields_ = [("n1", C.c_int32), ("n2", C.c_int32), ("desc1", C.c_void_p), ("desc2", C.c_void_p),
                ("has_mp1", C.c_void_p), ("has_mp2", C.c_void_p),
                ("x1", C.c_void_p), ("y1", C.c_void_p), ("angle1", C.c_void_p), ("u_right1", C.c_void_p),
                ("x2", C.c_void_p), ("y2", C.c_void_p), ("angle2", C.c_void_p), ("u_right2", C.c_void_p),
                ("octave2", C.c_void_p), ("scale_factors2", C.c_void_p), ("level_sigma2_2", C.c_void_p),
                ("n_levels2", C.c_int32), ("F12", C.c_float * 9), ("ex", C.c_float), ("ey", C.c_float),
                ("n_nodes1", C.c_int32), ("n_nodes2", C.c_int32),
                ("node_id1", C.c_void_p), ("node_off1", C.c_void_p), ("node_idx1", C.c_void_p),
                ("node_id2", C.c_void_p), ("node_off2", C.c_void_p), ("node_idx2", C.c_void_p)]


class _FrameView(C.Structure):
    _fields_ = [("n_f", C.c_int32), ("desc_f", C.c_void_p), ("kp_x", C.c_void_p), ("kp_y", C.c_void_p),
                ("kp_octave", C.c_void_p), ("kp_angle", C.c_void_p), ("u_right", C.c_void_p),
                ("scale_factors", C.c_void_p), ("n_levels", C.c_int32),
                ("min_x", C.c_float), ("min_y", C.c_float), ("max_x", C.c_float), ("max_y", C.c_float),
                ("grid_w_inv", C.c_float), ("grid_h_inv", C.c_float),
                ("grid_off", C.c_void_p), ("grid_idx", C.c_void_p), ("f_mp_state", C.c_void_p)]


class _ProjMp(C.Structure):
    _fields_ = [("n_mp", C.c_int32), ("track_in_view", C.c_void_p), ("pred_level", C.c_void_p),
                ("view_cos", C.c_void_p), ("proj_x", C.c_void_p), ("proj_y", C.c_void_p),
                ("proj_xr", C.c_void_p), ("desc", C.c_void_p), ("has_obs", C.c_void_p)]


class _ProjLast(C.Structure):
    _fields_ = [("n_last", C.c_int32), ("last_valid", C.c_void_p), ("world_pos", C.c_void_p),
                ("desc", C.c_void_p), ("last_octave", C.c_void_p), ("last_angle", C.c_void_p),
                ("has_obs", C.c_void_p), ("Tcw", C.c_float * 16), ("Tlw", C.c_float * 16),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("mb", C.c_float), ("mbf", C.c_float)]


class _ProjPoints(C.Structure):
    _fields_ = [("n_pts", C.c_int32), ("valid", C.c_void_p), ("pos", C.c_void_p), ("max_dist", C.c_void_p),
                ("min_dist", C.c_void_p), ("normal", C.c_void_p), ("desc", C.c_void_p), ("q_angle", C.c_void_p),
                ("R", C.c_float * 9), ("t", C.c_float * 3), ("Ow", C.c_float * 3), ("R2", C.c_float * 9),
                ("t2", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("bf", C.c_float), ("log_scale_factor", C.c_float), ("inv_level_sigma2", C.c_void_p), ("th", C.c_float)]


_DTYPES = dict(desc_kf=np.uint8, desc_f=np.uint8, kf_has_mp=np.uint8, angle_kf=np.float32, angle_f=np.float32,
               node_id_kf=np.int32, node_off_kf=np.int32, node_idx_kf=np.int32, node_id_f=np.int32,
               node_off_f=np.int32, node_idx_f=np.int32, kp_x=np.float32, kp_y=np.float32, kp_octave=np.int32,
               kp_angle=np.float32, u_right=np.float32, scale_factors=np.float32, grid_off=np.int32,
               grid_idx=np.int32, f_mp_state=np.uint8, track_in_view=np.uint8, pred_level=np.int32,
               view_cos=np.float32, proj_x=np.float32, proj_y=np.float32, proj_xr=np.float32, desc=np.uint8,
               has_obs=np.uint8, last_valid=np.uint8, world_pos=np.float32, last_octave=np.int32,
               last_angle=np.float32, desc1=np.uint8, desc2=np.uint8, has_mp1=np.uint8, has_mp2=np.uint8,
               angle1=np.float32, angle2=np.float32, node_id1=np.int32, node_off1=np.int32, node_idx1=np.int32,
               node_id2=np.int32, node_off2=np.int32, node_idx2=np.int32, x1=np.float32, y1=np.float32, x2=np.float32,
               y2=np.float32, u_right1=np.float32, u_right2=np.float32, octave2=np.int32, scale_factors2=np.float32,
               level_sigma2_2=np.float32, valid=np.uint8, pos=np.float32, max_dist=np.float32, min_dist=np.float32,
               normal=np.float32, q_angle=np.float32, inv_level_sigma2=np.float32)


def _fill_struct(st, d, keep):
    for name, ct in st._fields_:
        if name not in d:
            continue
        v = d[name]
        if ct is C.c_void_p:
            a = np.ascontiguousarray(v, _DTYPES[name])
            keep.append(a)
            setattr(st, name, a.ctypes.data)
        elif isinstance(v, np.ndarray) and hasattr(ct, "_length_"):
            setattr(st, name, ct(*[float(x) for x in v.reshape(-1)]))
        else:
            setattr(st, name, v.item() if hasattr(v, "item") else v)
    return st


class Matcher:
    """Mirror of ORBmatcher (include/ORBmatcher.h:37-102) over SoA snapshots."""
    TH_LOW, TH_HIGH, HISTO_LENGTH = 50, 100, 30

    def __init__(self, nnratio=0.6, check_orientation=True, device=0):
        self.L = lib()
        h = C.c_void_p()
        _check(self.L.aos2_matcher_create(float(nnratio), int(bool(check_orientation)), device, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.aos2_matcher_destroy(self.h)
            self.h = None

    __del__ = close

    def last_device_ms(self):
        return float(self.L.aos2_matcher_last_device_ms(self.h))

    @staticmethod
    def DescriptorDistance(a, b):
        a = np.ascontiguousarray(a, np.uint8)
        b = np.ascontiguousarray(b, np.uint8)
        return lib().aos2_descriptor_distance(_p(a), _p(b))

    def hamming_best2(self, q, t):
        q = np.ascontiguousarray(q, np.uint8)
        t = np.ascontiguousarray(t, np.uint8)
        bi = np.zeros(len(q), np.int32)
        bd = np.zeros(len(q), np.int32)
        sd = np.zeros(len(q), np.int32)
        _check(self.L.aos2_matcher_hamming_best2(self.h, _p(q), len(q), _p(t), len(t), _p(bi), _p(bd), _p(sd)))
        return bi, bd, sd

    def hamming_best2_device(self, d_q, nq, d_t, nt, d_bi, d_bd, d_sd, iters=1):
        ms = C.c_float(0)
        _check(self.L.aos2_matcher_hamming_best2_device(self.h, C.c_void_p(d_q), nq, C.c_void_p(d_t), nt,
                                                        C.c_void_p(d_bi), C.c_void_p(d_bd), C.c_void_p(d_sd),
                                                        iters, C.byref(ms)))
        return ms.value

    def SearchByBoW(self, problems):
        """problems: list of synth_bow_problem()-style dicts (or one dict). Returns [(nmatches, match_f)]."""
        single = isinstance(problems, dict)
        if single:
            problems = [problems]
        keep = []
        arr = (_BowPair * len(problems))()
        outs = []
        for i, p in enumerate(problems):
            d = dict(p)
            d["n_kf"], d["n_f"] = len(p["desc_kf"]), len(p["desc_f"])
            d["n_nodes_kf"], d["n_nodes_f"] = len(p["node_id_kf"]), len(p["node_id_f"])
            _fill_struct(arr[i], d, keep)
            outs.append(np.zeros(max(d["n_f"], 1), np.int32))
        ptrs = (C.c_void_p * len(problems))(*[o.ctypes.data for o in outs])
        nm = np.zeros(len(problems), np.int32)
        _check(self.L.aos2_matcher_search_by_bow(self.h, C.byref(arr), len(problems), ptrs, _p(nm)))
        res = [(int(nm[i]), outs[i][: len(problems[i]["desc_f"])]) for i in range(len(problems))]
        return res[0] if single else res

    def SearchByBoWDevice(self, pairs):
        """aos2_matcher_search_by_bow_device: pairs = list of dicts with DEVICE addresses (ints) desc_kf, desc_f, angle_kf,
        angle_f, sizes n_kf / n_f, and host arrays kf_has_mp, node_id_* / node_off_* / node_idx_* -> [(nmatches, match_f)]"""
        keep = []
        n = len(pairs)
        arr = (_BowPair * n)()
        outs = []
        for i, p in enumerate(pairs):
            a = arr[i]
            a.n_kf, a.n_f = int(p["n_kf"]), int(p["n_f"])
            a.desc_kf, a.desc_f, a.angle_kf, a.angle_f = int(p["desc_kf"]), int(p["desc_f"]), int(p["angle_kf"]), int(p["angle_f"])
            a.n_nodes_kf, a.n_nodes_f = len(p["node_id_kf"]), len(p["node_id_f"])
            for name in ("kf_has_mp", "node_id_kf", "node_off_kf", "node_idx_kf", "node_id_f", "node_off_f", "node_idx_f"):
                v = np.ascontiguousarray(p[name], _DTYPES[name])
                if v.size == 0:
                    v = np.zeros(1, _DTYPES[name])
                keep.append(v)
                setattr(a, name, v.ctypes.data)
            outs.append(np.zeros(max(a.n_f, 1), np.int32))
        ptrs = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        nm = np.zeros(n, np.int32)
        _check(self.L.aos2_matcher_search_by_bow_device(self.h, C.byref(arr), n, ptrs, _p(nm)))
        return [(int(nm[i]), outs[i][: int(pairs[i]["n_f"])]) for i in range(n)]

    def SearchByBoWFrames(self, n_frames, cap, kf_has_mp, match_f, nmatches, **dev):
        """aos2_matcher_search_by_bow_frames: dev = the device addresses (ints) named like aos2_bow_frames_t's fields;
        kf_has_mp uint8 [n][cap], match_f int32 [n][cap], nmatches int32 [n]: host arrays (filled in place)"""
        q = _BowFrames()
        q.n_frames, q.cap = int(n_frames), int(cap)
        for k, v in dev.items():
            setattr(q, k, int(v))
        q.kf_has_mp = kf_has_mp.ctypes.data
        _check(self.L.aos2_matcher_search_by_bow_frames(self.h, C.byref(q), _p(match_f), _p(nmatches)))

    def _kfkf(self, struct_t, fn, problems, *extra):
        single = isinstance(problems, dict)
        if single:
            problems = [problems]
        keep = []
        arr = (struct_t * len(problems))()
        outs = []
        for i, p in enumerate(problems):
            d = dict(p)
            d["n1"], d["n2"] = len(p["desc1"]), len(p["desc2"])
            d["n_nodes1"], d["n_nodes2"] = len(p["node_id1"]), len(p["node_id2"])
            if "scale_factors2" in p:
                d["n_levels2"] = len(p["scale_factors2"])
            _fill_struct(arr[i], d, keep)
            outs.append(np.zeros(max(d["n1"], 1), np.int32))
        ptrs = (C.c_void_p * len(problems))(*[o.ctypes.data for o in outs])
        nm = np.zeros(len(problems), np.int32)
        _check(fn(self.h, C.byref(arr), len(problems), *extra, ptrs, _p(nm)))
        res = [(int(nm[i]), outs[i][: len(problems[i]["desc1"])]) for i in range(len(problems))]
        return res[0] if single else res

    def SearchByBoWKF(self, problems):
        """SearchByBoW(pKF1, pKF2, vpMatches12) src/ORBmatcher.cc:522-655; synth_bow_kf_problem()-style dicts.
        Returns (nmatches, match12) per problem."""
        return self._kfkf(_BowKfPair, self.L.aos2_matcher_search_by_bow_kf, problems)

    def SearchForTriangulation(self, problems, only_stereo=False):
        """src/ORBmatcher.cc:657-823; synth_triang_problem()-style dicts. Returns (nmatches, vMatches12)."""
        return self._kfkf(_TriangPair, self.L.aos2_matcher_search_for_triangulation, problems, int(only_stereo))

    def ComputeDistinctiveDescriptors(self, off, desc):
        """MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:275-340) for a CSR batch of map points."""
        off = np.ascontiguousarray(off, np.int32)
        desc = np.ascontiguousarray(desc, np.uint8)
        n = len(off) - 1
        best = np.zeros(max(n, 1), np.int32)
        _check(self.L.aos2_compute_distinctive_descriptors(self.h, n, _p(off), _p(desc), _p(best)))
        return best[:n]

    def SearchByProjection(self, f, mp, th=3.0):
        keep = []
        fv = _fill_struct(_FrameView(), f, keep)
        pm = _fill_struct(_ProjMp(), mp, keep)
        match = np.zeros(max(f["n_f"], 1), np.int32)
        n = np.zeros(1, np.int32)
        _check(self.L.aos2_matcher_search_by_projection(self.h, C.byref(fv), C.byref(pm), float(th), _p(match), _p(n)))
        return int(n[0]), match[: f["n_f"]]

    def SearchByProjectionBatch(self, frames, mps, th=3.0):
        """n independent SearchByProjection(F, vpMapPoints, th) problems in one launch -> [(nmatches, match_f)]"""
        keep = []
        n = len(frames)
        fa, pa = (_FrameView * n)(), (_ProjMp * n)()
        outs = []
        for i in range(n):
            _fill_struct(fa[i], frames[i], keep)
            _fill_struct(pa[i], mps[i], keep)
            outs.append(np.zeros(max(frames[i]["n_f"], 1), np.int32))
        ptrs = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        nm = np.zeros(n, np.int32)
        _check(self.L.aos2_matcher_search_by_projection_batch(self.h, C.byref(fa), C.byref(pa), n, float(th), ptrs, _p(nm)))
        return [(int(nm[i]), outs[i][: frames[i]["n_f"]]) for i in range(n)]

    def SearchByProjectionLast(self, cur, last, th, mono):
        keep = []
        fv = _fill_struct(_FrameView(), cur, keep)
        pl = _fill_struct(_ProjLast(), last, keep)
        match = np.zeros(max(cur["n_f"], 1), np.int32)
        n = np.zeros(1, np.int32)
        _check(self.L.aos2_matcher_search_by_projection_last(self.h, C.byref(fv), C.byref(pl), float(th), int(mono),
                                                             _p(match), _p(n)))
        return int(n[0]), match[: cur["n_f"]]


    # ---- projection family; f / p: synth_proj_gen_problem()-style dicts
    def InitializerInitialize(self, problems, sentinel=None):
        """aos2_initializer_initialize: Initializer::Initialize (src/Initializer.cc) for a batch of monocular sequences; problems as
        debug_initializer_host -> one dict per problem.  `sentinel` pre-fills the result buffers (kept in self.init_last for a caller
        that expects an error and wants to see them untouched)"""
        P, R, keep, outs = _init_args(problems, sentinel)
        self.init_last = (R, outs, [bytes(R[i]) for i in range(len(problems))])
        _check(self.L.aos2_initializer_initialize(self.h, P, R, len(problems)))
        return _init_results(R, outs)

    def PnpRansac(self, problems, sentinel=None, with_counts=True):
        """aos2_pnp_ransac: the RANSAC of PnPsolver (src/PnPsolver.cc) for a batch of relocalisation candidates; problems as
        debug_pnp_host -> one dict per problem.  `sentinel` pre-fills the result buffers (kept in self.pnp_last for a caller that
        expects a refusal)"""
        P, R, keep, outs = _pnp_args(problems, sentinel, with_counts)
        self.pnp_last = (R, outs)
        _check(self.L.aos2_pnp_ransac(self.h, P, R, len(problems)))
        return _pnp_results(R, outs)

    def Fuse(self, kf, p, sim3=False):
        """search part of Fuse (src/ORBmatcher.cc:825-975, sim3: :977-1100) -> (nFused, best_idx, best_dist)"""
        keep = []
        fv = _fill_struct(_FrameView(), kf, keep)
        pp = _fill_struct(_ProjPoints(), p, keep)
        bi, bd = np.zeros(max(p["n_pts"], 1), np.int32), np.zeros(max(p["n_pts"], 1), np.int32)
        n = np.zeros(1, np.int32)
        _check(self.L.aos2_matcher_fuse(self.h, C.byref(fv), C.byref(pp), int(sim3), _p(bi), _p(bd), _p(n)))
        return int(n[0]), bi[: p["n_pts"]], bd[: p["n_pts"]]

    def SearchByProjectionKF(self, kf, p):
        """SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) :290-403 -> (nmatches, match_f)"""
        keep = []
        fv = _fill_struct(_FrameView(), kf, keep)
        pp = _fill_struct(_ProjPoints(), p, keep)
        match, n = np.zeros(max(kf["n_f"], 1), np.int32), np.zeros(1, np.int32)
        _check(self.L.aos2_matcher_search_by_projection_kf(self.h, C.byref(fv), C.byref(pp), _p(match), _p(n)))
        return int(n[0]), match[: kf["n_f"]]

    def SearchBySim3(self, kf1, kf2, p12, p21):
        """SearchBySim3 :1102-1326 -> (nFound, match12)"""
        keep = []
        a, b = _fill_struct(_FrameView(), kf1, keep), _fill_struct(_FrameView(), kf2, keep)
        c, d = _fill_struct(_ProjPoints(), p12, keep), _fill_struct(_ProjPoints(), p21, keep)
        match, n = np.zeros(max(p12["n_pts"], 1), np.int32), np.zeros(1, np.int32)
        _check(self.L.aos2_matcher_search_by_sim3(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d), _p(match), _p(n)))
        return int(n[0]), match[: p12["n_pts"]]

    def AssignFeaturesToGrid(self, kp_x, kp_y, min_x, min_y, grid_w_inv, grid_h_inv):
        """Frame::AssignFeaturesToGrid (src/Frame.cc:259-274) -> (grid_off[3073], grid_idx)"""
        kp_x, kp_y = np.ascontiguousarray(kp_x, np.float32), np.ascontiguousarray(kp_y, np.float32)
        off = np.zeros(64 * 48 + 1, np.int32)
        idx = np.zeros(max(len(kp_x), 1), np.int32)
        n = C.c_int32(0)
        _check(self.L.aos2_frame_assign_features_to_grid(self.h, len(kp_x), _p(kp_x), _p(kp_y), float(min_x), float(min_y),
                                                         float(grid_w_inv), float(grid_h_inv), _p(off), _p(idx), C.byref(n)))
        return off, idx[: n.value]

    def ComputeStereoFromRGBD(self, kp_x, kp_y, kpun_x, depth_img, mbf):
        """Frame::ComputeStereoFromRGBD (src/Frame.cc:672-693) -> (mvuRight, mvDepth)"""
        kp_x, kp_y, kpun_x = (np.ascontiguousarray(a, np.float32) for a in (kp_x, kp_y, kpun_x))
        depth_img = np.ascontiguousarray(depth_img, np.float32)
        ur, dp = np.zeros(max(len(kp_x), 1), np.float32), np.zeros(max(len(kp_x), 1), np.float32)
        _check(self.L.aos2_frame_stereo_from_rgbd(self.h, len(kp_x), _p(kp_x), _p(kp_y), _p(kpun_x), _p(depth_img),
                                                  depth_img.shape[1], depth_img.shape[0], depth_img.shape[1], float(mbf),
                                                  _p(ur), _p(dp)))
        return ur[: len(kp_x)], dp[: len(kp_x)]

    def isInFrustum(self, frame, p, viewing_cos_limit=0.5):
        """Frame::isInFrustum (src/Frame.cc:298-354) for all points of p -> dict with the aos2_proj_mp_t arrays"""
        keep = []
        pp = _fill_struct(_ProjPoints(), p, keep)
        n = p["n_pts"]
        iv = np.zeros(max(n, 1), np.uint8)
        px, py, pr, vc = (np.zeros(max(n, 1), np.float32) for _ in range(4))
        lv = np.zeros(max(n, 1), np.int32)
        _check(self.L.aos2_frame_is_in_frustum(self.h, C.byref(pp), float(frame["min_x"]), float(frame["max_x"]),
                                               float(frame["min_y"]), float(frame["max_y"]), int(frame["n_levels"]),
                                               float(viewing_cos_limit), _p(iv), _p(px), _p(py), _p(pr), _p(lv), _p(vc)))
        return dict(track_in_view=iv[:n], proj_x=px[:n], proj_y=py[:n], proj_xr=pr[:n], pred_level=lv[:n], view_cos=vc[:n])

    def SearchForInitialization(self, f2, q, window_size=100):
        """SearchForInitialization :405-520; q = dict(desc1, octave1, angle1, prev_xy) -> (nmatches, vnMatches12)"""
        keep = []
        fv = _fill_struct(_FrameView(), f2, keep)
        d1 = np.ascontiguousarray(q["desc1"], np.uint8)
        o1 = np.ascontiguousarray(q["octave1"], np.int32)
        a1 = np.ascontiguousarray(q["angle1"], np.float32)
        pv = np.ascontiguousarray(q["prev_xy"], np.float32)
        match, n = np.zeros(max(len(d1), 1), np.int32), np.zeros(1, np.int32)
        _check(self.L.aos2_matcher_search_for_initialization(self.h, C.byref(fv), len(d1), _p(d1), _p(o1), _p(a1), _p(pv),
                                                             int(window_size), _p(match), _p(n)))
        return int(n[0]), match[: len(d1)]

    def SearchByProjectionReloc(self, frame, p, orb_dist=100):
        """SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) :1472-1599 -> (nmatches, match_f)"""
        keep = []
        fv = _fill_struct(_FrameView(), frame, keep)
        pp = _fill_struct(_ProjPoints(), p, keep)
        match, n = np.zeros(max(frame["n_f"], 1), np.int32), np.zeros(1, np.int32)
        _check(self.L.aos2_matcher_search_by_projection_reloc(self.h, C.byref(fv), C.byref(pp), int(orb_dist), _p(match), _p(n)))
        return int(n[0]), match[: frame["n_f"]]

    def TriangulateMatches(self, kf1, kf2, obs1, obs2):
        """aos2_triangulate_matches: the loop body of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:290-436) for the matches of
        ONE (KF1, KF2) pair; arguments as debug_triangulate_host -> (status uint8 [n], x3D float32 [n][3])"""
        g, n, obs1, obs2, x3D, status = _triang_args(kf1, kf2, obs1, obs2)
        _check(self.L.aos2_triangulate_matches(self.h, C.byref(g), n, _p(obs1), _p(obs2), _p(x3D), _p(status)))
        return status, x3D

    def Sim3Ransac(self, problems, sentinel=None):
        """aos2_sim3_ransac: the RANSAC of Sim3Solver (src/Sim3Solver.cc) for a batch of loop candidates; problems as debug_sim3_host
        -> one dict per problem.  `sentinel` pre-fills the result buffers (kept in self.sim3_last for a caller that expects a refusal)"""
        P, R, keep, outs = _sim3_args(problems, sentinel)
        self.sim3_last = (R, outs)
        _check(self.L.aos2_sim3_ransac(self.h, P, R, len(problems)))
        return _sim3_results(R, outs)


# ------------------------------------------------------------------------------------------ local BA
class _LbaProblem(C.Structure):
    _fields_ = [("n_poses", C.c_int32), ("n_points", C.c_int32), ("n_edges", C.c_int32),
                ("pose_Tcw", C.c_void_p), ("pose_fixed", C.c_void_p), ("pose_id", C.c_void_p),
                ("point_xyz", C.c_void_p), ("point_id", C.c_void_p), ("edge_pose", C.c_void_p),
                ("edge_point", C.c_void_p), ("edge_obs", C.c_void_p), ("edge_stereo", C.c_void_p),
                ("edge_inv_sigma2", C.c_void_p),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("bf", C.c_float),
                ("stop_flag", C.c_void_p), ("iters_first", C.c_int32), ("iters_second", C.c_int32)]


class _LbaResult(C.Structure):
    _fields_ = [("pose_Tcw", C.c_void_p), ("point_xyz", C.c_void_p), ("edge_outlier", C.c_void_p),
                ("edge_chi2", C.c_void_p), ("iters_done_first", C.c_int32), ("iters_done_second", C.c_int32),
                ("final_chi2", C.c_double), ("final_lambda", C.c_double), ("ms_device", C.c_float),
                ("status", C.c_int32), ("trials_first", C.c_int32), ("trials_second", C.c_int32),
                ("polls", C.c_int32), ("stop_poll", C.c_int32)]


class _LbaSystem(C.Structure):
    _fields_ = [("np", C.c_int32), ("nl", C.c_int32), ("npad", C.c_int32), ("phase", C.c_int32), ("trials_first", C.c_int32),
                ("iters_done_first", C.c_int32), ("n_units", C.c_int32), ("lam", C.c_double), ("current_chi", C.c_double),
                ("hpose", C.c_void_p), ("hpoint", C.c_void_p), ("blk_off", C.c_void_p), ("units", C.c_void_p), ("pose", C.c_void_p),
                ("point", C.c_void_p), ("e_level1", C.c_void_p), ("e_robust", C.c_void_p), ("Hpp_init", C.c_void_p), ("b_init", C.c_void_p),
                ("b_p", C.c_void_p), ("Hll", C.c_void_p), ("b_l", C.c_void_p), ("Hs", C.c_void_p), ("bs", C.c_void_p)]


class _LbaLmState(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("lam", "ni", "currentChi", "iniChi", "final_chi2", "final_lambda")] + \
               [(k, C.c_int32) for k in ("phase", "run", "lin", "initp", "xmark", "it", "qmax", "nBad")] + \
               [("iters_done", C.c_int32 * 2), ("trials", C.c_int32 * 2)] + \
               [(k, C.c_int32) for k in ("polls", "stop_poll", "n_active", "solver_failed", "err_at", "ntr")] + \
               [(k, C.c_double * 48) for k in ("tr_rho", "tr_temp", "tr_cur", "tr_lambda")]


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


class _LbaTrialSnap(C.Structure):
    _fields_ = [("taken", C.c_int32), ("pad_", C.c_int32), ("st", _LbaLmState), ("scal3", C.c_double)] + \
               [(k, C.c_void_p) for k, _, _ in _LBA_SNAP_ARRAYS]


class _LbaTrial(C.Structure):
    _fields_ = [("np", C.c_int32), ("nl", C.c_int32), ("n_pl", C.c_int32), ("n_part", C.c_int32), ("hpose", C.c_void_p), ("hpoint", C.c_void_p),
                ("pt_off", C.c_void_p), ("pt_k", C.c_void_p), ("pl_pos", C.c_void_p), ("snap", _LbaTrialSnap * 5)]


class _PoseProblem(C.Structure):
    _fields_ = [("n", C.c_int32), ("Xw", C.c_void_p), ("obs", C.c_void_p), ("stereo", C.c_void_p),
                ("inv_sigma2", C.c_void_p), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("bf", C.c_float), ("Tcw", C.c_float * 16)]


class _PoseResult(C.Structure):
    _fields_ = [("Tcw", C.c_float * 16), ("outlier", C.c_void_p), ("n_bad", C.c_int32), ("n_inliers", C.c_int32)]


class _GbaOptions(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("robust", C.c_int32), ("huber_mono", C.c_float), ("huber_stereo", C.c_float)]


class _GbaResult(C.Structure):
    _fields_ = [("pose_Tcw", C.c_void_p), ("point_xyz", C.c_void_p), ("point_included", C.c_void_p),
                ("iterations", C.c_int32), ("trials", C.c_int32), ("chi2_initial", C.c_double), ("chi2_final", C.c_double),
                ("final_lambda", C.c_double), ("polls", C.c_int32), ("stop_poll", C.c_int32), ("h_blocks", C.c_int32),
                ("l_blocks", C.c_int32), ("ms_device", C.c_float), ("status", C.c_int32)]


GBA_HUBER = (float(np.float32(np.sqrt(5.99))), float(np.float32(np.sqrt(7.815))))       # Optimizer.cc:85-86
GBA_HUBER_LOCAL_BA = (float(np.float32(np.sqrt(5.991))), float(np.float32(np.sqrt(7.815))))   # Optimizer.cc:570-571: what the oracle uses
_GBA_SENTINEL_INT = -12345


def _gba_args(prob, iterations, robust, huber, stop_flag, sentinel=None):
    """the three structs of aos2_global_bundle_adjustment for a synth_lba_problem()-style dict; `sentinel` pre-fills the result"""
    keep = []
    s, o, r = _LbaProblem(), _GbaOptions(), _GbaResult()
    s.n_poses, s.n_points, s.n_edges = prob["n_poses"], prob["n_points"], prob["n_edges"]
    for name, dt in (("pose_Tcw", np.float32), ("pose_fixed", np.uint8), ("pose_id", np.int64), ("point_xyz", np.float32),
                     ("point_id", np.int64), ("edge_pose", np.int32), ("edge_point", np.int32), ("edge_obs", np.float32),
                     ("edge_stereo", np.uint8), ("edge_inv_sigma2", np.float32)):
        if prob.get(name) is None:   # (a test of the argument checks)
            continue
        a = np.ascontiguousarray(prob[name], dt)
        keep.append(a)
        setattr(s, name, a.ctypes.data)
    s.fx, s.fy, s.cx, s.cy, s.bf = (float(np.float32(prob[k])) for k in ("fx", "fy", "cx", "cy", "bf"))
    if stop_flag is not None:
        keep.append(stop_flag)
        s.stop_flag = stop_flag.ctypes.data
    o.iterations, o.robust, o.huber_mono, o.huber_stereo = int(iterations), int(bool(robust)), float(huber[0]), float(huber[1])
    fill = 0 if sentinel is None else sentinel
    Tout = np.full((max(s.n_poses, 1), 16), fill, np.float32)
    Pout = np.full((max(s.n_points, 1), 3), fill, np.float32)
    inc = np.full(max(s.n_points, 1), 0 if sentinel is None else 77, np.uint8)
    r.pose_Tcw, r.point_xyz, r.point_included = Tout.ctypes.data, Pout.ctypes.data, inc.ctypes.data
    if sentinel is not None:
        r.iterations = r.trials = r.status = _GBA_SENTINEL_INT
    return s, o, r, keep, (Tout[: s.n_poses], Pout[: s.n_points], inc[: s.n_points])


def _gba_result(r, arrs):
    Tout, Pout, inc = arrs
    return dict(status=r.status, pose_Tcw=Tout, point_xyz=Pout, point_included=inc, iterations=r.iterations, trials=r.trials,
                chi2_initial=r.chi2_initial, chi2_final=r.chi2_final, final_lambda=r.final_lambda, polls=r.polls,
                stop_poll=r.stop_poll, h_blocks=r.h_blocks, l_blocks=r.l_blocks, ms_device=r.ms_device)


def debug_global_ba_host(prob, iterations=10, robust=False, huber=GBA_HUBER, stop_flag=None, stop_at_poll=0, sentinel=None):
    """aos2_debug_global_ba_host: the arithmetic and the lists of the device path run serially on the CPU with a skyline solve -> the
    fields of aos2_gba_result_t"""
    s, o, r, keep, arrs = _gba_args(prob, iterations, robust, huber, stop_flag, sentinel)
    debug_global_ba_host.last = (r, arrs)
    _check(lib().aos2_debug_global_ba_host(C.byref(s), C.byref(o), C.byref(r), int(stop_at_poll)))
    return _gba_result(r, arrs)


def lba_host_phase(probs, threads):
    """aos2_lba_debug_host_phase: (build ms, stage ms) of the host part of a LocalBA batch; needs no device"""
    n = len(probs)
    keep = []
    S = (_LbaProblem * n)()
    for i, prob in enumerate(probs):
        s = S[i]
        s.n_poses, s.n_points, s.n_edges = prob["n_poses"], prob["n_points"], prob["n_edges"]
        for name, dt in (("pose_Tcw", np.float32), ("pose_fixed", np.uint8), ("pose_id", np.int64), ("point_xyz", np.float32),
                         ("point_id", np.int64), ("edge_pose", np.int32), ("edge_point", np.int32), ("edge_obs", np.float32),
                         ("edge_stereo", np.uint8), ("edge_inv_sigma2", np.float32)):
            a = np.ascontiguousarray(prob[name], dt)
            keep.append(a)
            setattr(s, name, a.ctypes.data)
    b, st = C.c_double(), C.c_double()
    _check(lib().aos2_lba_debug_host_phase(C.byref(S), n, int(threads), C.byref(b), C.byref(st)))
    return float(b.value), float(st.value)


class LocalBA:
    """Optimizer::LocalBundleAdjustment numerical part (include/Optimizer.h:45, src/Optimizer.cc:454-779)."""

    def __init__(self, device=0):
        self.L = lib()
        h = C.c_void_p()
        _check(self.L.aos2_lba_create(device, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.aos2_lba_destroy(self.h)
            self.h = None

    __del__ = close

    def _fill(self, s, r, prob, stop_flag, iters, keep):
        s.n_poses, s.n_points, s.n_edges = prob["n_poses"], prob["n_points"], prob["n_edges"]
        for name, dt in (("pose_Tcw", np.float32), ("pose_fixed", np.uint8), ("pose_id", np.int64),
                         ("point_xyz", np.float32), ("point_id", np.int64), ("edge_pose", np.int32),
                         ("edge_point", np.int32), ("edge_obs", np.float32), ("edge_stereo", np.uint8),
                         ("edge_inv_sigma2", np.float32)):
            a = np.ascontiguousarray(prob[name], dt)
            keep.append(a)
            setattr(s, name, a.ctypes.data)
        s.fx, s.fy, s.cx, s.cy, s.bf = (float(np.float32(prob[k])) for k in ("fx", "fy", "cx", "cy", "bf"))
        if stop_flag is not None:
            keep.append(stop_flag)
            s.stop_flag = stop_flag.ctypes.data
        s.iters_first, s.iters_second = iters
        Tout = np.zeros((s.n_poses, 16), np.float32)
        Pout = np.zeros((s.n_points, 3), np.float32)
        outl = np.zeros(s.n_edges, np.uint8)
        chi2 = np.zeros(s.n_edges, np.float64)
        r.pose_Tcw, r.point_xyz, r.edge_outlier, r.edge_chi2 = Tout.ctypes.data, Pout.ctypes.data, outl.ctypes.data, chi2.ctypes.data
        return Tout, Pout, outl, chi2

    @staticmethod
    def _result(r, arrs):
        Tout, Pout, outl, chi2 = arrs
        return dict(status=r.status, pose_Tcw=Tout, point_xyz=Pout, edge_outlier=outl, edge_chi2=chi2,
                    iters=(r.iters_done_first, r.iters_done_second), trials=(r.trials_first, r.trials_second),
                    final_chi2=r.final_chi2, final_lambda=r.final_lambda, ms_device=r.ms_device,
                    polls=r.polls, stop_poll=r.stop_poll)

    def LocalBundleAdjustment(self, prob, stop_flag=None, iters=(5, 10)):
        keep = []
        s, r = _LbaProblem(), _LbaResult()
        arrs = self._fill(s, r, prob, stop_flag, iters, keep)
        _check(self.L.aos2_lba_solve(self.h, C.byref(s), C.byref(r)), ok=(AOS2_OK, AOS2_ERR_STOPPED))
        return self._result(r, arrs)

    def LocalBundleAdjustmentBatch(self, probs, stop_flags=None, iters=(5, 10)):
        """aos2_lba_solve_batch: independent windows in one call."""
        n = len(probs)
        keep = []
        S, R = (_LbaProblem * n)(), (_LbaResult * n)()
        arrs = [self._fill(S[i], R[i], probs[i], None if stop_flags is None else stop_flags[i], iters, keep) for i in range(n)]
        _check(self.L.aos2_lba_solve_batch(self.h, C.byref(S), C.byref(R), n))
        return [self._result(R[i], arrs[i]) for i in range(n)]

    def prepare_batch(self, probs, iters=(5, 10), want_chi2=False):
        """ctypes problem / result arrays for repeated aos2_lba_solve_batch calls on the same inputs (bench harness)"""
        n = len(probs)
        keep = []
        S, R = (_LbaProblem * n)(), (_LbaResult * n)()
        arrs = [self._fill(S[i], R[i], probs[i], None, iters, keep) for i in range(n)]
        if not want_chi2:
            for i in range(n):
                R[i].edge_chi2 = None
        return dict(S=S, R=R, arrs=arrs, keep=keep, n=n)

    def solve_prepared(self, prep):
        _check(self.L.aos2_lba_solve_batch(self.h, C.byref(prep["S"]), C.byref(prep["R"]), prep["n"]))
        return prep["R"]

    LAYOUTS = {"slots": 0, "walk": 1}

    def debug_assemble(self, probs, layout="slots", stage=0, lam=None, iters=(5, 10)):
        """test tap aos2_debug_lba_assemble_device: the reduced system of a trial as k_lin / k_lm_init / k_schur assemble it, for a batch
        of windows -> one dict per window (include/aos2.h: aos2_lba_system_t; Hs is npad x npad, Hpp_init np x 6 x 6, Hll nl x 3 x 3)"""
        n = len(probs)
        keep = []
        S, R, O = (_LbaProblem * n)(), (_LbaResult * n)(), (_LbaSystem * n)()
        bufs = []
        for i in range(n):
            self._fill(S[i], R[i], probs[i], None, iters, keep)
            q, m, E = S[i].n_poses, S[i].n_points, S[i].n_edges
            npad = (6 * q + 15) // 16 * 16
            b = dict(hpose=np.zeros(q, np.int32), hpoint=np.zeros(m, np.int32), blk_off=np.zeros(q * (q + 1) // 2 + 1, np.int32),
                     units=np.zeros(q + q * (q - 1) // 2 + 1, np.int32), pose=np.zeros((q, 7)), point=np.zeros((m, 3)),
                     e_level1=np.zeros(E, np.uint8), e_robust=np.zeros(E, np.uint8), Hpp_init=np.zeros(36 * q), b_init=np.zeros(6 * q),
                     b_p=np.zeros(6 * q), Hll=np.zeros(9 * m), b_l=np.zeros(3 * m), Hs=np.zeros(npad * npad), bs=np.zeros(6 * q))
            for k, a in b.items():
                setattr(O[i], k, a.ctypes.data)
            bufs.append(b)
        lam_a = None if lam is None else np.ascontiguousarray(lam, np.float64)
        assert lam_a is None or lam_a.shape == (n,)
        _check(self.L.aos2_debug_lba_assemble_device(self.h, C.byref(S), n, self.LAYOUTS.get(layout, layout), int(stage),
                                                     None if lam_a is None else _p(lam_a), C.byref(O)))
        out = []
        for o, b in zip(O, bufs):
            q, m, npad = o.np, o.nl, o.npad
            out.append(dict(np=q, nl=m, npad=npad, phase=o.phase, trials_first=o.trials_first, iters_done_first=o.iters_done_first,
                            lam=o.lam, current_chi=o.current_chi, hpose=b["hpose"][:q], hpoint=b["hpoint"][:m],
                            blk_off=b["blk_off"][:q * (q + 1) // 2 + 1], units=b["units"][:o.n_units], pose=b["pose"], point=b["point"],
                            e_level1=b["e_level1"], e_robust=b["e_robust"], Hpp_init=b["Hpp_init"][:36 * q].reshape(q, 6, 6),
                            b_init=b["b_init"][:6 * q], b_p=b["b_p"][:6 * q], Hll=b["Hll"][:9 * m].reshape(m, 3, 3), b_l=b["b_l"][:3 * m],
                            Hs=b["Hs"][:npad * npad].reshape(npad, npad), bs=b["bs"][:6 * q]))
        return out

    def debug_trial(self, probs, layout="slots", trials_before=0, lam=None, force_solver_failed=None, tail=0, iters=(5, 10)):
        """test tap aos2_debug_lba_trial_device: the landmark half of a trial, the LM decision, the outlier pass and the final check,
        read between the shipped launches -> one dict per window: np, nl, n_pl, n_part, hpose, hpoint, pt_off, pt_k, pl_pos and the
        snapshots "A" .. "E" (None where `tail` did not reach): dicts of the arrays of aos2_lba_trial_snap_t, pose [n_poses, 7], point
        [n_points, 3] and their backups bk_pose, bk_point, scal3, and st = the LmState scalars (traces cut to ntr)"""
        n = len(probs)
        keep = []
        S, R, O = (_LbaProblem * n)(), (_LbaResult * n)(), (_LbaTrial * n)()
        bufs = []
        for i in range(n):
            self._fill(S[i], R[i], probs[i], None, iters, keep)
            q, m, E = S[i].n_poses, S[i].n_points, S[i].n_edges
            b = dict(hpose=np.zeros(q, np.int32), hpoint=np.zeros(m, np.int32), pt_off=np.zeros(m + 1, np.int32), pt_k=np.zeros(E, np.int32),
                     pl_pos=np.zeros(E, np.int32))
            for k, a in b.items():
                setattr(O[i], k, a.ctypes.data)
            b["snap"] = []
            for j in range(5):
                sb = {k: np.zeros(size(q, m, E), dt) for k, dt, size in _LBA_SNAP_ARRAYS}
                for k, a in sb.items():
                    setattr(O[i].snap[j], k, a.ctypes.data)
                b["snap"].append(sb)
            bufs.append(b)
        lam_a = None if lam is None else np.ascontiguousarray(lam, np.float64)
        fail_a = None if force_solver_failed is None else np.ascontiguousarray(force_solver_failed, np.uint8)
        assert (lam_a is None or lam_a.shape == (n,)) and (fail_a is None or fail_a.shape == (n,))
        _check(self.L.aos2_debug_lba_trial_device(self.h, C.byref(S), n, self.LAYOUTS.get(layout, layout), int(trials_before),
                                                  None if lam_a is None else _p(lam_a), None if fail_a is None else _p(fail_a), int(tail),
                                                  C.byref(O)))
        out = []
        for i, (o, b) in enumerate(zip(O, bufs)):
            q, m, npl = o.np, o.nl, o.n_pl
            NP, NL = S[i].n_poses, S[i].n_points
            w = dict(np=q, nl=m, n_pl=npl, n_part=o.n_part, hpose=b["hpose"][:q], hpoint=b["hpoint"][:m], pt_off=b["pt_off"][:m + 1],
                     pt_k=b["pt_k"], pl_pos=b["pl_pos"])
            for j, name in enumerate("ABCDE"):
                sn, sb = o.snap[j], b["snap"][j]
                if not sn.taken:
                    w[name] = None
                    continue
                st = {k: getattr(sn.st, k) for k, _ in _LbaLmState._fields_ if not k.startswith("tr_") and k not in ("iters_done", "trials")}
                st["iters_done"], st["trials"] = tuple(sn.st.iters_done), tuple(sn.st.trials)
                for k in ("tr_rho", "tr_temp", "tr_cur", "tr_lambda"):
                    st[k] = np.array(getattr(sn.st, k)[:sn.st.ntr], np.float64)
                d = dict(sb, st=st, scal3=sn.scal3, pose=sb["est"][:7 * NP].reshape(NP, 7), point=sb["est"][7 * NP:].reshape(NL, 3),
                         bk_pose=sb["bk"][:7 * NP].reshape(NP, 7), bk_point=sb["bk"][7 * NP:].reshape(NL, 3))
                d.update(x=sb["x"][:6 * q + 3 * m], b=sb["b"][:6 * q + 3 * m], Hll=sb["Hll"][:9 * m].reshape(m, 3, 3), Rl=sb["Rl"][:9 * q].reshape(q, 3, 3),
                         tmp=sb["tmp"][:6 * q], part=sb["part"][:2 * m], lrec=sb["lrec"][:4 * npl].reshape(npl, 4), err=sb["err"].reshape(-1, 3),
                         out_Tcw=sb["out_Tcw"].reshape(NP, 16), out_xyz=sb["out_xyz"].reshape(NL, 3))
                w[name] = d
            out.append(w)
        return out

    def set_host_threads(self, n):
        _check(self.L.aos2_lba_set_host_threads(self.h, int(n)))

    def set_window_groups(self, n):
        """0 = default, 1 = one program for all windows of a batch, 2 = two staggered window groups (include/aos2.h)"""
        _check(self.L.aos2_lba_set_window_groups(self.h, int(n)))

    def last_program(self):
        """(trial slots enqueued for every window, host rounds) of the last solve"""
        a, b = C.c_int32(), C.c_int32()
        _check(self.L.aos2_lba_last_program(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def last_window_slots(self):
        """trial slots of the last solve summed over the windows each round covered (include/aos2.h)"""
        a = C.c_int64()
        _check(self.L.aos2_lba_last_window_slots(self.h, C.byref(a)))
        return int(a.value)

    def debug_stop_at_poll(self, poll):
        _check(self.L.aos2_lba_debug_stop_at_poll(self.h, int(poll)))

    def GlobalBundleAdjustment(self, prob, iterations=10, robust=False, huber=GBA_HUBER, stop_flag=None, sentinel=None):
        """aos2_global_bundle_adjustment: Optimizer::BundleAdjustment (src/Optimizer.cc:41-237) on a synth_lba_problem()-style dict.
        The defaults are LoopClosing::RunGlobalBundleAdjustment's; `sentinel` pre-fills the result (kept in self.global_ba_last for a
        caller that expects a refusal)"""
        s, o, r, keep, arrs = _gba_args(prob, iterations, robust, huber, stop_flag, sentinel)
        self.global_ba_last = (r, arrs)
        _check(self.L.aos2_global_bundle_adjustment(self.h, C.byref(s), C.byref(o), C.byref(r)))
        return _gba_result(r, arrs)

    def global_ba_profile(self, on):
        """aos2_debug_global_ba_profile: switch the per-family events on / off -> the family ms of the last profiled call (linearise +
        sums, landmarks + update, assemble, factor_solve, begin + trial_edges + decide, prepare + finish)"""
        ms = (C.c_float * 6)()
        _check(self.L.aos2_debug_global_ba_profile(self.h, int(bool(on)), ms))
        return [float(v) for v in ms]

    def debug_global_ba_solve(self, n_blocks, rows, cols, val, diag, b, lam, x0=None):
        """aos2_debug_global_ba_solve_device: the symbolic phase and k_gba_factor_solve alone (6x6 blocks) -> (x, ok, l_blocks); x0 =
        what x holds before (kept when the solve fails)"""
        rows, cols = np.ascontiguousarray(rows, np.int32), np.ascontiguousarray(cols, np.int32)
        val = np.ascontiguousarray(val, np.float64).reshape(-1, 36)
        diag, b = np.ascontiguousarray(diag, np.float64).reshape(-1, 36), np.ascontiguousarray(b, np.float64).reshape(-1)
        if len(diag) != n_blocks or len(b) != 6 * n_blocks or not len(rows) == len(cols) == len(val):
            raise ValueError("diag [n_blocks][36], b [6 n_blocks], rows / cols / val one per triplet")
        x = np.zeros(6 * n_blocks) if x0 is None else np.array(x0, np.float64).reshape(6 * n_blocks)
        ok, lb = C.c_int32(-1), C.c_int32(-1)
        _check(self.L.aos2_debug_global_ba_solve_device(self.h, int(n_blocks), len(rows), _p(rows), _p(cols), _p(val), _p(diag), _p(b),
                                                        float(lam), _p(x), C.byref(ok), C.byref(lb)))
        return x, int(ok.value), int(lb.value)

    def debug_global_ba_reduced(self, prob, lam, n_free, robust=False, huber=GBA_HUBER):
        """aos2_debug_global_ba_reduced_device: the reduced camera system of the first linearisation at lambda = lam as the device
        assembles it -> (S [6 n_free][6 n_free] with lam on its diagonal, bs [6 n_free], h_blocks)"""
        s, o, r, keep, arrs = _gba_args(prob, 1, robust, huber, None)
        S, bs, hb = np.zeros((6 * n_free, 6 * n_free)), np.zeros(6 * n_free), C.c_int32(-1)
        _check(self.L.aos2_debug_global_ba_reduced_device(self.h, C.byref(s), C.byref(o), float(lam), int(n_free), _p(S), _p(bs), C.byref(hb)))
        return S, bs, int(hb.value)

    def PoseOptimization(self, problems):
        """int Optimizer::PoseOptimization(Frame*) (src/Optimizer.cc:239-452) for one dict or a list of
        synth_pose_problem()-style dicts (one workgroup per frame, one launch)."""
        single = isinstance(problems, dict)
        if single:
            problems = [problems]
        keep = []
        P = (_PoseProblem * len(problems))()
        R = (_PoseResult * len(problems))()
        outs = []
        for i, p in enumerate(problems):
            P[i].n = int(p["n"])
            for name, dt in (("Xw", np.float32), ("obs", np.float32), ("stereo", np.uint8), ("inv_sigma2", np.float32)):
                a = np.ascontiguousarray(p[name], dt)
                keep.append(a)
                setattr(P[i], name, a.ctypes.data)
            P[i].fx, P[i].fy, P[i].cx, P[i].cy, P[i].bf = (float(np.float32(p[k])) for k in ("fx", "fy", "cx", "cy", "bf"))
            P[i].Tcw = (C.c_float * 16)(*[float(x) for x in np.asarray(p["Tcw"], np.float32).reshape(-1)])
            o = np.zeros(max(P[i].n, 1), np.uint8)
            outs.append(o)
            R[i].outlier = o.ctypes.data
        _check(self.L.aos2_pose_optimization(self.h, C.byref(P), C.byref(R), len(problems)))
        res = [dict(n_inliers=R[i].n_inliers, n_bad=R[i].n_bad, outlier=outs[i][: P[i].n].copy(),
                    Tcw=np.array(list(R[i].Tcw), np.float32)) for i in range(len(problems))]
        return res[0] if single else res

    def pose_last_device_ms(self):
        return float(self.L.aos2_pose_optimization_last_device_ms(self.h))

    def OptimizeSim3(self, problems, sentinel=None):
        """aos2_optimize_sim3: Optimizer::OptimizeSim3 (src/Optimizer.cc:1047-1242) for a batch of loop candidates; problems as
        debug_sim3_opt_host -> one dict per problem.  `sentinel` pre-fills the result buffers (kept in self.sim3_opt_last for a caller
        that expects a refusal)"""
        P, R, keep, outs = _sim3_opt_args(problems, sentinel)
        self.sim3_opt_last = (R, outs)
        _check(self.L.aos2_optimize_sim3(self.h, P, R, len(problems)))
        return _sim3_opt_results(R, outs)

    def debug_sim3_opt_steps(self, items, sentinel=0x5A):
        """aos2_debug_sim3_opt_steps_device: linearise / trial / reject of the device's edges alone; items and result as
        debug_sim3_opt_steps_host"""
        I, keep, outs = _sim3_opt_steps_args(items, sentinel)
        _check(self.L.aos2_debug_sim3_opt_steps_device(self.h, I, len(items)))
        return outs

    def sim3_opt_last_device_ms(self):
        return float(self.L.aos2_optimize_sim3_last_device_ms(self.h))

    def optimize_essential_graph(self, problems, sentinel=None):
        """aos2_optimize_essential_graph: Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:782-1045) for a batch of pose graphs;
        problems as debug_essential_graph_host -> one dict per problem.  `sentinel` pre-fills the result buffers (kept in
        self.essential_graph_last for a caller that expects a refusal)"""
        P, R, keep, outs = _essential_graph_args(problems, sentinel)
        self.essential_graph_last = (R, outs)
        _check(self.L.aos2_optimize_essential_graph(self.h, P, R, len(problems)))
        return _essential_graph_results(R, outs)

    def essential_graph_last_device_ms(self):
        return float(self.L.aos2_optimize_essential_graph_last_device_ms(self.h))

    def essential_graph_profile(self, on):
        """aos2_debug_essential_graph_profile: switch the per-family events on / off -> the family ms of the last profiled call
        (perturb + linearise, assemble, factor_solve, begin + trial, finish)"""
        ms = (C.c_float * 5)()
        _check(self.L.aos2_debug_essential_graph_profile(self.h, int(bool(on)), ms))
        return [float(v) for v in ms]

    def debug_essential_graph_solve(self, n_blocks, rows, cols, val, diag, b, lam, x0=None):
        """aos2_debug_essential_graph_solve_device: the symbolic phase and k_eg_factor_solve alone -> (x, ok, l_blocks); x0 = what x
        holds before (kept when the solve fails)"""
        rows, cols = np.ascontiguousarray(rows, np.int32), np.ascontiguousarray(cols, np.int32)
        val = np.ascontiguousarray(val, np.float64).reshape(-1, 49)
        diag, b = np.ascontiguousarray(diag, np.float64).reshape(-1, 49), np.ascontiguousarray(b, np.float64).reshape(-1)
        if len(diag) != n_blocks or len(b) != 7 * n_blocks or not len(rows) == len(cols) == len(val):
            raise ValueError("diag [n_blocks][49], b [7 n_blocks], rows / cols / val one per triplet")
        x = np.zeros(7 * n_blocks) if x0 is None else np.array(x0, np.float64).reshape(7 * n_blocks)
        ok, lb = C.c_int32(-1), C.c_int32(-1)
        _check(self.L.aos2_debug_essential_graph_solve_device(self.h, int(n_blocks), len(rows), _p(rows), _p(cols), _p(val), _p(diag), _p(b),
                                                              float(lam), _p(x), C.byref(ok), C.byref(lb)))
        return x, int(ok.value), int(lb.value)

    def debug_essential_graph_linearised(self, problem):
        """aos2_debug_essential_graph_linearised_device: the first linearisation of one problem as the device forms it -> dict(J
        [ne][2][7][7] (a fixed side keeps the bytes 0x5A), E [ne][7], H [7 nf][7 nf], b [7 nf], chi2, chi2_initial, l_blocks)"""
        P, R, keep, outs = _essential_graph_args([problem])
        ne, nf = max(int(P[0].n_edges), 0), max(int(P[0].n_vertices) - 1, 0)
        J, E = np.zeros((ne, 2, 7, 7)), np.zeros((ne, 7))
        H, b, chi = np.zeros((7 * nf, 7 * nf)), np.zeros(7 * nf), np.zeros(2)
        lb = C.c_int32(-1)
        _check(self.L.aos2_debug_essential_graph_linearised_device(self.h, P, _p(J), _p(E), _p(H), _p(b), _p(chi), C.byref(lb)))
        return dict(J=J, E=E, H=H, b=b, chi2=float(chi[0]), chi2_initial=float(chi[1]), l_blocks=int(lb.value))

    EG_CONTROL_D = ("lambda", "ni", "currentChi", "iniChi", "rho", "chi2_initial")
    EG_CONTROL_I = ("nBad", "qmax", "open", "running", "solved", "max_iterations", "iterations", "trials", "rejected", "accepted_first")

    def debug_essential_graph_trial(self, problem, x, lam, current_chi, ni=2.0, solved=1, iterations=0, qmax=0):
        """aos2_debug_essential_graph_trial_device: one k_eg_trial on one problem with the solver's vector x and the seeded control
        words -> dict(est_try, est [nv][8], control (the words of EG_CONTROL_D / EG_CONTROL_I by name), tempChi, scale)"""
        P, R, keep, outs = _essential_graph_args([problem])
        nv, nf = max(int(P[0].n_vertices), 0), max(int(P[0].n_vertices) - 1, 0)
        x = np.ascontiguousarray(x, np.float64).reshape(-1)
        if len(x) != 7 * nf:
            raise ValueError("x [7 (n_vertices - 1)]")
        seed_d, seed_i = np.array([lam, current_chi, ni], np.float64), np.array([solved, iterations, qmax], np.int32)
        est_try, est = np.zeros((nv, 8)), np.zeros((nv, 8))
        cd, ci, sums = np.zeros(6), np.zeros(10, np.int32), np.zeros(2)
        _check(self.L.aos2_debug_essential_graph_trial_device(self.h, P, _p(x), _p(seed_d), _p(seed_i), _p(est_try), _p(est), _p(cd), _p(ci), _p(sums)))
        control = dict(zip(self.EG_CONTROL_D, (float(v) for v in cd)))
        control.update(zip(self.EG_CONTROL_I, (int(v) for v in ci)))
        return dict(est_try=est_try, est=est, control=control, tempChi=float(sums[0]), scale=float(sums[1]))


# ---------------------------------------------------------------------------------------------------------------
# Device-resident frame batches (include/aos2.h: aos2_frames_*).  Device arrays are passed as raw pointers (torch
# tensors' data_ptr()); this wrapper owns nothing but the handle.
class _MapPointsDev(C.Structure):
    _fields_ = [("n", C.c_int32), ("pos", C.c_void_p), ("desc", C.c_void_p), ("has_obs", C.c_void_p),
                ("normal", C.c_void_p), ("min_dist", C.c_void_p), ("max_dist", C.c_void_p)]


def map_points_dev(n, pos, desc, has_obs, normal=0, min_dist=0, max_dist=0):
    """aos2_map_points_dev_t from device pointers (ints)"""
    t = _MapPointsDev()
    t.n, t.pos, t.desc, t.has_obs, t.normal, t.min_dist, t.max_dist = int(n), pos, desc, has_obs, normal or None, min_dist or None, max_dist or None
    return t


def frame_image_bounds(w, h, fx, fy, cx, cy, dist):
    """Frame::ComputeImageBounds (src/Frame.cc:463-493) -> (mnMinX, mnMaxX, mnMinY, mnMaxY)"""
    d = np.zeros(5, np.float32)
    d[: len(dist)] = np.asarray(dist, np.float32)
    out = np.zeros(4, np.float32)
    _check(lib().aos2_frame_image_bounds(int(w), int(h), float(fx), float(fy), float(cx), float(cy), _p(d), _p(out)))
    return out


class _FramesTriang(C.Structure):
    _fields_ = [("n_pairs", C.c_int32)] + [(k, C.c_void_p) for k in ("kf1", "kf2", "F12", "epipole", "d_node_of1", "d_fv_node1", "d_fv_off1",
                                                                      "d_fv_idx1", "d_n_fv1", "d_fv_node2", "d_fv_off2", "d_fv_idx2", "d_n_fv2")]


class Frames:
    MAP_POINTS, OUTLIER, TCW, U_RIGHT, DEPTH, GRID_OFF, GRID_IDX, KEYS_UN_X, KEYS_UN_Y = range(9)

    def __init__(self, batch, cap, device=0):
        self.L = lib()
        h = C.c_void_p()
        _check(self.L.aos2_frames_create(device, batch, cap, C.byref(h)))
        self.h, self.batch, self.cap = h, batch, cap

    def close(self):
        if getattr(self, "h", None):
            self.L.aos2_frames_destroy(self.h)
            self.h = None

    __del__ = close

    def build(self, extractor, d_kps, d_desc, d_n, w, h, d_depth, fx, fy, cx, cy, mbf, depth_stride=None, depth_image_stride=None):
        _check(self.L.aos2_frames_build(self.h, extractor.h, self.batch, d_kps, d_desc, d_n, self.cap, w, h, d_depth or None,
                                        depth_stride or w, depth_image_stride or w * h, fx, fy, cx, cy, mbf))

    def build_stereo(self, extractor_left, d_kps, d_desc, d_n, w, h, d_u_right, d_depth_kp, fx, fy, cx, cy, mbf):
        """Frame::Frame(imLeft, imRight, ...) after ExtractORB x 2 + ComputeStereoMatches (src/Frame.cc:57-113)"""
        _check(self.L.aos2_frames_build_stereo(self.h, extractor_left.h, self.batch, d_kps, d_desc, d_n, self.cap, w, h, d_u_right, d_depth_kp,
                                               fx, fy, cx, cy, mbf))

    def set_pose(self, d_Tcw):
        _check(self.L.aos2_frames_set_pose(self.h, d_Tcw))

    def set_distortion(self, dist):
        """mDistCoef = k1 k2 p1 p2 k3 for the following build() calls"""
        d = list(dist) + [0.0] * (5 - len(dist))
        _check(self.L.aos2_frames_set_distortion(self.h, *[float(v) for v in d[:5]]))

    def set_map_points(self, mp, table, outlier=None):
        mp = np.ascontiguousarray(mp, np.int32).reshape(self.batch, self.cap)
        if outlier is not None:
            outlier = np.ascontiguousarray(outlier, np.uint8).reshape(self.batch, self.cap)
        _check(self.L.aos2_frames_set_map_points(self.h, _p(mp), None if outlier is None else _p(outlier), C.byref(table)))

    def get(self, what):
        B, cap = self.batch, self.cap
        shape, dt = {0: ((B, cap), np.int32), 1: ((B, cap), np.uint8), 2: ((B, 16), np.float32), 3: ((B, cap), np.float32),
                     4: ((B, cap), np.float32), 5: ((B, 64 * 48 + 1), np.int32), 6: ((B, cap), np.int32), 7: ((B, cap), np.float32),
                     8: ((B, cap), np.float32)}.get(what, ((B, cap), np.int32))   # (any other id: the library refuses it, whatever the size)
        a = np.zeros(shape, dt)
        _check(self.L.aos2_frames_get(self.h, what, _p(a), a.nbytes))
        return a

    def SearchByProjectionLast(self, last, table, th, mono=False, check_orientation=True, d_nmatches=0):
        _check(self.L.aos2_frames_search_by_projection_last(self.h, last.h, C.byref(table), th, int(mono), int(check_orientation),
                                                            d_nmatches or None))

    def PoseOptimization(self, table, d_inliers=0):
        _check(self.L.aos2_frames_pose_optimization(self.h, C.byref(table), d_inliers or None))

    def discard_outliers(self):
        _check(self.L.aos2_frames_discard_outliers(self.h))

    def SearchLocalPoints(self, table, d_local, n_local, th, nnratio, d_nmatches=0):
        _check(self.L.aos2_frames_search_local_points(self.h, C.byref(table), d_local, n_local, th, nnratio, d_nmatches or None))

    def set_async_keyframe_calls(self, on=True):
        """SearchForTriangulation / Fuse of this handle return after enqueueing (include/aos2.h); wait() completes them"""
        self.L.aos2_frames_set_async_keyframe_calls.argtypes = [C.c_void_p, C.c_int]
        _check(self.L.aos2_frames_set_async_keyframe_calls(self.h, 1 if on else 0))

    def wait(self):
        _check(self.L.aos2_frames_wait(self.h))

    def stream(self):
        return self.L.aos2_frames_stream(self.h)

    KEYS_ANGLE, KEYS_OCTAVE = 9, 10

    def device_ptr(self, what):
        """device address (int) of a member array [batch][cap]"""
        return self.L.aos2_frames_device_ptr(self.h, int(what)) or 0

    def SearchForTriangulation(self, other, kf1, kf2, F12, epipole, d_node_of1, fv1, fv2, d_match12, d_nmatches,
                               only_stereo=False, check_orientation=True):
        """aos2_frames_search_for_triangulation: pairs (frame kf1[p] of this batch, frame kf2[p] of `other`); kf1 / kf2 int32 [n], F12 float32
        [n][9], epipole float32 [n][2]: host arrays; d_node_of1 and fv1 / fv2 = (fv_node, fv_off, fv_idx, n_fv): device addresses (ints);
        results in d_match12 [n][cap], d_nmatches [n]"""
        kf1, kf2 = np.ascontiguousarray(kf1, np.int32), np.ascontiguousarray(kf2, np.int32)
        F12, epipole = np.ascontiguousarray(F12, np.float32), np.ascontiguousarray(epipole, np.float32)
        q = _FramesTriang()
        q.n_pairs = len(kf1)
        q.kf1, q.kf2, q.F12, q.epipole = kf1.ctypes.data, kf2.ctypes.data, F12.ctypes.data, epipole.ctypes.data
        q.d_node_of1 = int(d_node_of1)
        q.d_fv_node1, q.d_fv_off1, q.d_fv_idx1, q.d_n_fv1 = (int(x) for x in fv1)
        q.d_fv_node2, q.d_fv_off2, q.d_fv_idx2, q.d_n_fv2 = (int(x) for x in fv2)
        _check(self.L.aos2_frames_search_for_triangulation(self.h, other.h, C.byref(q), int(only_stereo), int(check_orientation), d_match12, d_nmatches))

    def Fuse(self, table, target, d_rows, n_pts, th, d_best_idx, d_best_dist):
        """aos2_frames_fuse: target int32 [n] host (frames of this batch), d_rows device [n][n_pts] table rows (-1 = rejected by the loop head)"""
        target = np.ascontiguousarray(target, np.int32)
        _check(self.L.aos2_frames_fuse(self.h, C.byref(table), len(target), int(n_pts), target.ctypes.data, d_rows, float(th), d_best_idx, d_best_dist))

    def TriangulateMatches(self, other, kf1, kf2, d_match12, d_x3D, d_status, d_nnew, first_wins=True):
        """aos2_frames_triangulate_matches: the loop body of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:290-436) for the pairs
        (frame kf1[p] of this batch, frame kf2[p] of `other`) and the d_match12 [n][cap] SearchForTriangulation wrote for them; results in
        d_x3D float32 [n][cap][3], d_status uint8 [n][cap] (capi.TRI_*), d_nnew int32 [n]: device addresses (ints)"""
        kf1, kf2 = np.ascontiguousarray(kf1, np.int32), np.ascontiguousarray(kf2, np.int32)
        _check(self.L.aos2_frames_triangulate_matches(self.h, other.h, len(kf1), kf1.ctypes.data, kf2.ctypes.data, d_match12, int(bool(first_wins)),
                                                      d_x3D, d_status, d_nnew))

    def wait_for_stream(self, hip_stream=None):
        """device-side ordering: what is enqueued on the batch from now on runs behind the work on `hip_stream` so far"""
        _check(self.L.aos2_frames_wait_for_stream(self.h, hip_stream))
