"""ctypes binding of include/scl_engine.h + a Python mirror of the reference's plugin class.

``ScanContextEngine`` exposes the C ABI one-to-one (numpy arrays in / out).
``ScanContextDescriptor`` mirrors ``scan_context_descriptor`` (reference
include/descriptor.h:1304-1801): same constructor arguments, same six method names,
same return conventions (``(-1, 0.0)`` = no loop).
"""
import ctypes
import os
from ctypes import POINTER, byref, c_char_p, c_double, c_float, c_int, c_int8, c_uint64, c_void_p

import numpy as np

from ._native import load_library

QUERY_STAGED = -1


class SclConfig(ctypes.Structure):
    """scl_config; defaults = scan_context_descriptor ctor defaults (D.h:1308-1316)."""
    _fields_ = [
        ("num_ring", c_int), ("num_sector", c_int), ("num_candidates", c_int),
        ("dist_thres", c_double), ("lidar_height", c_double), ("max_radius", c_double),
        ("num_exclude_recent", c_int), ("tree_making_period", c_int),
        ("search_ratio", c_double), ("knn_exclude_eps", c_float),
        ("device", c_int), ("initial_capacity", c_int),
    ]


class IcpParams(ctypes.Structure):
    """scl_icp_params; defaults = the settings at DM.h:1109-1112."""
    _fields_ = [
        ("max_iterations", c_int), ("max_correspondence_dist", c_double),
        ("transformation_epsilon", c_double), ("euclidean_fitness_epsilon", c_double),
        ("estimator", c_int), ("normal_radius", c_double),
    ]


class PgoParams(ctypes.Structure):
    """scl_pgo_params; PgoParams.defaults() = scl_pgo_default_params (the project's own choice: scl_engine.h POSE-GRAPH SOLVE)."""
    _fields_ = [
        ("max_iterations", c_int), ("lambda_initial", c_double), ("lambda_factor", c_double), ("lambda_max", c_double),
        ("relative_cost_tolerance", c_double), ("step_tolerance", c_double), ("cg_tolerance", c_double), ("cg_max_iterations", c_int),
    ]

    @classmethod
    def defaults(cls, **overrides):
        lib = load_library(); _bind(lib)
        p = cls()
        rc = lib.scl_pgo_default_params(byref(p))
        if rc != 0:
            raise SclError(rc, "scl_pgo_default_params")
        for k, v in overrides.items():
            if k not in dict(cls._fields_):
                raise TypeError(f"scl_pgo_params has no field {k}")
            setattr(p, k, v)
        return p


class PgoResult(ctypes.Structure):
    """scl_pgo_result; stop_reason: 1 cost, 2 step, 3 iterations, 4 lambda"""
    _fields_ = [
        ("iterations", c_int), ("accepted", c_int), ("rejected", c_int), ("cg_iterations", c_int), ("stop_reason", c_int),
        ("initial_cost", c_double), ("final_cost", c_double), ("final_lambda", c_double), ("gradient_max", c_double),
    ]
    STOP_COST, STOP_STEP, STOP_ITERATIONS, STOP_LAMBDA = 1, 2, 3, 4


class MapStats(ctypes.Structure):
    """struct scl_map_stats (scl_engine.h GLOBAL MAP)"""
    _fields_ = [
        ("keyframes", c_uint64), ("points_added", c_uint64), ("points_skipped", c_uint64), ("occupied_voxels", c_uint64),
        ("capacity", c_uint64), ("growths", c_uint64),
    ]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


MAP_RECORD = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("n", "<u4")])   # a record of scl_map_extract


class SclProfile(ctypes.Structure):
    _fields_ = [
        ("sc_distance_ms", c_double), ("sc_distance_launches", c_uint64), ("sc_distance_pairs", c_uint64),
        ("ringkey_topk_ms", c_double), ("ringkey_topk_launches", c_uint64),
        ("argmin_ms", c_double), ("argmin_launches", c_uint64),
        ("make_sc_ms", c_double), ("make_sc_launches", c_uint64), ("make_sc_points", c_uint64),
        ("ingest_ms", c_double), ("ingest_launches", c_uint64),
        ("icp_nn_ms", c_double), ("icp_nn_launches", c_uint64),
        ("icp_reduce_ms", c_double), ("icp_reduce_launches", c_uint64),
    ]


class SclError(RuntimeError):
    def __init__(self, status, where, detail=""):
        self.status = status
        super().__init__(f"{where}: status {status}" + (f" ({detail})" if detail else ""))


_bound = False


def _bind(lib):
    global _bound
    if _bound:
        return
    P = c_void_p
    fp, dp, ip = POINTER(c_float), POINTER(c_double), POINTER(c_int)
    sig = {
        "scl_status_string": (c_char_p, [c_int]),
        "scl_last_error": (c_char_p, [P]),
        "scl_abi_version": (c_int, []),
        "scl_default_config": (c_int, [POINTER(SclConfig)]),
        "scl_create": (c_int, [POINTER(SclConfig), POINTER(P)]),
        "scl_create_sharded": (c_int, [POINTER(SclConfig), ip, c_int, c_int, POINTER(P)]),
        "scl_shard_info": (c_int, [P, ip, ip]),
        "scl_destroy": (c_int, [P]),
        "scl_make_and_save": (c_int, [P, P, c_int, c_int, c_int8, c_int, fp]),
        "scl_save_from_wire": (c_int, [P, fp, c_int8, c_int]),
        "scl_make_and_save_filtered": (c_int, [P, P, c_int, c_int, c_float, c_int8, c_int, fp, ip]),
        "scl_detect_intra": (c_int, [P, c_int, ip, fp, dp]),
        "scl_detect_inter": (c_int, [P, c_int, ip, fp, dp]),
        "scl_get_index": (c_int, [P, c_int, POINTER(c_int8), ip]),
        "scl_get_size": (c_int, [P, c_int]),
        "scl_make_descriptor": (c_int, [P, P, c_int, c_int, fp]),
        "scl_save_bulk": (c_int, [P, fp, c_int, POINTER(c_int8), ip]),
        "scl_get_descriptor": (c_int, [P, c_int, fp]),
        "scl_get_ringkey": (c_int, [P, c_int, fp]),
        "scl_get_sectorkey": (c_int, [P, c_int, dp]),
        "scl_get_descriptors": (c_int, [P, c_int, c_int, fp]),
        "scl_find_key": (c_int, [P, c_int8, c_int, ip]),
        "scl_db_dump_file": (c_int, [P, c_char_p]),
        "scl_db_load_file": (c_int, [P, c_char_p, ip]),
        "scl_matrix_to_pose": (c_int, [fp, fp, fp, fp, fp, fp, fp]),
        "scl_loop_pose_between": (c_int, [fp, fp, fp, dp, dp]),
        "scl_stage_query": (c_int, [P, fp]),
        "scl_ringkey_topk": (c_int, [P, c_int, c_int, c_int, c_int, ip, fp, ip]),
        "scl_sc_distance_batch": (c_int, [P, c_int, ip, c_int, dp, ip]),
        "scl_sc_distance_matrix": (c_int, [P, ip, c_int, c_int, c_int, dp, ip]),
        "scl_sc_search_range": (c_int, [P, ip, ip, ip, c_int, c_int, ip, ip, dp, ip]),
        "scl_sc_search": (c_int, [P, ip, c_int, c_int, ip, ip, dp, ip]),
        "scl_sc_search_intra": (c_int, [P, ip, c_int, c_int, ip, ip, dp, ip]),
        "scl_sc_search_inter": (c_int, [P, ip, c_int, c_int, c_int, ip, ip, dp, ip]),
        "scl_detect_full": (c_int, [P, c_int, ip, ip, ip, dp]),
        "scl_detect_full_range": (c_int, [P, c_int, c_int, c_int, ip, ip, dp]),
        "scl_get_last_topk": (c_int, [P, c_int, ip, fp]),
        "scl_screen_distances": (c_int, [P, c_int, c_int, c_int, fp, ip, ip, fp]),
        "scl_screen_distances_many": (c_int, [P, ip, c_int, c_int, c_int, fp, fp]),
        "scl_detect_full_submit": (c_int, [P, c_int, c_int, c_int, ip]),
        "scl_detect_full_collect": (c_int, [P, c_int, ip, ip, dp]),
        "scl_detect_full_submit_many": (c_int, [P, ip, ip, ip, c_int, ip]),
        "scl_detect_full_stream": (c_int, [P, ip, ip, ip, c_int, c_int, c_int, ip, ip, dp]),
        "scl_topk_with_distance": (c_int, [P, c_int, c_int, c_int, c_int, ip, fp, dp, ip, ip]),
        "scl_icp_default_params": (c_int, [POINTER(IcpParams)]),
        "scl_icp_align": (c_int, [P, P, c_int, P, c_int, c_int, POINTER(IcpParams), fp, fp, ip, ip]),
        "scl_icp_align_batch": (c_int, [P, P, c_int, POINTER(c_void_p), ip, c_int, c_int, POINTER(IcpParams), fp, fp, ip, ip]),
        "scl_nn_correspondences": (c_int, [P, P, c_int, P, c_int, c_int, ip, fp]),
        "scl_nn_correspondences_moved": (c_int, [P, P, c_int, P, c_int, c_int, fp, ip, fp]),
        "scl_rigid_svd": (c_int, [P, P, c_int, P, c_int, c_int, ip, ip, c_int, fp]),
        "scl_transform_cloud": (c_int, [P, P, c_int, c_int, fp, P]),
        "scl_voxel_grid": (c_int, [P, P, c_int, c_int, c_float, P, c_int, ip]),
        "scl_pose_to_matrix": (c_int, [c_float, c_float, c_float, c_float, c_float, c_float, fp]),
        "scl_assemble_submap": (c_int, [P, POINTER(c_void_p), ip, fp, c_int, c_int, c_float, P, c_int, ip]),
        "scl_ransac_correspondences": (c_int, [P, P, c_int, P, c_int, c_int, ip, ip, c_int, c_int, c_double, c_uint64, ip, ip, ip, fp]),
        "scl_geometric_verification": (c_int, [P, P, c_int, P, c_int, c_int, c_int, c_double, c_double, c_uint64, fp, ip, ip, ip]),
        "scl_keyframe_put": (c_int, [P, c_int, c_int, P, c_int, c_int]),
        "scl_keyframe_count": (c_int, [P, c_int]),
        "scl_keyframe_get": (c_int, [P, c_int, c_int, P, c_int, ip]),
        "scl_submap_from_store": (c_int, [P, c_int, c_int, c_int, fp, c_float, P, c_int, ip]),
        "scl_loop_icp_from_store": (c_int, [P, c_int, c_int, fp, c_int, c_int, fp, c_float, POINTER(IcpParams), c_int, c_int,
                                            fp, fp, ip, ip, ip, ip]),
        "scl_loop_icp_batch_from_store": (c_int, [P, c_int, c_int, fp, c_int, ip, c_int, fp, c_float, POINTER(IcpParams), c_int, c_int,
                                                  fp, fp, ip, ip, ip, ip]),
        "scl_geometric_verification_from_store": (c_int, [P, P, c_int, c_int, c_float, c_int, c_int, c_int, fp, c_float, c_int, c_int,
                                                          c_int, c_double, c_double, c_uint64, fp, ip, ip, ip, ip, ip]),
        "scl_geometric_verification_batch": (c_int, [P, P, c_int, POINTER(c_void_p), ip, c_int, c_int, c_int, c_double, c_double, c_uint64,
                                                     fp, ip, ip, ip]),
        "scl_geometric_verification_batch_from_store": (c_int, [P, P, c_int, c_int, c_float, c_int, c_int, ip, c_int, fp, c_float, c_int, c_int,
                                                                c_int, c_double, c_double, c_uint64, fp, ip, ip, ip, ip, ip]),
        "scl_geometric_verification_batch_guess": (c_int, [P, P, c_int, POINTER(c_void_p), ip, c_int, c_int, fp, c_int, c_double, c_double, c_uint64,
                                                           fp, fp, ip, ip, ip]),
        "scl_geometric_verification_batch_from_store_guess": (c_int, [P, P, c_int, c_int, c_float, c_int, c_int, ip, c_int, fp, c_float, fp, c_int, c_int,
                                                                      c_int, c_double, c_double, c_uint64, fp, fp, ip, ip, ip, ip, ip]),
        "scl_loop_guess_from_shift": (c_int, [c_int, c_int, fp, fp, fp]),
        "scl_icp_align_batch_guess": (c_int, [P, P, c_int, POINTER(c_void_p), ip, c_int, c_int, fp, POINTER(IcpParams), fp, fp, fp, ip, ip]),
        "scl_loop_icp_batch_from_store_guess": (c_int, [P, c_int, c_int, fp, c_int, ip, c_int, fp, c_float, fp, POINTER(IcpParams), c_int, c_int,
                                                        fp, fp, fp, ip, ip, ip, ip]),
        "scl_icp_align_batch_from_store_guess": (c_int, [P, P, c_int, c_int, c_float, c_int, c_int, ip, c_int, fp, c_float, fp, POINTER(IcpParams),
                                                         c_int, c_int, fp, fp, fp, ip, ip, ip, ip]),
        "scl_registration_eval_batch": (c_int, [P, P, c_int, POINTER(c_void_p), ip, c_int, c_int, fp, c_double, ip, ip, dp]),
        "scl_registration_eval_batch_from_store": (c_int, [P, P, c_int, c_int, c_float, c_int, c_int, ip, c_int, fp, c_float, fp, c_int, c_int,
                                                           c_double, ip, ip, dp, ip, ip]),
        "scl_loop_eval_batch_from_store": (c_int, [P, c_int, c_int, fp, c_int, ip, c_int, fp, c_float, fp, c_int, c_int, c_double,
                                                   ip, ip, dp, ip, ip]),
        "scl_registration_information": (c_int, [c_int, dp, dp]),
        "scl_target_normals": (c_int, [P, P, c_int, c_int, c_double, fp]),
        "scl_registration_eval_plane_batch": (c_int, [P, P, c_int, POINTER(c_void_p), ip, c_int, c_int, fp, c_double, c_double, ip, ip, ip, dp]),
        "scl_registration_eval_plane_batch_from_store": (c_int, [P, P, c_int, c_int, c_float, c_int, c_int, ip, c_int, fp, c_float, fp, c_int, c_int,
                                                                 c_double, c_double, ip, ip, ip, dp, ip, ip]),
        "scl_loop_eval_plane_batch_from_store": (c_int, [P, c_int, c_int, fp, c_int, ip, c_int, fp, c_float, fp, c_int, c_int, c_double, c_double,
                                                         ip, ip, ip, dp, ip, ip]),
        "scl_registration_information_plane": (c_int, [dp, dp, dp]),
        "scl_pcm_consistency": (c_int, [P, dp, c_int, dp, c_int, ip, ip, dp, dp, c_int, dp, c_double, dp, POINTER(c_uint64), ip]),
        "scl_pcm_max_clique": (c_int, [P, POINTER(c_uint64), c_int, ip, ip, ip]),
        "scl_pcm_select": (c_int, [P, dp, c_int, dp, c_int, ip, ip, dp, dp, c_int, dp, c_double, ip, ip, ip, ip]),
        "scl_pcm_last_timing": (c_int, [P, dp, dp]),
        "scl_loop_covariance": (c_int, [dp, c_double, dp]),
        "scl_pgo_default_params": (c_int, [POINTER(PgoParams)]),
        "scl_pgo_linearize": (c_int, [P, dp, c_int, ip, ip, dp, dp, c_int, ip, dp, dp, c_int, dp, dp, dp, dp]),
        "scl_pgo_hessian_apply": (c_int, [P, dp, c_int, ip, ip, dp, dp, c_int, ip, dp, dp, c_int, c_double, dp, dp]),
        "scl_pgo_optimize": (c_int, [P, dp, c_int, ip, ip, dp, dp, c_int, ip, dp, dp, c_int, POINTER(PgoParams), dp, POINTER(PgoResult), dp]),
        "scl_pgo_last_timing": (c_int, [P, dp, dp]),
        "scl_pgo_count_junctions": (c_int, [c_int, ip, ip, c_int, ip, c_int, ip, ip, ip]),
        "scl_pgo_solve_condensed": (c_int, [P, dp, c_int, ip, ip, dp, dp, c_int, ip, dp, dp, c_int, c_double, dp]),
        "scl_pgo_optimize_condensed": (c_int, [P, dp, c_int, ip, ip, dp, dp, c_int, ip, dp, dp, c_int, POINTER(PgoParams), dp, POINTER(PgoResult), dp,
                                               ip]),
        "scl_pgo_condensed_last_timing": (c_int, [P, dp]),
        "scl_pgo_solve_condensed_many": (c_int, [P, dp, c_int, ip, ip, dp, dp, c_int, ip, dp, dp, c_int, c_double, dp, c_int, dp]),
        "scl_pgo_marginals": (c_int, [P, dp, c_int, ip, ip, dp, dp, c_int, ip, dp, dp, c_int, ip, ip, c_int, dp, dp]),
        "scl_map_reset": (c_int, [P, c_float]),
        "scl_map_set_keyframes": (c_int, [P, ip, ip, dp, c_int]),
        "scl_map_remove_keyframes": (c_int, [P, ip, ip, c_int]),
        "scl_map_extract": (c_int, [P, dp, c_void_p, c_int, ip]),
        "scl_map_stats": (c_int, [P, POINTER(MapStats)]),
        "scl_map_last_timing": (c_int, [P, dp]),
        "scl_selftest_map_capacity": (c_int, [P, c_uint64]),
        "scl_profile_enable": (c_int, [P, c_int]),
        "scl_profile_reset": (c_int, [P]),
        "scl_profile_get": (c_int, [P, POINTER(SclProfile)]),
        "scl_alignment_stats": (c_int, [P, POINTER(ctypes.c_uint64), POINTER(ctypes.c_uint64), c_int]),
        "scl_survivor_stats": (c_int, [P, POINTER(ctypes.c_uint64), POINTER(ctypes.c_uint64), POINTER(ctypes.c_uint64), c_int]),
        "scl_device_name": (c_int, [P, c_char_p, c_int]),
        "scl_make_and_save_many": (c_int, [P, POINTER(c_void_p), ip, c_int, c_int, POINTER(c_int8), ip, fp]),
        "scl_stream_from_points": (c_int, [P, POINTER(c_void_p), ip, c_int, c_int, POINTER(c_int8), ip, ip, ip, dp, fp]),
        "scl_stream_from_store": (c_int, [P, c_int, c_int, c_int, ip, ip, dp, fp]),
        "scl_host_alloc": (c_int, [P, ctypes.c_size_t, POINTER(c_void_p)]),
        "scl_host_free": (c_int, [P, c_void_p]),
        "scl_host_register": (c_int, [P, c_void_p, ctypes.c_size_t]),
        "scl_host_unregister": (c_int, [P, c_void_p]),
        "scl_selftest_atanf_blocks": (c_int, [P, c_int, c_int, POINTER(ctypes.c_uint64)]),
        "scl_host_copy_rate": (c_int, [P, ctypes.c_size_t, c_int, dp]),
        "scl_selftest_bin_paths": (c_int, [P, c_int, c_uint64, c_uint64, POINTER(ctypes.c_uint64), POINTER(ctypes.c_uint64)]),
        "scl_selftest_bin_margin": (c_int, [P, c_int, c_uint64, c_uint64, POINTER(ctypes.c_uint64), POINTER(ctypes.c_uint64),
                                            POINTER(c_double), POINTER(c_double)]),
        "scl_selftest_sort_pairs": (c_int, [P, c_int, c_void_p, POINTER(ctypes.c_uint32), c_int, c_int, POINTER(c_int), c_int, c_void_p, POINTER(ctypes.c_uint32)]),
        "scl_selftest_prefix_sum": (c_int, [P, POINTER(ctypes.c_int32), c_int, c_int, POINTER(ctypes.c_int32)]),
        "scl_selftest_submaps_batch": (c_int, [P, c_int, c_int, ip, ip, fp, c_float, P, c_int, ip]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _bound = True


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _ptr(a, ctype):
    return a.ctypes.data_as(POINTER(ctype))


def _cloud(points):
    """Accept (n,3|4|8) float32 arrays; returns (array, n, stride_bytes)."""
    a = np.ascontiguousarray(points, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] < 3:
        raise ValueError("point cloud must be (n, >=3) float32")
    return a, a.shape[0], a.shape[1] * 4


class RegistrationEval:
    """What registration_eval_batch and its store forms answer for m candidates: n_src (the source's size, after the filter in the
    store forms), n_valid[m], n_inliers[m], moments[m,10] (fp64 sums over the inliers of the matched target point's x, y, z, xx, yy,
    zz, xy, xz, yz and of the squared distance) and, from the store forms, n_tgts[m]."""

    def __init__(self, n_src, n_valid, n_inliers, moments, n_tgts=None):
        self.n_src, self.n_valid, self.n_inliers, self.moments, self.n_tgts = n_src, n_valid, n_inliers, moments, n_tgts

    def __len__(self):
        return len(self.n_inliers)

    @property
    def overlap(self):
        """n_inliers / n_src per candidate (0 for an empty source)"""
        return self.n_inliers / float(self.n_src) if self.n_src > 0 else np.zeros(len(self), np.float64)

    @property
    def rmse(self):
        """sqrt(sum d2 / n_inliers) per candidate, NaN where there is no inlier"""
        m = self.n_inliers.astype(np.float64)
        return np.sqrt(np.divide(self.moments[:, 9], m, out=np.full(len(self), np.nan), where=m > 0))

    def information(self, c):
        """the 6 x 6 information matrix of candidate c's pairs, rotation first (scl_registration_information)"""
        return ScanContextEngine.registration_information(int(self.n_inliers[c]), self.moments[c])


class RegistrationPlaneEval:
    """What registration_eval_plane_batch and its store forms answer for m candidates: n_src (after the filter in the store forms),
    n_valid[m], n_inliers[m], n_planar[m] (the inliers whose matched target point has a normal), sums[m,29] (the upper triangle of
    sum J^T J for J = [p x n | n], rotation first; sum J r for r = (q - p) . n; sum r r; the sum of the squared distances of ALL
    inliers) and, from the store forms, n_tgts[m]."""

    def __init__(self, n_src, n_valid, n_inliers, n_planar, sums, n_tgts=None):
        self.n_src, self.n_valid, self.n_inliers, self.n_planar, self.sums, self.n_tgts = n_src, n_valid, n_inliers, n_planar, sums, n_tgts

    def __len__(self):
        return len(self.n_inliers)

    def information(self, c):
        """the 6 x 6 point-to-plane information matrix sum J^T J of candidate c's pairs, rotation first"""
        return ScanContextEngine.registration_information_plane(self.sums[c])[0]

    def gradient(self, c):
        """sum J r of candidate c's pairs: the right-hand side of the point-to-plane normal equations at T_c"""
        return ScanContextEngine.registration_information_plane(self.sums[c])[1]

    def rmse_plane(self, c):
        """sqrt(sum r r / n_planar): the root mean square point-to-plane distance of candidate c, NaN without a planar inlier"""
        m = int(self.n_planar[c])
        return float(np.sqrt(self.sums[c, 27] / m)) if m > 0 else float("nan")


class PcmConsistency:
    """What pcm_consistency answers for n loops: d2[n,n] (the squared Mahalanobis distance of every pair's cycle, symmetric, zero
    diagonal, +inf where the covariance could not be factored), adj[n,n] (bool: d2 <= threshold), words[n,W] (the same graph as
    scl_pcm_consistency writes it: bit j of row i = word j // 64, bit j % 64) and degree[n]."""

    def __init__(self, d2, adj, words, degree):
        self.d2, self.adj, self.words, self.degree = d2, adj, words, degree

    def __len__(self):
        return len(self.degree)


def pcm_words_to_bool(words, n):
    """the n x n bool matrix of n rows of (n + 63) // 64 uint64 adjacency words"""
    w = np.ascontiguousarray(words, dtype="<u8").reshape(n, (n + 63) // 64 if n else 0)
    return np.unpackbits(w.view(np.uint8), axis=1, bitorder="little")[:, :n].astype(bool) if n else np.zeros((0, 0), bool)


def pcm_bool_to_words(adj):
    """n rows of (n + 63) // 64 uint64 adjacency words of an n x n bool matrix"""
    a = np.asarray(adj, dtype=bool)
    n = a.shape[0]
    W = (n + 63) // 64
    if n == 0:
        return np.zeros((0, 0), np.uint64)
    padded = np.zeros((n, W * 64), np.uint8)
    padded[:, :n] = a
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view("<u8").reshape(n, W)


class ScanContextEngine:
    """One engine = one keyframe database resident in one GPU's HBM, or -- with ``devices=[...]`` -- ONE database
    sharded over several GPUs behind the same interface (``scl_create_sharded``: keyframe g on shard g % len(devices);
    ``exchange`` 0 auto, 1 host merge, 2 RCCL min all-reduce of the full-DB winners)."""

    def __init__(self, num_ring=20, num_sector=60, num_candidates=3, dist_thres=0.14,
                 lidar_height=1.65, max_radius=80.0, num_exclude_recent=100,
                 tree_making_period=10, search_ratio=0.1, knn_exclude_eps=0.0,
                 device=0, initial_capacity=4096, devices=None, exchange=0):
        self._lib = load_library()
        _bind(self._lib)
        cfg = SclConfig()
        self._lib.scl_default_config(byref(cfg))
        cfg.num_ring, cfg.num_sector, cfg.num_candidates = num_ring, num_sector, num_candidates
        cfg.dist_thres, cfg.lidar_height, cfg.max_radius = dist_thres, lidar_height, max_radius
        cfg.num_exclude_recent, cfg.tree_making_period = num_exclude_recent, tree_making_period
        cfg.search_ratio, cfg.knn_exclude_eps = search_ratio, knn_exclude_eps
        cfg.device, cfg.initial_capacity = device, initial_capacity
        self.cfg = cfg
        self.R, self.S = num_ring, num_sector
        self._pinned = {}
        self._h = c_void_p()
        if devices is not None:
            devs = np.ascontiguousarray(devices, dtype=np.int32)
            rc = self._lib.scl_create_sharded(byref(cfg), _ptr(devs, c_int), devs.size, exchange, byref(self._h))
        else:
            rc = self._lib.scl_create(byref(cfg), byref(self._h))
        if rc != 0:
            self._h = c_void_p()
            raise SclError(rc, "scl_create", self._lib.scl_status_string(rc).decode())

    def shard_info(self):
        """(number of shards, exchange in use: 0 none, 1 host merge, 2 RCCL)"""
        n, x = c_int(), c_int()
        self._check(self._lib.scl_shard_info(self._h, byref(n), byref(x)), "scl_shard_info")
        return n.value, x.value

    # -- plumbing -----------------------------------------------------------
    def _check(self, rc, where):
        if rc != 0:
            raise SclError(rc, where, self._lib.scl_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.scl_destroy(self._h)
            self._h = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- the six virtuals -----------------------------------------------------
    def make_and_save(self, points, robot=0, index=0):
        a, n, stride = _cloud(points)
        out = np.empty(self.R * self.S, dtype=np.float32)
        self._check(self._lib.scl_make_and_save(self._h, a.ctypes.data_as(c_void_p), n, stride,
                                                robot, index, _ptr(out, c_float)), "scl_make_and_save")
        return out

    def make_and_save_filtered(self, points, leaf, robot=0, index=0):
        """makeDescriptors (DM.h:996-1002): voxel filter + descriptor + append, the filtered cloud stays on the device"""
        a, n, stride = _cloud(points)
        out = np.empty(self.R * self.S, dtype=np.float32); m = c_int()
        self._check(self._lib.scl_make_and_save_filtered(self._h, a.ctypes.data_as(c_void_p), n, stride, leaf,
                                                         robot, index, _ptr(out, c_float), byref(m)), "scl_make_and_save_filtered")
        return out, m.value

    def _cloud_list(self, clouds):
        arrs, ptrs, counts, stride = [], [], [], None
        for c in clouds:
            a, n, st = _cloud(c)
            if stride is None:
                stride = st
            elif st != stride:
                raise ValueError("the clouds of a batch share one point stride")
            arrs.append(a); ptrs.append(a.ctypes.data); counts.append(n)
        m = len(arrs)
        return arrs, (c_void_p * max(1, m))(*ptrs), np.asarray(counts, dtype=np.int32), m, (stride or 16)

    def make_and_save_many(self, clouds, robots=None, indexs=None, want_values=True):
        """scl_make_and_save_many: the clouds' descriptors appended in order; returns the wire-format values [count, R*S] (or None)"""
        arrs, ptrs, counts, m, stride = self._cloud_list(clouds)
        out = np.empty((m, self.R * self.S), dtype=np.float32) if want_values else None
        rb = None if robots is None else np.ascontiguousarray(robots, dtype=np.int8)
        ib = None if indexs is None else np.ascontiguousarray(indexs, dtype=np.int32)
        self._check(self._lib.scl_make_and_save_many(self._h, ptrs, _ptr(counts, c_int), m, stride,
                                                     None if rb is None else _ptr(rb, c_int8), None if ib is None else _ptr(ib, c_int),
                                                     None if out is None else _ptr(out, c_float)), "scl_make_and_save_many")
        return out

    def stream_from_points(self, clouds, robots=None, indexs=None, want_values=False):
        """scl_stream_from_points: per scan descriptor + append + full-database detection; returns (nn_idx, shift, dist[, values])"""
        arrs, ptrs, counts, m, stride = self._cloud_list(clouds)
        nn = np.empty(m, dtype=np.int32); sh = np.empty(m, dtype=np.int32); dd = np.empty(m, dtype=np.float64)
        out = np.empty((m, self.R * self.S), dtype=np.float32) if want_values else None
        rb = None if robots is None else np.ascontiguousarray(robots, dtype=np.int8)
        ib = None if indexs is None else np.ascontiguousarray(indexs, dtype=np.int32)
        self._check(self._lib.scl_stream_from_points(self._h, ptrs, _ptr(counts, c_int), m, stride,
                                                     None if rb is None else _ptr(rb, c_int8), None if ib is None else _ptr(ib, c_int),
                                                     _ptr(nn, c_int), _ptr(sh, c_int), _ptr(dd, c_double),
                                                     None if out is None else _ptr(out, c_float)), "scl_stream_from_points")
        return (nn, sh, dd, out) if want_values else (nn, sh, dd)

    def stream_from_store(self, robot, first_index, count, want_values=False):
        """scl_stream_from_store: descriptors from the stored keyframes' clouds + append + full-database detection"""
        nn = np.empty(count, dtype=np.int32); sh = np.empty(count, dtype=np.int32); dd = np.empty(count, dtype=np.float64)
        out = np.empty((count, self.R * self.S), dtype=np.float32) if want_values else None
        self._check(self._lib.scl_stream_from_store(self._h, robot, first_index, count, _ptr(nn, c_int), _ptr(sh, c_int), _ptr(dd, c_double),
                                                    None if out is None else _ptr(out, c_float)), "scl_stream_from_store")
        return (nn, sh, dd, out) if want_values else (nn, sh, dd)

    def host_alloc(self, shape, dtype=np.float32):
        """a numpy array over pinned host memory (scl_host_alloc): clouds handed over from it travel by DMA.  Freed with the engine
        (or host_free(array)); the array must not be used after that."""
        shape = tuple(int(x) for x in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = c_void_p()
        self._check(self._lib.scl_host_alloc(self._h, max(1, nbytes), byref(p)), "scl_host_alloc")
        buf = (ctypes.c_char * max(1, nbytes)).from_address(p.value)
        a = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
        self._pinned[a.ctypes.data] = p.value
        return a

    def host_free(self, array):
        p = self._pinned.pop(array.ctypes.data, None)
        if p is not None:
            self._check(self._lib.scl_host_free(self._h, c_void_p(p)), "scl_host_free")

    def host_copy_rate(self, nbytes=64 << 20, reps=8):
        g = c_double()
        self._check(self._lib.scl_host_copy_rate(self._h, nbytes, reps, byref(g)), "scl_host_copy_rate")
        return g.value

    def selftest_bin_paths(self, mode, seed, n_points):
        bad, sure = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self._lib.scl_selftest_bin_paths(self._h, mode, seed, n_points, byref(bad), byref(sure)), "scl_selftest_bin_paths")
        return bad.value, sure.value

    def selftest_bin_margin(self, mode, seed, n_points):
        """(disagreements, sure, largest ring deviation, largest sector deviation) of the fast binning's quotients from the chain's
        over the sure points; mode 0 uniform, 1 / 2 at the edges of the ring / sector guard bands"""
        bad, sure, dr, ds = ctypes.c_uint64(), ctypes.c_uint64(), c_double(), c_double()
        self._check(self._lib.scl_selftest_bin_margin(self._h, mode, seed, n_points, byref(bad), byref(sure), byref(dr), byref(ds)),
                    "scl_selftest_bin_margin")
        return bad.value, sure.value, dr.value, ds.value

    def selftest_sort_pairs(self, keys, values, bits, segment_offsets=None):
        """(keys, values) stably sorted on the key bits [0, bits) by csrc/device_sort.hip; keys uint32 or uint64"""
        keys = np.ascontiguousarray(keys); values = np.ascontiguousarray(values, dtype=np.uint32)
        assert keys.dtype in (np.uint32, np.uint64) and keys.shape == values.shape
        ko, vo = np.empty_like(keys), np.empty_like(values)
        seg = None if segment_offsets is None else np.ascontiguousarray(segment_offsets, dtype=np.int32)
        self._check(self._lib.scl_selftest_sort_pairs(self._h, keys.dtype.itemsize, c_void_p(keys.ctypes.data), _ptr(values, ctypes.c_uint32), keys.size, bits,
                                                      None if seg is None else _ptr(seg, c_int), 0 if seg is None else seg.size - 1,
                                                      c_void_p(ko.ctypes.data), _ptr(vo, ctypes.c_uint32)), "scl_selftest_sort_pairs")
        return ko, vo

    def selftest_prefix_sum(self, values, inclusive=False):
        v = np.ascontiguousarray(values, dtype=np.int32); out = np.empty_like(v)
        self._check(self._lib.scl_selftest_prefix_sum(self._h, _ptr(v, ctypes.c_int32), v.size, 1 if inclusive else 0, _ptr(out, ctypes.c_int32)), "scl_selftest_prefix_sum")
        return out

    def selftest_submaps_batch(self, robot, keys, search_nums, poses, leaf, floats_per_point=8):
        """the submaps of voxel.hip's batched filter, one array per job: job j = the window of keys[j] with search_nums[j] of the
        keyframe store, poses[j] its 2 * search_nums[j] + 1 matrices (as submap_from_store takes them)"""
        keys = np.ascontiguousarray(keys, dtype=np.int32); sns = np.ascontiguousarray(search_nums, dtype=np.int32)
        m = keys.size
        assert sns.size == m and len(poses) == m
        Ts = [_f32(np.asarray(p)).reshape(-1, 16) for p in poses]
        assert all(T.shape[0] == 2 * int(sn) + 1 for T, sn in zip(Ts, sns))
        Tp = np.concatenate(Ts) if m else np.zeros((1, 16), np.float32)
        stored, cap, n = self.keyframe_count(robot), 0, c_int()
        for k, sn in zip(keys, sns):                                   # room for every window unfiltered
            for i in range(max(0, int(k) - int(sn)), min(stored, int(k) + int(sn) + 1)):
                self._check(self._lib.scl_keyframe_get(self._h, robot, i, None, 0, byref(n)), "scl_keyframe_get")
                cap += n.value
        out = np.empty((max(cap, 1), floats_per_point), dtype=np.float32); n_out = np.zeros(max(m, 1), dtype=np.int32)
        self._check(self._lib.scl_selftest_submaps_batch(self._h, robot, m, _ptr(keys, c_int), _ptr(sns, c_int), _ptr(Tp, c_float), leaf,
                                                         out.ctypes.data_as(c_void_p), cap, _ptr(n_out, c_int)), "scl_selftest_submaps_batch")
        ends = np.cumsum(n_out[:m])
        return [out[e - c:e].copy() for e, c in zip(ends, n_out[:m])]

    def selftest_atanf_blocks(self, first_block, n_blocks):
        out = np.zeros(n_blocks, dtype=np.uint64)
        self._check(self._lib.scl_selftest_atanf_blocks(self._h, first_block, n_blocks, out.ctypes.data_as(POINTER(ctypes.c_uint64))),
                    "scl_selftest_atanf_blocks")
        return out

    def save_from_wire(self, values, robot=0, index=0):
        v = _f32(values).reshape(-1)
        if v.size != self.R * self.S:
            raise ValueError("values must hold R*S floats")
        self._check(self._lib.scl_save_from_wire(self._h, _ptr(v, c_float), robot, index), "scl_save_from_wire")

    def detect_intra(self, cur):
        lid, sh, d = c_int(), c_float(), c_double()
        self._check(self._lib.scl_detect_intra(self._h, cur, byref(lid), byref(sh), byref(d)), "scl_detect_intra")
        return lid.value, sh.value, d.value

    def detect_inter(self, cur):
        lid, yaw, d = c_int(), c_float(), c_double()
        self._check(self._lib.scl_detect_inter(self._h, cur, byref(lid), byref(yaw), byref(d)), "scl_detect_inter")
        return lid.value, yaw.value, d.value

    def get_index(self, key):
        r, i = c_int8(), c_int()
        self._check(self._lib.scl_get_index(self._h, key, byref(r), byref(i)), "scl_get_index")
        return r.value, i.value

    def get_size(self, id_in=-1):
        n = self._lib.scl_get_size(self._h, id_in)
        if n < 0:
            raise SclError(n, "scl_get_size")
        return n

    # -- building blocks -------------------------------------------------------
    def make_descriptor(self, points):
        a, n, stride = _cloud(points)
        out = np.empty(self.R * self.S, dtype=np.float32)
        self._check(self._lib.scl_make_descriptor(self._h, a.ctypes.data_as(c_void_p), n, stride,
                                                  _ptr(out, c_float)), "scl_make_descriptor")
        return out

    def save_bulk(self, values, robots=None, indexs=None):
        v = _f32(values).reshape(-1, self.R * self.S)
        count = v.shape[0]
        rp = ip = None
        if robots is not None:
            robots = np.ascontiguousarray(robots, dtype=np.int8); rp = _ptr(robots, c_int8)
        if indexs is not None:
            indexs = np.ascontiguousarray(indexs, dtype=np.int32); ip = _ptr(indexs, c_int)
        self._check(self._lib.scl_save_bulk(self._h, _ptr(v, c_float), count, rp, ip), "scl_save_bulk")

    def get_descriptor(self, key):
        out = np.empty(self.R * self.S, dtype=np.float32)
        self._check(self._lib.scl_get_descriptor(self._h, key, _ptr(out, c_float)), "scl_get_descriptor")
        return out.reshape(self.R, self.S)

    def get_ringkey(self, key):
        out = np.empty(self.R, dtype=np.float32)
        self._check(self._lib.scl_get_ringkey(self._h, key, _ptr(out, c_float)), "scl_get_ringkey")
        return out

    def get_sectorkey(self, key):
        out = np.empty(self.S, dtype=np.float64)
        self._check(self._lib.scl_get_sectorkey(self._h, key, _ptr(out, c_double)), "scl_get_sectorkey")
        return out

    def get_descriptors(self, first, count):
        out = np.empty((max(count, 1), self.R * self.S), dtype=np.float32)
        self._check(self._lib.scl_get_descriptors(self._h, first, count, _ptr(out, c_float)), "scl_get_descriptors")
        return out[:count].reshape(count, self.R, self.S)

    def find_key(self, robot, index):
        """reverse of get_index: database key of (robot, index) or -1 (DM.h:1281-1284)"""
        k = c_int()
        self._check(self._lib.scl_find_key(self._h, robot, index, byref(k)), "scl_find_key")
        return k.value

    def db_dump(self, path):
        self._check(self._lib.scl_db_dump_file(self._h, os.fsencode(path)), "scl_db_dump_file")

    def db_load(self, path):
        n = c_int()
        self._check(self._lib.scl_db_load_file(self._h, os.fsencode(path), byref(n)), "scl_db_load_file")
        return n.value

    def matrix_to_pose(self, T):
        Tm = _f32(T).reshape(16)
        v = [c_float() for _ in range(6)]
        self._check(self._lib.scl_matrix_to_pose(_ptr(Tm, c_float), *[byref(x) for x in v]), "scl_matrix_to_pose")
        return tuple(x.value for x in v)

    def loop_pose_between(self, T_icp, pose_cur, pose_pre):
        """DM.h:1130-1141: (translation xyz + quaternion xyzw, roll/pitch/yaw) of poseFrom.between(poseTo)"""
        Tm = _f32(T_icp).reshape(16); pc = _f32(pose_cur).reshape(6); pp = _f32(pose_pre).reshape(6)
        out = np.empty(7, np.float64); rpy = np.empty(3, np.float64)
        self._check(self._lib.scl_loop_pose_between(_ptr(Tm, c_float), _ptr(pc, c_float), _ptr(pp, c_float), _ptr(out, c_double), _ptr(rpy, c_double)),
                    "scl_loop_pose_between")
        return out, rpy

    def stage_query(self, values):
        v = _f32(values).reshape(-1)
        if v.size != self.R * self.S:
            raise ValueError("values must hold R*S floats")
        self._check(self._lib.scl_stage_query(self._h, _ptr(v, c_float)), "scl_stage_query")

    def ringkey_topk(self, query, lo, hi, k):
        idx = np.empty(k, dtype=np.int32); d2 = np.empty(k, dtype=np.float32); found = c_int()
        self._check(self._lib.scl_ringkey_topk(self._h, query, lo, hi, k, _ptr(idx, c_int), _ptr(d2, c_float),
                                               byref(found)), "scl_ringkey_topk")
        return idx, d2, found.value

    def sc_distance_batch(self, query, cand=None, n=None):
        if cand is not None:
            cand = np.ascontiguousarray(cand, dtype=np.int32); n = cand.size; cp = _ptr(cand, c_int)
        else:
            cp = None
            if n is None:
                raise ValueError("give cand or n")
        dist = np.empty(n, dtype=np.float64); shift = np.empty(n, dtype=np.int32)
        self._check(self._lib.scl_sc_distance_batch(self._h, query, cp, n, _ptr(dist, c_double),
                                                    _ptr(shift, c_int)), "scl_sc_distance_batch")
        return dist, shift

    def sc_distance_matrix(self, queries, lo, hi):
        """exact fp64 distance and shift of every (queries[r], keyframe lo..hi-1) pair: two arrays of shape (len(queries), hi - lo)"""
        q = np.ascontiguousarray(queries, dtype=np.int32)
        n = max(0, int(hi) - int(lo))
        dist = np.empty((q.size, n), dtype=np.float64); shift = np.empty((q.size, n), dtype=np.int32)
        self._check(self._lib.scl_sc_distance_matrix(self._h, _ptr(q, c_int), q.size, int(lo), int(hi), _ptr(dist, c_double), _ptr(shift, c_int)),
                    "scl_sc_distance_matrix")
        return dist, shift

    @staticmethod
    def _search_out(n, k, out):
        if out is not None:
            return out
        return (np.empty((n, k), dtype=np.int32), np.empty((n, k), dtype=np.int32), np.empty((n, k), dtype=np.float64),
                np.empty(n, dtype=np.int32))

    def sc_search_range(self, queries, lo, hi, k, out=None):
        """the ranked search (scl_engine.h, THE RANKED SEARCH): query i = keyframe queries[i] (or a staged query, -1 - slot) against the
        keyframes lo[i] .. hi[i]-1, the k best by SC distance: (ids int32 [n,k], shifts int32 [n,k], dists float64 [n,k], n_found
        int32 [n]); entries behind n_found are (-1, 0, 1e7).  lo / hi: one value for all queries or one per query.  out: four
        C-contiguous arrays of those shapes to write into instead of new ones (an error leaves them as they are)."""
        q = np.ascontiguousarray(queries, dtype=np.int32).reshape(-1)
        n = q.size
        lo_ = np.ascontiguousarray(np.broadcast_to(np.asarray(lo, dtype=np.int32), (n,)))
        hi_ = np.ascontiguousarray(np.broadcast_to(np.asarray(hi, dtype=np.int32), (n,)))
        ids, shifts, dists, found = self._search_out(n, max(int(k), 0), out)
        self._check(self._lib.scl_sc_search_range(self._h, _ptr(q, c_int), _ptr(lo_, c_int), _ptr(hi_, c_int), n, int(k), _ptr(ids, c_int),
                                                  _ptr(shifts, c_int), _ptr(dists, c_double), _ptr(found, c_int)), "scl_sc_search_range")
        return ids, shifts, dists, found

    def sc_search(self, curs, k, out=None):
        """... over the search set of detect_full: query i = keyframe curs[i] against [0, curs[i] - num_exclude_recent)"""
        q = np.ascontiguousarray(curs, dtype=np.int32).reshape(-1)
        ids, shifts, dists, found = self._search_out(q.size, max(int(k), 0), out)
        self._check(self._lib.scl_sc_search(self._h, _ptr(q, c_int), q.size, int(k), _ptr(ids, c_int), _ptr(shifts, c_int),
                                            _ptr(dists, c_double), _ptr(found, c_int)), "scl_sc_search")
        return ids, shifts, dists, found

    def sc_search_intra(self, curs, k, out=None):
        """... over this robot's older keyframes, by VALUE (scl_engine.h, THE RANKED SEARCH PER ROBOT): with (r, x) = get_index(curs[i]),
        every keyframe of robot r whose index is < x - num_exclude_recent, wherever it sits in the database"""
        q = np.ascontiguousarray(curs, dtype=np.int32).reshape(-1)
        ids, shifts, dists, found = self._search_out(q.size, max(int(k), 0), out)
        self._check(self._lib.scl_sc_search_intra(self._h, _ptr(q, c_int), q.size, int(k), _ptr(ids, c_int), _ptr(shifts, c_int),
                                                  _ptr(dists, c_double), _ptr(found, c_int)), "scl_sc_search_intra")
        return ids, shifts, dists, found

    def sc_search_inter(self, curs, k, robot_pre=-1, out=None):
        """... over the other robots' keyframes: robot_pre = -1 (SCL_SC_ANY_OTHER_ROBOT): every keyframe of a robot other than
        curs[i]'s; robot_pre in 0 .. 127: the keyframes of that robot (which must not be the robot of a query) -- the list for
        geometric_verification_batch_from_store*(robot=robot_pre) once get_index has turned the ids into that robot's keys"""
        q = np.ascontiguousarray(curs, dtype=np.int32).reshape(-1)
        ids, shifts, dists, found = self._search_out(q.size, max(int(k), 0), out)
        self._check(self._lib.scl_sc_search_inter(self._h, _ptr(q, c_int), q.size, int(robot_pre), int(k), _ptr(ids, c_int), _ptr(shifts, c_int),
                                                  _ptr(dists, c_double), _ptr(found, c_int)), "scl_sc_search_inter")
        return ids, shifts, dists, found

    def detect_full(self, cur):
        lid, nn, sh, d = c_int(), c_int(), c_int(), c_double()
        self._check(self._lib.scl_detect_full(self._h, cur, byref(lid), byref(nn), byref(sh), byref(d)),
                    "scl_detect_full")
        return lid.value, nn.value, sh.value, d.value

    def detect_full_range(self, query, lo, hi):
        nn, sh, d = c_int(), c_int(), c_double()
        self._check(self._lib.scl_detect_full_range(self._h, query, lo, hi, byref(nn), byref(sh), byref(d)),
                    "scl_detect_full_range")
        return nn.value, sh.value, d.value

    def detect_full_submit(self, query, lo, hi):
        t = c_int()
        self._check(self._lib.scl_detect_full_submit(self._h, query, lo, hi, byref(t)), "scl_detect_full_submit")
        return t.value

    def detect_full_submit_many(self, queries, lo, hi):
        """several database keyframes as queries, up to four per launch; returns one ticket per query"""
        q = np.ascontiguousarray(queries, dtype=np.int32)
        m = q.shape[0]
        lo_ = np.ascontiguousarray(np.broadcast_to(np.asarray(lo, dtype=np.int32), (m,)))
        hi_ = np.ascontiguousarray(np.broadcast_to(np.asarray(hi, dtype=np.int32), (m,)))
        t = np.zeros(m, dtype=np.int32)
        self._check(self._lib.scl_detect_full_submit_many(self._h, _ptr(q, c_int), _ptr(lo_, c_int), _ptr(hi_, c_int), m, _ptr(t, c_int)),
                    "scl_detect_full_submit_many")
        return [int(x) for x in t]

    def detect_full_stream(self, queries, lo, hi, scans_per_launch=2, launches_in_flight=2):
        """a backlog of scans through the native submit / collect pipeline; returns (nn_idx, shift, dist) arrays"""
        q = np.ascontiguousarray(queries, dtype=np.int32)
        m = q.shape[0]
        lo_ = np.ascontiguousarray(np.broadcast_to(np.asarray(lo, dtype=np.int32), (m,)))
        hi_ = np.ascontiguousarray(np.broadcast_to(np.asarray(hi, dtype=np.int32), (m,)))
        nn = np.empty(max(m, 1), np.int32); sh = np.empty(max(m, 1), np.int32); d = np.empty(max(m, 1), np.float64)
        self._check(self._lib.scl_detect_full_stream(self._h, _ptr(q, c_int), _ptr(lo_, c_int), _ptr(hi_, c_int), m,
                                                     scans_per_launch, launches_in_flight, _ptr(nn, c_int), _ptr(sh, c_int),
                                                     _ptr(d, c_double)), "scl_detect_full_stream")
        return nn[:m], sh[:m], d[:m]

    def detect_full_collect(self, ticket):
        nn, sh, d = c_int(), c_int(), c_double()
        self._check(self._lib.scl_detect_full_collect(self._h, ticket, byref(nn), byref(sh), byref(d)),
                    "scl_detect_full_collect")
        return nn.value, sh.value, d.value

    def screen_distances_many(self, queries, lo, hi):
        """diagnostic: the screening pass of up to 16 scans in one launch over slots lo..hi-1 -> (approx [nq, n], eps)"""
        q = np.ascontiguousarray(queries, dtype=np.int32)
        n = max(0, min(hi, self.get_size()) - max(lo, 0))
        approx = np.empty((q.shape[0], max(n, 1)), np.float32); eps = c_float()
        self._check(self._lib.scl_screen_distances_many(self._h, _ptr(q, c_int), q.shape[0], lo, hi, _ptr(approx, c_float), byref(eps)),
                    "scl_screen_distances_many")
        return approx.reshape(-1)[:q.shape[0] * n].reshape(q.shape[0], n), eps.value

    def screen_distances(self, query, lo, hi):
        """diagnostic: (approximate distances of slots lo..hi-1, surviving slots, eps) of the screening pass"""
        n = max(0, min(hi, self.get_size()) - max(lo, 0))
        approx = np.empty(max(n, 1), np.float32); surv = np.empty(max(n, 1), np.int32); ns = c_int(); eps = c_float()
        self._check(self._lib.scl_screen_distances(self._h, query, lo, hi, _ptr(approx, c_float), _ptr(surv, c_int), byref(ns), byref(eps)),
                    "scl_screen_distances")
        return approx[:n], surv[:ns.value].copy(), eps.value

    def last_topk(self, k):
        idx = np.empty(k, dtype=np.int32); d2 = np.empty(k, dtype=np.float32)
        self._check(self._lib.scl_get_last_topk(self._h, k, _ptr(idx, c_int), _ptr(d2, c_float)), "scl_get_last_topk")
        return idx, d2

    def topk_with_distance(self, query, lo, hi, k):
        idx = np.empty(k, dtype=np.int32); d2 = np.empty(k, dtype=np.float32)
        dist = np.empty(k, dtype=np.float64); shift = np.empty(k, dtype=np.int32); found = c_int()
        self._check(self._lib.scl_topk_with_distance(self._h, query, lo, hi, k, _ptr(idx, c_int), _ptr(d2, c_float),
                                                     _ptr(dist, c_double), _ptr(shift, c_int), byref(found)),
                    "scl_topk_with_distance")
        return idx, d2, dist, shift, found.value

    # -- geometric verification ---------------------------------------------------
    def icp_default_params(self):
        p = IcpParams()
        self._lib.scl_icp_default_params(byref(p))
        return p

    def icp_align(self, src, tgt, params=None):
        s, ns, stride = _cloud(src)
        t, nt, stride_t = _cloud(tgt)
        if stride != stride_t:
            raise ValueError("source and target must share a record layout")
        p = params or self.icp_default_params()
        T = np.empty(16, dtype=np.float32); fit = c_float(); conv = c_int(); it = c_int()
        self._check(self._lib.scl_icp_align(self._h, s.ctypes.data_as(c_void_p), ns, t.ctypes.data_as(c_void_p), nt,
                                            stride, byref(p), _ptr(T, c_float), byref(fit), byref(conv), byref(it)),
                    "scl_icp_align")
        return T.reshape(4, 4), fit.value, bool(conv.value), it.value

    def icp_align_batch(self, src, tgts, params=None):
        """one source against several targets (the loop candidates of one scan), alignments overlapped on the device"""
        s_, ns, stride = _cloud(src)
        arrs = [_cloud(t) for t in tgts]
        for a, n, st in arrs:
            if st != stride:
                raise ValueError("source and targets must share a record layout")
        m = len(arrs)
        p = params or self.icp_default_params()
        ptrs = (c_void_p * max(1, m))(*[a.ctypes.data_as(c_void_p) for a, _, _ in arrs])
        counts = np.array([n for _, n, _ in arrs] or [0], dtype=np.int32)
        T = np.empty((max(1, m), 16), dtype=np.float32); fit = np.zeros(max(1, m), np.float32)
        conv = np.zeros(max(1, m), np.int32); it = np.zeros(max(1, m), np.int32)
        self._check(self._lib.scl_icp_align_batch(self._h, s_.ctypes.data_as(c_void_p), ns, ptrs, _ptr(counts, c_int), m, stride,
                                                  byref(p), _ptr(T, c_float), _ptr(fit, c_float), _ptr(conv, c_int), _ptr(it, c_int)),
                    "scl_icp_align_batch")
        return T[:m].reshape(m, 4, 4), fit[:m], conv[:m].astype(bool), it[:m]

    def nn_correspondences(self, src, tgt):
        s, ns, stride = _cloud(src)
        t, nt, stride_t = _cloud(tgt)
        if stride != stride_t:
            raise ValueError("source and target must share a record layout")
        idx = np.empty(ns, dtype=np.int32); d2 = np.empty(ns, dtype=np.float32)
        self._check(self._lib.scl_nn_correspondences(self._h, s.ctypes.data_as(c_void_p), ns,
                                                     t.ctypes.data_as(c_void_p), nt, stride,
                                                     _ptr(idx, c_int), _ptr(d2, c_float)), "scl_nn_correspondences")
        return idx, d2

    def nn_correspondences_moved(self, src, tgt, T):
        """Correspondences of `src` moved by the 4x4 `T`, searched warm from those of the unmoved cloud."""
        s, ns, stride = _cloud(src)
        t, nt, stride_t = _cloud(tgt)
        if stride != stride_t:
            raise ValueError("source and target must share a record layout")
        Tm = np.ascontiguousarray(T, dtype=np.float32).reshape(16)
        idx = np.empty(ns, dtype=np.int32); d2 = np.empty(ns, dtype=np.float32)
        self._check(self._lib.scl_nn_correspondences_moved(self._h, s.ctypes.data_as(c_void_p), ns,
                                                           t.ctypes.data_as(c_void_p), nt, stride, _ptr(Tm, c_float),
                                                           _ptr(idx, c_int), _ptr(d2, c_float)), "scl_nn_correspondences_moved")
        return idx, d2

    def rigid_svd(self, src, tgt, src_index, tgt_index):
        s, ns, stride = _cloud(src)
        t, nt, stride_t = _cloud(tgt)
        if stride != stride_t:
            raise ValueError("source and target must share a record layout")
        si = np.ascontiguousarray(src_index, dtype=np.int32); ti = np.ascontiguousarray(tgt_index, dtype=np.int32)
        T = np.empty(16, dtype=np.float32)
        self._check(self._lib.scl_rigid_svd(self._h, s.ctypes.data_as(c_void_p), ns, t.ctypes.data_as(c_void_p), nt,
                                            stride, _ptr(si, c_int), _ptr(ti, c_int), si.size, _ptr(T, c_float)),
                    "scl_rigid_svd")
        return T.reshape(4, 4)

    def ransac_correspondences(self, src, tgt, src_index, tgt_index, max_iterations=1000, inlier_threshold=0.25, seed=1):
        """CorrespondenceRejectorSampleConsensus (DM.h:1218-1225); defaults = ransacMaxIter / ransacOutlierTreshold (DM.h:187-188)"""
        s, ns, stride = _cloud(src)
        t, nt, stride_t = _cloud(tgt)
        if stride != stride_t:
            raise ValueError("source and target must share a record layout")
        si = np.ascontiguousarray(src_index, dtype=np.int32); ti = np.ascontiguousarray(tgt_index, dtype=np.int32)
        mask = np.empty(si.size, dtype=np.int32); ninl = c_int(); best = c_int(); T = np.empty(16, dtype=np.float32)
        self._check(self._lib.scl_ransac_correspondences(self._h, s.ctypes.data_as(c_void_p), ns, t.ctypes.data_as(c_void_p), nt,
                                                         stride, _ptr(si, c_int), _ptr(ti, c_int), si.size, max_iterations,
                                                         inlier_threshold, seed, _ptr(mask, c_int), byref(ninl), byref(best),
                                                         _ptr(T, c_float)), "scl_ransac_correspondences")
        return mask, ninl.value, best.value, T.reshape(4, 4)

    def geometric_verification(self, src, tgt, ransac_iterations=1000, inlier_threshold=0.25, inlier_ratio=0.45, seed=1):
        """compute core of geometricVerificationService (DM.h:1211-1243); defaults DM.h:187-189"""
        s, ns, stride = _cloud(src)
        t, nt, stride_t = _cloud(tgt)
        if stride != stride_t:
            raise ValueError("source and target must share a record layout")
        T = np.empty(16, dtype=np.float32); ok = c_int(); nc = c_int(); ni = c_int()
        self._check(self._lib.scl_geometric_verification(self._h, s.ctypes.data_as(c_void_p), ns, t.ctypes.data_as(c_void_p), nt,
                                                         stride, ransac_iterations, inlier_threshold, inlier_ratio, seed,
                                                         _ptr(T, c_float), byref(ok), byref(nc), byref(ni)),
                    "scl_geometric_verification")
        return T.reshape(4, 4), bool(ok.value), nc.value, ni.value

    def voxel_grid(self, cloud, leaf):
        """pcl::VoxelGrid with one leaf size (DM.h:501,503)"""
        a, n, stride = _cloud(cloud)
        out = np.empty_like(a); m = c_int()
        self._check(self._lib.scl_voxel_grid(self._h, a.ctypes.data_as(c_void_p), n, stride, leaf,
                                             out.ctypes.data_as(c_void_p), n, byref(m)), "scl_voxel_grid")
        return out[:m.value].copy()

    def pose_to_matrix(self, x, y, z, roll, pitch, yaw):
        T = np.empty(16, dtype=np.float32)
        self._check(self._lib.scl_pose_to_matrix(x, y, z, roll, pitch, yaw, _ptr(T, c_float)), "scl_pose_to_matrix")
        return T.reshape(4, 4)

    def assemble_submap(self, clouds, transforms, leaf):
        """loopFindNearKeyframes (DM.h:1163-1186): transformed keyframes concatenated, then voxel-filtered"""
        arrs = [np.ascontiguousarray(c, dtype=np.float32) for c in clouds]
        stride = arrs[0].shape[1] * 4 if arrs else 32
        counts = np.array([a.shape[0] for a in arrs], dtype=np.int32)
        ptrs = (c_void_p * max(1, len(arrs)))(*[a.ctypes.data_as(c_void_p) for a in arrs])
        Ts = _f32(np.stack(transforms)).reshape(-1, 16) if arrs else np.zeros((1, 16), np.float32)
        total = int(counts.sum())
        out = np.empty((max(total, 1), stride // 4), dtype=np.float32); m = c_int()
        self._check(self._lib.scl_assemble_submap(self._h, ptrs, _ptr(counts, c_int), _ptr(Ts, c_float), len(arrs), stride,
                                                  leaf, out.ctypes.data_as(c_void_p), total, byref(m)), "scl_assemble_submap")
        return out[:m.value].copy()

    def transform_cloud(self, cloud, T):
        a, n, stride = _cloud(cloud)
        out = np.empty_like(a)
        Tm = _f32(T).reshape(16)
        self._check(self._lib.scl_transform_cloud(self._h, a.ctypes.data_as(c_void_p), n, stride, _ptr(Tm, c_float),
                                                  out.ctypes.data_as(c_void_p)), "scl_transform_cloud")
        return out

    # -- on-device keyframe store (robots[id].keyFrameArray, DM.h:86) -------------
    def keyframe_put(self, robot, index, cloud):
        a, n, stride = _cloud(cloud)
        self._check(self._lib.scl_keyframe_put(self._h, robot, index, a.ctypes.data_as(c_void_p), n, stride), "scl_keyframe_put")

    def keyframe_count(self, robot):
        return self._lib.scl_keyframe_count(self._h, robot)

    def keyframe_get(self, robot, index, floats_per_point=8):
        n = c_int()
        self._check(self._lib.scl_keyframe_get(self._h, robot, index, None, 0, byref(n)), "scl_keyframe_get")
        out = np.empty((max(n.value, 1), floats_per_point), dtype=np.float32)
        self._check(self._lib.scl_keyframe_get(self._h, robot, index, out.ctypes.data_as(c_void_p), n.value, byref(n)), "scl_keyframe_get")
        return out[:n.value].copy()

    def submap_from_store(self, robot, key, search_num, poses, leaf, capacity, floats_per_point=8):
        """loopFindNearKeyframes (DM.h:1163-1186) on stored keyframes; poses[i] belongs to keyframe key-search_num+i"""
        Ts = _f32(np.asarray(poses)).reshape(-1, 16)
        assert Ts.shape[0] == 2 * search_num + 1
        out = np.empty((max(capacity, 1), floats_per_point), dtype=np.float32); m = c_int()
        self._check(self._lib.scl_submap_from_store(self._h, robot, key, search_num, _ptr(Ts, c_float), leaf,
                                                    out.ctypes.data_as(c_void_p), capacity, byref(m)), "scl_submap_from_store")
        return out[:m.value].copy()

    def loop_icp_from_store(self, robot, key_cur, pose_cur, key_pre, search_num, poses_pre, leaf, params=None,
                            min_src_points=300, min_tgt_points=1000):
        """performIntraLoopClosure stage 2 (DM.h:1104-1121) without moving clouds over PCIe"""
        p = params if params is not None else self.icp_default_params()
        Tc = _f32(np.asarray(pose_cur)).reshape(16)
        Tp = _f32(np.asarray(poses_pre)).reshape(-1, 16)
        assert Tp.shape[0] == 2 * search_num + 1
        T = np.empty(16, dtype=np.float32); fit = c_float(); conv = c_int(); it = c_int(); ns = c_int(); nt = c_int()
        self._check(self._lib.scl_loop_icp_from_store(self._h, robot, key_cur, _ptr(Tc, c_float), key_pre, search_num,
                                                      _ptr(Tp, c_float), leaf, byref(p), min_src_points, min_tgt_points,
                                                      _ptr(T, c_float), byref(fit), byref(conv), byref(it), byref(ns), byref(nt)),
                    "scl_loop_icp_from_store")
        return T.reshape(4, 4), fit.value, bool(conv.value), it.value, ns.value, nt.value

    def loop_icp_batch_from_store(self, robot, key_cur, pose_cur, keys_pre, search_num, poses_pre, leaf, params=None,
                                  min_src_points=300, min_tgt_points=1000):
        """stage 2 of performIntraLoopClosure for all loop candidates of one scan, ICP loops fused (BASELINE configs[2])"""
        p = params if params is not None else self.icp_default_params()
        keys = np.ascontiguousarray(keys_pre, dtype=np.int32); m = keys.size
        Tc = _f32(np.asarray(pose_cur)).reshape(16)
        Tp = _f32(np.asarray(poses_pre)).reshape(m, 2 * search_num + 1, 16)
        T = np.empty((max(m, 1), 16), np.float32); fit = np.zeros(max(m, 1), np.float32)
        conv = np.zeros(max(m, 1), np.int32); it = np.zeros(max(m, 1), np.int32); ns = c_int(); nt = np.zeros(max(m, 1), np.int32)
        self._check(self._lib.scl_loop_icp_batch_from_store(self._h, robot, key_cur, _ptr(Tc, c_float), m, _ptr(keys, c_int), search_num,
                                                            _ptr(Tp, c_float), leaf, byref(p), min_src_points, min_tgt_points,
                                                            _ptr(T, c_float), _ptr(fit, c_float), _ptr(conv, c_int), _ptr(it, c_int),
                                                            byref(ns), _ptr(nt, c_int)), "scl_loop_icp_batch_from_store")
        return T[:m].reshape(m, 4, 4), fit[:m], conv[:m].astype(bool), it[:m], ns.value, nt[:m]

    def geometric_verification_from_store(self, src, src_leaf, robot, key_pre, search_num, poses_pre, leaf,
                                          ransac_iterations=1000, inlier_threshold=0.25, inlier_ratio=0.45, seed=1,
                                          min_src_points=300, min_tgt_points=1000):
        """geometricVerificationService (DM.h:1189-1268) against a submap of stored keyframes"""
        a, n, stride = _cloud(src)
        Tp = _f32(np.asarray(poses_pre)).reshape(-1, 16)
        assert Tp.shape[0] == 2 * search_num + 1
        T = np.empty(16, dtype=np.float32); ok = c_int(); ns = c_int(); nt = c_int(); nc = c_int(); ni = c_int()
        self._check(self._lib.scl_geometric_verification_from_store(
            self._h, a.ctypes.data_as(c_void_p), n, stride, src_leaf, robot, key_pre, search_num, _ptr(Tp, c_float), leaf,
            min_src_points, min_tgt_points, ransac_iterations, inlier_threshold, inlier_ratio, seed,
            _ptr(T, c_float), byref(ok), byref(ns), byref(nt), byref(nc), byref(ni)), "scl_geometric_verification_from_store")
        return T.reshape(4, 4), bool(ok.value), ns.value, nt.value, nc.value, ni.value

    def geometric_verification_batch(self, src, tgts, ransac_iterations=1000, inlier_threshold=0.25, inlier_ratio=0.45, seed=1):
        """geometric_verification of one source against every cloud of `tgts`, every step one launch over all of them; returns
        (T[m,4,4], success[m], n_correspondences[m], n_inliers[m]), entry c equal to geometric_verification(src, tgts[c], ...)"""
        s, ns, stride = _cloud(src)
        arrs, ptrs, counts, m, stride_t = self._cloud_list(tgts)
        if m and stride != stride_t:
            raise ValueError("source and targets must share a record layout")
        k = max(m, 1)
        T = np.empty((k, 16), np.float32); ok = np.zeros(k, np.int32); nc = np.zeros(k, np.int32); ni = np.zeros(k, np.int32)
        self._check(self._lib.scl_geometric_verification_batch(self._h, s.ctypes.data_as(c_void_p), ns, ptrs, _ptr(counts, c_int), m, stride,
                                                               ransac_iterations, inlier_threshold, inlier_ratio, seed,
                                                               _ptr(T, c_float), _ptr(ok, c_int), _ptr(nc, c_int), _ptr(ni, c_int)),
                    "scl_geometric_verification_batch")
        return T[:m].reshape(m, 4, 4), ok[:m].astype(bool), nc[:m], ni[:m]

    def geometric_verification_batch_from_store(self, src, src_leaf, robot, keys_pre, search_num, poses_pre, leaf,
                                                ransac_iterations=1000, inlier_threshold=0.25, inlier_ratio=0.45, seed=1,
                                                min_src_points=300, min_tgt_points=1000):
        """geometricVerificationService (DM.h:1189-1268) for one received scan against the submaps of keys_pre (a peer's ranked
        list): returns (T[m,4,4], success[m], n_src_filtered, n_tgts[m], n_correspondences[m], n_inliers[m]), entry c equal to
        geometric_verification_from_store(src, src_leaf, robot, keys_pre[c], search_num, poses_pre[c], leaf, ...)"""
        a, n, stride = _cloud(src)
        keys = np.ascontiguousarray(keys_pre, dtype=np.int32); m = keys.size
        Tp = _f32(np.asarray(poses_pre)).reshape(m, 2 * search_num + 1, 16)
        k = max(m, 1)
        T = np.empty((k, 16), np.float32); ok = np.zeros(k, np.int32); ns = c_int(); nt = np.zeros(k, np.int32)
        nc = np.zeros(k, np.int32); ni = np.zeros(k, np.int32)
        self._check(self._lib.scl_geometric_verification_batch_from_store(
            self._h, a.ctypes.data_as(c_void_p), n, stride, src_leaf, robot, m, _ptr(keys, c_int), search_num, _ptr(Tp, c_float), leaf,
            min_src_points, min_tgt_points, ransac_iterations, inlier_threshold, inlier_ratio, seed,
            _ptr(T, c_float), _ptr(ok, c_int), byref(ns), _ptr(nt, c_int), _ptr(nc, c_int), _ptr(ni, c_int)),
            "scl_geometric_verification_batch_from_store")
        return T[:m].reshape(m, 4, 4), ok[:m].astype(bool), ns.value, nt[:m], nc[:m], ni[:m]

    def geometric_verification_batch_guess(self, src, tgts, guesses, ransac_iterations=1000, inlier_threshold=0.25, inlier_ratio=0.45, seed=1):
        """geometric_verification_batch with an initial guess per target (guesses[m,4,4]): entry c is answered for the source moved by
        guesses[c]; returns (T[m,4,4] = T_fit @ guess, success[m], n_correspondences[m], n_inliers[m], T_fit[m,4,4])"""
        s, ns, stride = _cloud(src)
        arrs, ptrs, counts, m, stride_t = self._cloud_list(tgts)
        if m and stride != stride_t:
            raise ValueError("source and targets must share a record layout")
        G = _f32(np.asarray(guesses)).reshape(m, 16)
        k = max(m, 1)
        T = np.empty((k, 16), np.float32); Tf = np.empty((k, 16), np.float32)
        ok = np.zeros(k, np.int32); nc = np.zeros(k, np.int32); ni = np.zeros(k, np.int32)
        self._check(self._lib.scl_geometric_verification_batch_guess(self._h, s.ctypes.data_as(c_void_p), ns, ptrs, _ptr(counts, c_int), m, stride,
                                                                     _ptr(G, c_float), ransac_iterations, inlier_threshold, inlier_ratio, seed,
                                                                     _ptr(T, c_float), _ptr(Tf, c_float), _ptr(ok, c_int), _ptr(nc, c_int), _ptr(ni, c_int)),
                    "scl_geometric_verification_batch_guess")
        return T[:m].reshape(m, 4, 4), ok[:m].astype(bool), nc[:m], ni[:m], Tf[:m].reshape(m, 4, 4)

    def geometric_verification_batch_from_store_guess(self, src, src_leaf, robot, keys_pre, search_num, poses_pre, leaf, guesses,
                                                      ransac_iterations=1000, inlier_threshold=0.25, inlier_ratio=0.45, seed=1,
                                                      min_src_points=300, min_tgt_points=1000):
        """geometric_verification_batch_from_store with an initial guess per candidate (guesses[m,4,4]), applied to the filtered received
        cloud: returns (T[m,4,4] = T_fit @ guess, success[m], n_src_filtered, n_tgts[m], n_correspondences[m], n_inliers[m], T_fit[m,4,4])"""
        a, n, stride = _cloud(src)
        keys = np.ascontiguousarray(keys_pre, dtype=np.int32); m = keys.size
        Tp = _f32(np.asarray(poses_pre)).reshape(m, 2 * search_num + 1, 16)
        G = _f32(np.asarray(guesses)).reshape(m, 16)
        k = max(m, 1)
        T = np.empty((k, 16), np.float32); Tf = np.empty((k, 16), np.float32); ok = np.zeros(k, np.int32); ns = c_int(); nt = np.zeros(k, np.int32)
        nc = np.zeros(k, np.int32); ni = np.zeros(k, np.int32)
        self._check(self._lib.scl_geometric_verification_batch_from_store_guess(
            self._h, a.ctypes.data_as(c_void_p), n, stride, src_leaf, robot, m, _ptr(keys, c_int), search_num, _ptr(Tp, c_float), leaf,
            _ptr(G, c_float), min_src_points, min_tgt_points, ransac_iterations, inlier_threshold, inlier_ratio, seed,
            _ptr(T, c_float), _ptr(Tf, c_float), _ptr(ok, c_int), byref(ns), _ptr(nt, c_int), _ptr(nc, c_int), _ptr(ni, c_int)),
            "scl_geometric_verification_batch_from_store_guess")
        return T[:m].reshape(m, 4, 4), ok[:m].astype(bool), ns.value, nt[:m], nc[:m], ni[:m], Tf[:m].reshape(m, 4, 4)

    def icp_align_batch_guess(self, src, tgts, guesses, params=None):
        """icp_align_batch with an initial guess per target (guesses[m,4,4]): entry c is icp_align(transform_cloud(src, guesses[c]),
        tgts[c]); returns (T[m,4,4] = T_icp @ guess, T_icp[m,4,4], fitness[m], converged[m], iterations[m])"""
        s_, ns, stride = _cloud(src)
        arrs, ptrs, counts, m, stride_t = self._cloud_list(tgts)
        if m and stride != stride_t:
            raise ValueError("source and targets must share a record layout")
        p = params if params is not None else self.icp_default_params()
        G = _f32(np.asarray(guesses)).reshape(m, 16)
        k = max(m, 1)
        T = np.empty((k, 16), np.float32); Ti = np.empty((k, 16), np.float32); fit = np.zeros(k, np.float32)
        conv = np.zeros(k, np.int32); it = np.zeros(k, np.int32)
        self._check(self._lib.scl_icp_align_batch_guess(self._h, s_.ctypes.data_as(c_void_p), ns, ptrs, _ptr(counts, c_int), m, stride,
                                                        _ptr(G, c_float), byref(p), _ptr(T, c_float), _ptr(Ti, c_float), _ptr(fit, c_float),
                                                        _ptr(conv, c_int), _ptr(it, c_int)), "scl_icp_align_batch_guess")
        return T[:m].reshape(m, 4, 4), Ti[:m].reshape(m, 4, 4), fit[:m], conv[:m].astype(bool), it[:m]

    def loop_icp_batch_from_store_guess(self, robot, key_cur, pose_cur, keys_pre, search_num, poses_pre, leaf, guesses, params=None,
                                        min_src_points=300, min_tgt_points=1000):
        """loop_icp_batch_from_store with an initial guess per candidate (guesses[m,4,4]; loop_guess_from_shift with both poses of the
        same robot), applied to submap(key_cur, 0): returns (T[m,4,4] = T_icp @ guess, T_icp[m,4,4], fitness[m], converged[m],
        iterations[m], n_src, n_tgts[m])"""
        p = params if params is not None else self.icp_default_params()
        keys = np.ascontiguousarray(keys_pre, dtype=np.int32); m = keys.size
        Tc = _f32(np.asarray(pose_cur)).reshape(16)
        Tp = _f32(np.asarray(poses_pre)).reshape(m, 2 * search_num + 1, 16)
        G = _f32(np.asarray(guesses)).reshape(m, 16)
        k = max(m, 1)
        T = np.empty((k, 16), np.float32); Ti = np.empty((k, 16), np.float32); fit = np.zeros(k, np.float32)
        conv = np.zeros(k, np.int32); it = np.zeros(k, np.int32); ns = c_int(); nt = np.zeros(k, np.int32)
        self._check(self._lib.scl_loop_icp_batch_from_store_guess(
            self._h, robot, key_cur, _ptr(Tc, c_float), m, _ptr(keys, c_int), search_num, _ptr(Tp, c_float), leaf, _ptr(G, c_float), byref(p),
            min_src_points, min_tgt_points, _ptr(T, c_float), _ptr(Ti, c_float), _ptr(fit, c_float), _ptr(conv, c_int), _ptr(it, c_int),
            byref(ns), _ptr(nt, c_int)), "scl_loop_icp_batch_from_store_guess")
        return T[:m].reshape(m, 4, 4), Ti[:m].reshape(m, 4, 4), fit[:m], conv[:m].astype(bool), it[:m], ns.value, nt[:m]

    def icp_align_batch_from_store_guess(self, src, src_leaf, robot, keys_pre, search_num, poses_pre, leaf, guesses, params=None,
                                         min_src_points=300, min_tgt_points=1000):
        """ICP of one RECEIVED scan (voxel-filtered once with src_leaf) against the submaps of keys_pre, from one initial guess per
        candidate (guesses[m,4,4]: the T of geometric_verification_batch_from_store_guess): returns (T[m,4,4] = T_icp @ guess,
        T_icp[m,4,4], fitness[m], converged[m], iterations[m], n_src_filtered, n_tgts[m])"""
        a, n, stride = _cloud(src)
        p = params if params is not None else self.icp_default_params()
        keys = np.ascontiguousarray(keys_pre, dtype=np.int32); m = keys.size
        Tp = _f32(np.asarray(poses_pre)).reshape(m, 2 * search_num + 1, 16)
        G = _f32(np.asarray(guesses)).reshape(m, 16)
        k = max(m, 1)
        T = np.empty((k, 16), np.float32); Ti = np.empty((k, 16), np.float32); fit = np.zeros(k, np.float32)
        conv = np.zeros(k, np.int32); it = np.zeros(k, np.int32); ns = c_int(); nt = np.zeros(k, np.int32)
        self._check(self._lib.scl_icp_align_batch_from_store_guess(
            self._h, a.ctypes.data_as(c_void_p), n, stride, src_leaf, robot, m, _ptr(keys, c_int), search_num, _ptr(Tp, c_float), leaf,
            _ptr(G, c_float), byref(p), min_src_points, min_tgt_points, _ptr(T, c_float), _ptr(Ti, c_float), _ptr(fit, c_float),
            _ptr(conv, c_int), _ptr(it, c_int), byref(ns), _ptr(nt, c_int)), "scl_icp_align_batch_from_store_guess")
        return T[:m].reshape(m, 4, 4), Ti[:m].reshape(m, 4, 4), fit[:m], conv[:m].astype(bool), it[:m], ns.value, nt[:m]

    def registration_eval_batch(self, src, tgts, transforms, max_dist):
        """the pairs of m finished registrations scored in one chain: candidate c's source is src moved by transforms[c] (m,4,4: the T
        of the guessed verification or of the guessed ICP); returns a RegistrationEval (overlap, rmse, information(c))"""
        s, ns, stride = _cloud(src)
        arrs, ptrs, counts, m, stride_t = self._cloud_list(tgts)
        if m and stride != stride_t:
            raise ValueError("source and targets must share a record layout")
        Tm = _f32(np.asarray(transforms)).reshape(m, 16)
        k = max(m, 1)
        nv = np.zeros(k, np.int32); ni = np.zeros(k, np.int32); mo = np.zeros((k, 10), np.float64)
        self._check(self._lib.scl_registration_eval_batch(self._h, s.ctypes.data_as(c_void_p), ns, ptrs, _ptr(counts, c_int), m, stride,
                                                          _ptr(Tm, c_float), max_dist, _ptr(nv, c_int), _ptr(ni, c_int), _ptr(mo, c_double)),
                    "scl_registration_eval_batch")
        return RegistrationEval(ns, nv[:m], ni[:m], mo[:m])

    def registration_eval_batch_from_store(self, src, src_leaf, robot, keys_pre, search_num, poses_pre, leaf, transforms, max_dist,
                                           min_src_points=300, min_tgt_points=1000):
        """registration_eval_batch for one RECEIVED scan (voxel-filtered once with src_leaf) against the submaps of keys_pre, with the
        layout and gates of geometric_verification_batch_from_store_guess; n_src is the filtered size"""
        a, n, stride = _cloud(src)
        keys = np.ascontiguousarray(keys_pre, dtype=np.int32); m = keys.size
        Tp = _f32(np.asarray(poses_pre)).reshape(m, 2 * search_num + 1, 16)
        Tm = _f32(np.asarray(transforms)).reshape(m, 16)
        k = max(m, 1)
        nv = np.zeros(k, np.int32); ni = np.zeros(k, np.int32); mo = np.zeros((k, 10), np.float64); ns = c_int(); nt = np.zeros(k, np.int32)
        self._check(self._lib.scl_registration_eval_batch_from_store(
            self._h, a.ctypes.data_as(c_void_p), n, stride, src_leaf, robot, m, _ptr(keys, c_int), search_num, _ptr(Tp, c_float), leaf,
            _ptr(Tm, c_float), min_src_points, min_tgt_points, max_dist, _ptr(nv, c_int), _ptr(ni, c_int), _ptr(mo, c_double),
            byref(ns), _ptr(nt, c_int)), "scl_registration_eval_batch_from_store")
        return RegistrationEval(ns.value, nv[:m], ni[:m], mo[:m], nt[:m])

    def loop_eval_batch_from_store(self, robot, key_cur, pose_cur, keys_pre, search_num, poses_pre, leaf, transforms, max_dist,
                                   min_src_points=300, min_tgt_points=1000):
        """registration_eval_batch on the intra-robot side: the source is submap(key_cur, 0), with the layout and gates of
        loop_icp_batch_from_store_guess, whose T is the intended transforms"""
        keys = np.ascontiguousarray(keys_pre, dtype=np.int32); m = keys.size
        Tc = _f32(np.asarray(pose_cur)).reshape(16)
        Tp = _f32(np.asarray(poses_pre)).reshape(m, 2 * search_num + 1, 16)
        Tm = _f32(np.asarray(transforms)).reshape(m, 16)
        k = max(m, 1)
        nv = np.zeros(k, np.int32); ni = np.zeros(k, np.int32); mo = np.zeros((k, 10), np.float64); ns = c_int(); nt = np.zeros(k, np.int32)
        self._check(self._lib.scl_loop_eval_batch_from_store(
            self._h, robot, key_cur, _ptr(Tc, c_float), m, _ptr(keys, c_int), search_num, _ptr(Tp, c_float), leaf, _ptr(Tm, c_float),
            min_src_points, min_tgt_points, max_dist, _ptr(nv, c_int), _ptr(ni, c_int), _ptr(mo, c_double), byref(ns), _ptr(nt, c_int)),
            "scl_loop_eval_batch_from_store")
        return RegistrationEval(ns.value, nv[:m], ni[:m], mo[:m], nt[:m])

    @staticmethod
    def registration_information(n_inliers, moments):
        """the 6 x 6 information matrix (rotation first) of a candidate's pairs from its inlier count and ten sums
        (scl_registration_information); needs no engine"""
        lib = load_library(); _bind(lib)
        mo = np.ascontiguousarray(moments, dtype=np.float64).reshape(10)
        info = np.empty(36, np.float64)
        rc = lib.scl_registration_information(int(n_inliers), _ptr(mo, c_double), _ptr(info, c_double))
        if rc != 0:
            raise SclError(rc, "scl_registration_information")
        return info.reshape(6, 6)

    def target_normals(self, tgt, radius):
        """the normals the point-to-plane estimator uses for this cloud and radius, (n,3) float32 ((0, 0, 0): fewer than three
        neighbours within the radius)"""
        a, n, stride = _cloud(tgt)
        out = np.zeros((max(n, 1), 3), np.float32)
        self._check(self._lib.scl_target_normals(self._h, a.ctypes.data_as(c_void_p), n, stride, radius, _ptr(out, c_float)), "scl_target_normals")
        return out[:n]

    def registration_eval_plane_batch(self, src, tgts, transforms, max_dist, normal_radius):
        """registration_eval_batch against the planes of the targets (normals at normal_radius); returns a RegistrationPlaneEval
        (information(c), gradient(c), rmse_plane(c))"""
        s, ns, stride = _cloud(src)
        arrs, ptrs, counts, m, stride_t = self._cloud_list(tgts)
        if m and stride != stride_t:
            raise ValueError("source and targets must share a record layout")
        Tm = _f32(np.asarray(transforms)).reshape(m, 16)
        k = max(m, 1)
        nv = np.zeros(k, np.int32); ni = np.zeros(k, np.int32); npl = np.zeros(k, np.int32); su = np.zeros((k, 29), np.float64)
        self._check(self._lib.scl_registration_eval_plane_batch(self._h, s.ctypes.data_as(c_void_p), ns, ptrs, _ptr(counts, c_int), m, stride,
                                                                _ptr(Tm, c_float), max_dist, normal_radius, _ptr(nv, c_int), _ptr(ni, c_int),
                                                                _ptr(npl, c_int), _ptr(su, c_double)),
                    "scl_registration_eval_plane_batch")
        return RegistrationPlaneEval(ns, nv[:m], ni[:m], npl[:m], su[:m])

    def registration_eval_plane_batch_from_store(self, src, src_leaf, robot, keys_pre, search_num, poses_pre, leaf, transforms, max_dist,
                                                 normal_radius, min_src_points=300, min_tgt_points=1000):
        """registration_eval_plane_batch with the layout and gates of registration_eval_batch_from_store"""
        a, n, stride = _cloud(src)
        keys = np.ascontiguousarray(keys_pre, dtype=np.int32); m = keys.size
        Tp = _f32(np.asarray(poses_pre)).reshape(m, 2 * search_num + 1, 16)
        Tm = _f32(np.asarray(transforms)).reshape(m, 16)
        k = max(m, 1)
        nv = np.zeros(k, np.int32); ni = np.zeros(k, np.int32); npl = np.zeros(k, np.int32); su = np.zeros((k, 29), np.float64)
        ns = c_int(); nt = np.zeros(k, np.int32)
        self._check(self._lib.scl_registration_eval_plane_batch_from_store(
            self._h, a.ctypes.data_as(c_void_p), n, stride, src_leaf, robot, m, _ptr(keys, c_int), search_num, _ptr(Tp, c_float), leaf,
            _ptr(Tm, c_float), min_src_points, min_tgt_points, max_dist, normal_radius, _ptr(nv, c_int), _ptr(ni, c_int), _ptr(npl, c_int),
            _ptr(su, c_double), byref(ns), _ptr(nt, c_int)), "scl_registration_eval_plane_batch_from_store")
        return RegistrationPlaneEval(ns.value, nv[:m], ni[:m], npl[:m], su[:m], nt[:m])

    def loop_eval_plane_batch_from_store(self, robot, key_cur, pose_cur, keys_pre, search_num, poses_pre, leaf, transforms, max_dist,
                                         normal_radius, min_src_points=300, min_tgt_points=1000):
        """registration_eval_plane_batch with the layout and gates of loop_eval_batch_from_store"""
        keys = np.ascontiguousarray(keys_pre, dtype=np.int32); m = keys.size
        Tc = _f32(np.asarray(pose_cur)).reshape(16)
        Tp = _f32(np.asarray(poses_pre)).reshape(m, 2 * search_num + 1, 16)
        Tm = _f32(np.asarray(transforms)).reshape(m, 16)
        k = max(m, 1)
        nv = np.zeros(k, np.int32); ni = np.zeros(k, np.int32); npl = np.zeros(k, np.int32); su = np.zeros((k, 29), np.float64)
        ns = c_int(); nt = np.zeros(k, np.int32)
        self._check(self._lib.scl_loop_eval_plane_batch_from_store(
            self._h, robot, key_cur, _ptr(Tc, c_float), m, _ptr(keys, c_int), search_num, _ptr(Tp, c_float), leaf, _ptr(Tm, c_float),
            min_src_points, min_tgt_points, max_dist, normal_radius, _ptr(nv, c_int), _ptr(ni, c_int), _ptr(npl, c_int), _ptr(su, c_double),
            byref(ns), _ptr(nt, c_int)), "scl_loop_eval_plane_batch_from_store")
        return RegistrationPlaneEval(ns.value, nv[:m], ni[:m], npl[:m], su[:m], nt[:m])

    @staticmethod
    def registration_information_plane(sums):
        """(info[6,6], grad[6]) of a candidate's 29 plane sums: the symmetric sum J^T J, rotation first, and sum J r
        (scl_registration_information_plane); needs no engine"""
        lib = load_library(); _bind(lib)
        su = np.ascontiguousarray(sums, dtype=np.float64).reshape(29)
        info = np.empty(36, np.float64); grad = np.empty(6, np.float64)
        rc = lib.scl_registration_information_plane(_ptr(su, c_double), _ptr(info, c_double), _ptr(grad, c_double))
        if rc != 0:
            raise SclError(rc, "scl_registration_information_plane")
        return info.reshape(6, 6), grad

    @staticmethod
    def loop_guess_from_shift(shift, num_sector, pose_cur, pose_pre):
        """the initial guess of an inter-robot verification from a Scan Context match (scl_loop_guess_from_shift): poses are
        (x, y, z, roll, pitch, yaw) of the received and of the candidate keyframe; needs no engine"""
        lib = load_library(); _bind(lib)
        pc = _f32(np.asarray(pose_cur)).reshape(6); pp = _f32(np.asarray(pose_pre)).reshape(6)
        G = np.empty(16, np.float32)
        rc = lib.scl_loop_guess_from_shift(int(shift), int(num_sector), _ptr(pc, c_float), _ptr(pp, c_float), _ptr(G, c_float))
        if rc != 0:
            raise SclError(rc, "scl_loop_guess_from_shift")
        return G.reshape(4, 4)

    # -- pairwise consistency of loop closures (scl_engine.h: PAIRWISE CONSISTENCY OF LOOP CLOSURES) ------------------
    @staticmethod
    def _pcm_inputs(poses_a, poses_b, idx_a, idx_b, z, cov, odom_var):
        pa = np.ascontiguousarray(poses_a, dtype=np.float64).reshape(-1, 7)
        pb = pa if poses_b is poses_a else np.ascontiguousarray(poses_b, dtype=np.float64).reshape(-1, 7)
        ia = np.ascontiguousarray(idx_a, dtype=np.int32).reshape(-1); ib = np.ascontiguousarray(idx_b, dtype=np.int32).reshape(-1)
        n = ia.size
        zz = np.ascontiguousarray(z, dtype=np.float64).reshape(n, 7); cc = np.ascontiguousarray(cov, dtype=np.float64).reshape(n, 36)
        if ib.size != n:
            raise ValueError("idx_a and idx_b must have one entry per loop")
        ov = None if odom_var is None else np.ascontiguousarray(odom_var, dtype=np.float64).reshape(6)
        keep = (pa, pb, ia, ib, zz, cc, ov)
        args = (_ptr(pa, c_double), pa.shape[0], _ptr(pb, c_double), pb.shape[0], _ptr(ia, c_int), _ptr(ib, c_int), _ptr(zz, c_double),
                _ptr(cc, c_double), n, None if ov is None else _ptr(ov, c_double))
        return keep, args, n

    def pcm_consistency(self, poses_a, poses_b, idx_a, idx_b, z, cov, threshold, odom_var=None, want_d2=True):
        """the consistency of every pair of the n loops (idx_a[i], idx_b[i], z[i], cov[i]) between trajectories poses_a and poses_b
        ((n,7): x, y, z, qx, qy, qz, qw; pass the same array twice for intra-robot loops): a PcmConsistency (d2 None with
        want_d2=False -- the n x n matrix then never leaves the device)"""
        keep, args, n = self._pcm_inputs(poses_a, poses_b, idx_a, idx_b, z, cov, odom_var)
        W = (n + 63) // 64
        d2 = np.zeros((max(n, 1), max(n, 1)), np.float64) if want_d2 else None
        words = np.zeros((max(n, 1), max(W, 1)), np.uint64); deg = np.zeros(max(n, 1), np.int32)
        self._check(self._lib.scl_pcm_consistency(self._h, *args, float(threshold), None if d2 is None else _ptr(d2, c_double),
                                                  _ptr(words, c_uint64), _ptr(deg, c_int)), "scl_pcm_consistency")
        words = words[:n, :W]
        return PcmConsistency(None if d2 is None else d2[:n, :n], pcm_words_to_bool(words, n), words, deg[:n])

    def pcm_max_clique(self, adj):
        """the greedy maximum clique of the contract on a graph from the host -- an n x n bool matrix, or n x W uint64 words --:
        (members ascending, seed); ((), -1) for an empty graph"""
        a = np.asarray(adj)
        words = np.ascontiguousarray(a, dtype=np.uint64) if a.dtype == np.uint64 else pcm_bool_to_words(a)
        n = words.shape[0]
        mem = np.zeros(max(n, 1), np.int32); m = c_int(-7); seed = c_int(-7)
        self._check(self._lib.scl_pcm_max_clique(self._h, _ptr(words, c_uint64), n, _ptr(mem, c_int), byref(m), byref(seed)), "scl_pcm_max_clique")
        return mem[:m.value].copy(), seed.value

    def pcm_select(self, poses_a, poses_b, idx_a, idx_b, z, cov, threshold, odom_var=None):
        """pcm_consistency and pcm_max_clique in one call on the device: (members ascending, seed, degree[n])"""
        keep, args, n = self._pcm_inputs(poses_a, poses_b, idx_a, idx_b, z, cov, odom_var)
        mem = np.zeros(max(n, 1), np.int32); deg = np.zeros(max(n, 1), np.int32); m = c_int(-7); seed = c_int(-7)
        self._check(self._lib.scl_pcm_select(self._h, *args, float(threshold), _ptr(mem, c_int), byref(m), byref(seed), _ptr(deg, c_int)),
                    "scl_pcm_select")
        return mem[:m.value].copy(), seed.value, deg[:n]

    def pcm_last_timing(self):
        """(pairs_ms, clique_ms): device time of the two stages of the last PCM call made under profile_enable(1)"""
        a, b = c_double(0.0), c_double(0.0)
        self._check(self._lib.scl_pcm_last_timing(self._h, byref(a), byref(b)), "scl_pcm_last_timing")
        return a.value, b.value

    @staticmethod
    def loop_covariance(info, s2):
        """cov = s2 * info^-1 (6 x 6, by Cholesky): the covariance of a loop from the information matrix of its pairs and the variance
        of a pair's residual (scl_loop_covariance); needs no engine.  A singular info is refused: regularise it first"""
        lib = load_library(); _bind(lib)
        a = np.ascontiguousarray(info, dtype=np.float64).reshape(36)
        cov = np.empty(36, np.float64)
        rc = lib.scl_loop_covariance(_ptr(a, c_double), float(s2), _ptr(cov, c_double))
        if rc != 0:
            raise SclError(rc, "scl_loop_covariance")
        return cov.reshape(6, 6)

    # -- pose-graph solve (scl_engine.h: POSE-GRAPH SOLVE) -------------------------------------------------------------
    @staticmethod
    def _pgo_inputs(poses, f_i, f_j, f_z, f_cov, p_idx, p_z, p_cov):
        x = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 7)
        fi = np.ascontiguousarray(f_i, dtype=np.int32).reshape(-1); fj = np.ascontiguousarray(f_j, dtype=np.int32).reshape(-1)
        pi = np.ascontiguousarray(p_idx, dtype=np.int32).reshape(-1)
        nf, npr = fi.size, pi.size
        if fj.size != nf:
            raise ValueError("f_i and f_j must have one entry per factor")
        fz = np.ascontiguousarray(f_z, dtype=np.float64).reshape(nf, 7); fc = np.ascontiguousarray(f_cov, dtype=np.float64).reshape(nf, 36)
        pz = np.ascontiguousarray(p_z, dtype=np.float64).reshape(npr, 7); pc = np.ascontiguousarray(p_cov, dtype=np.float64).reshape(npr, 36)
        keep = (x, fi, fj, fz, fc, pi, pz, pc)
        opt = lambda a, t: _ptr(a, t) if a.size else None
        args = (_ptr(x, c_double), x.shape[0], opt(fi, c_int), opt(fj, c_int), opt(fz, c_double), opt(fc, c_double), nf,
                opt(pi, c_int), opt(pz, c_double), opt(pc, c_double), npr)
        return keep, args, x.shape[0], nf + npr

    def pgo_linearize(self, poses, f_i, f_j, f_z, f_cov, p_idx, p_z, p_cov):
        """the pose graph linearised at `poses` ((n,7): x, y, z, qx, qy, qz, qw): (cost, gradient[n,6], diag[n,6,6], chi2[n_factors +
        n_priors]) for between factors (f_i, f_j, f_z[.,7], f_cov[.,6,6]) and priors (p_idx, p_z, p_cov)"""
        keep, args, n, m = self._pgo_inputs(poses, f_i, f_j, f_z, f_cov, p_idx, p_z, p_cov)
        cost = c_double(0.0); g = np.zeros((max(n, 1), 6)); d = np.zeros((max(n, 1), 6, 6)); chi2 = np.zeros(max(m, 1))
        self._check(self._lib.scl_pgo_linearize(self._h, *args, byref(cost), _ptr(g, c_double), _ptr(d, c_double), _ptr(chi2, c_double)),
                    "scl_pgo_linearize")
        return cost.value, g[:n], d[:n], chi2[:m]

    def pgo_hessian_apply(self, poses, f_i, f_j, f_z, f_cov, p_idx, p_z, p_cov, lam, x):
        """y[n,6] = (H + lam diag(H)) x for the Gauss-Newton matrix H of the graph at `poses`: the operator pgo_optimize iterates"""
        keep, args, n, m = self._pgo_inputs(poses, f_i, f_j, f_z, f_cov, p_idx, p_z, p_cov)
        xx = np.ascontiguousarray(x, dtype=np.float64).reshape(n, 6); y = np.zeros((max(n, 1), 6))
        self._check(self._lib.scl_pgo_hessian_apply(self._h, *args, float(lam), _ptr(xx, c_double), _ptr(y, c_double)), "scl_pgo_hessian_apply")
        return y[:n]

    def pgo_optimize(self, poses, f_i, f_j, f_z, f_cov, p_idx, p_z, p_cov, params=None, want_chi2=True):
        """Levenberg-Marquardt over the graph from `poses`: (poses_out[n,7] with unit quaternions and w >= 0, PgoResult, chi2 at poses_out
        or None); params: a PgoParams (None: the defaults)"""
        keep, args, n, m = self._pgo_inputs(poses, f_i, f_j, f_z, f_cov, p_idx, p_z, p_cov)
        out = np.zeros((max(n, 1), 7)); res = PgoResult(); chi2 = np.zeros(max(m, 1)) if want_chi2 else None
        self._check(self._lib.scl_pgo_optimize(self._h, *args, None if params is None else byref(params), _ptr(out, c_double), byref(res),
                                               None if chi2 is None else _ptr(chi2, c_double)), "scl_pgo_optimize")
        return out[:n], res, None if chi2 is None else chi2[:m]

    @staticmethod
    def pgo_count_junctions(n_poses, f_i, f_j, p_idx):
        """(n_junctions, n_segments, longest_segment) of the condensed direct step (scl_engine.h: POSE-GRAPH SOLVE, CONDENSED DIRECT STEP);
        host only.  More than 1024 junctions: pgo_solve_condensed and pgo_optimize_condensed refuse the graph"""
        lib = load_library(); _bind(lib)
        fi = np.ascontiguousarray(f_i, dtype=np.int32).reshape(-1); fj = np.ascontiguousarray(f_j, dtype=np.int32).reshape(-1)
        pi = np.ascontiguousarray(p_idx, dtype=np.int32).reshape(-1)
        if fj.size != fi.size:
            raise ValueError("f_i and f_j must have one entry per factor")
        opt = lambda a: _ptr(a, c_int) if a.size else None
        nj, ns, longest = c_int(0), c_int(0), c_int(0)
        rc = lib.scl_pgo_count_junctions(int(n_poses), opt(fi), opt(fj), fi.size, opt(pi), pi.size, byref(nj), byref(ns), byref(longest))
        if rc != 0:
            raise SclError(rc, "scl_pgo_count_junctions")
        return nj.value, ns.value, longest.value

    def pgo_solve_condensed(self, poses, f_i, f_j, f_z, f_cov, p_idx, p_z, p_cov, lam):
        """delta[n,6] with (H + lam diag(H)) delta = -g at `poses`, by the condensed direct step: exact up to rounding"""
        keep, args, n, m = self._pgo_inputs(poses, f_i, f_j, f_z, f_cov, p_idx, p_z, p_cov)
        delta = np.zeros((max(n, 1), 6))
        self._check(self._lib.scl_pgo_solve_condensed(self._h, *args, float(lam), _ptr(delta, c_double)), "scl_pgo_solve_condensed")
        return delta[:n]

    def pgo_optimize_condensed(self, poses, f_i, f_j, f_z, f_cov, p_idx, p_z, p_cov, params=None, want_chi2=True):
        """pgo_optimize with the condensed direct step in place of PCG: (poses_out, PgoResult, chi2 or None, failed_factorisations)"""
        keep, args, n, m = self._pgo_inputs(poses, f_i, f_j, f_z, f_cov, p_idx, p_z, p_cov)
        out = np.zeros((max(n, 1), 7)); res = PgoResult(); chi2 = np.zeros(max(m, 1)) if want_chi2 else None
        failed = c_int(0)
        self._check(self._lib.scl_pgo_optimize_condensed(self._h, *args, None if params is None else byref(params), _ptr(out, c_double), byref(res),
                                                         None if chi2 is None else _ptr(chi2, c_double), byref(failed)),
                    "scl_pgo_optimize_condensed")
        return out[:n], res, None if chi2 is None else chi2[:m], failed.value

    def pgo_solve_condensed_many(self, poses, f_i, f_j, f_z, f_cov, p_idx, p_z, p_cov, lam, rhs):
        """x[n_rhs,n,6] with (H + lam diag(H)) x_c = rhs_c for the columns rhs[n_rhs,n,6], on one factorisation of the condensed direct
        step (scl_engine.h: POSE-GRAPH SOLVE, MANY RIGHT-HAND SIDES AND MARGINAL COVARIANCES).  A column's bits depend on the graph and
        on that column alone"""
        keep, args, n, m = self._pgo_inputs(poses, f_i, f_j, f_z, f_cov, p_idx, p_z, p_cov)
        b = np.ascontiguousarray(rhs, dtype=np.float64).reshape(-1, max(n, 1), 6)
        x = np.zeros(b.shape)
        self._check(self._lib.scl_pgo_solve_condensed_many(self._h, *args, float(lam), _ptr(b, c_double), b.shape[0], _ptr(x, c_double)),
                    "scl_pgo_solve_condensed_many")
        return x

    def pgo_marginals(self, poses, f_i, f_j, f_z, f_cov, p_idx, p_z, p_cov, q_i, q_j, want_blocks=True, want_rel=True):
        """(blocks[k,6,6] or None, rel[k,6,6] or None) for the queries (q_i[k], q_j[k]): blocks = Sigma[q_i, q_j] of Sigma = H^-1 at `poses`
        (right perturbations, rotation first), rel = the first-order covariance of X_i^-1 X_j.  At most 256 distinct poses.  rel is a
        difference of terms of the size of Sigma_jj: see the header for what that costs far from the prior"""
        keep, args, n, m = self._pgo_inputs(poses, f_i, f_j, f_z, f_cov, p_idx, p_z, p_cov)
        qi = np.ascontiguousarray(q_i, dtype=np.int32).reshape(-1); qj = np.ascontiguousarray(q_j, dtype=np.int32).reshape(-1)
        if qj.size != qi.size:
            raise ValueError("q_i and q_j must have one entry per query")
        k = qi.size
        blocks = np.zeros((max(k, 1), 6, 6)) if want_blocks else None
        rel = np.zeros((max(k, 1), 6, 6)) if want_rel else None
        opt = lambda a: _ptr(a, c_int) if a.size else None
        self._check(self._lib.scl_pgo_marginals(self._h, *args, opt(qi), opt(qj), k, None if blocks is None else _ptr(blocks, c_double),
                                                None if rel is None else _ptr(rel, c_double)), "scl_pgo_marginals")
        return None if blocks is None else blocks[:k], None if rel is None else rel[:k]

    # ---- the global voxel map (scl_engine.h GLOBAL MAP) ----

    def map_reset(self, leaf):
        """create or empty the engine's global map with voxels of `leaf` metres"""
        self._check(self._lib.scl_map_reset(self._h, float(leaf)), "scl_map_reset")

    @staticmethod
    def _map_ids(robots, indices):
        r = np.ascontiguousarray(robots, dtype=np.int32).ravel(); x = np.ascontiguousarray(indices, dtype=np.int32).ravel()
        if r.size != x.size:
            raise ValueError("robots and indices must have one entry per keyframe")
        return r, x

    def map_set_keyframes(self, robots, indices, poses):
        """keyframes of the store placed at poses[n,7] (x, y, z, qx, qy, qz, qw; pgo_optimize's poses_out): added, left alone where
        the pose is bitwise the one they are in the map at, or subtracted at the old pose and added at the new one"""
        r, x = self._map_ids(robots, indices)
        p = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 7)
        if p.shape[0] != r.size:
            raise ValueError("one pose of 7 doubles per keyframe")
        opt = lambda a, t: _ptr(a, t) if a.size else None
        self._check(self._lib.scl_map_set_keyframes(self._h, opt(r, c_int), opt(x, c_int), opt(p, c_double), r.size), "scl_map_set_keyframes")

    def map_remove_keyframes(self, robots, indices):
        r, x = self._map_ids(robots, indices)
        opt = lambda a, t: _ptr(a, t) if a.size else None
        self._check(self._lib.scl_map_remove_keyframes(self._h, opt(r, c_int), opt(x, c_int), r.size), "scl_map_remove_keyframes")

    def map_extract(self, box=None, count_only=False):
        """the map's voxels in ascending key as MAP_RECORD records (x, y, z, n); box = (lo xyz, hi xyz): those whose centroid lies in the
        closed box.  count_only: the number alone"""
        b = None if box is None else np.ascontiguousarray(box, dtype=np.float64).reshape(6)
        bp = None if b is None else _ptr(b, c_double)
        n = c_int(-1)
        self._check(self._lib.scl_map_extract(self._h, bp, None, 0, byref(n)), "scl_map_extract")
        if count_only:
            return n.value
        out = np.zeros(max(n.value, 1), dtype=MAP_RECORD)
        self._check(self._lib.scl_map_extract(self._h, bp, out.ctypes.data_as(c_void_p), n.value, byref(n)), "scl_map_extract")
        return out[:n.value].copy()

    def map_stats(self):
        st = MapStats()
        self._check(self._lib.scl_map_stats(self._h, byref(st)), "scl_map_stats")
        return st

    def map_last_timing(self):
        """(integrate_ms, grow_ms, extract_ms) of the last map calls made under profile_enable(1)"""
        ms = np.zeros(3, np.float64)
        self._check(self._lib.scl_map_last_timing(self._h, _ptr(ms, c_double)), "scl_map_last_timing")
        return tuple(ms.tolist())

    def selftest_map_capacity(self, slots):
        self._check(self._lib.scl_selftest_map_capacity(self._h, int(slots)), "scl_selftest_map_capacity")

    def pgo_condensed_last_timing(self):
        """(elimination, assembly, factorisation, solves and the way back) in ms, summed over the steps of the last condensed call made
        under profile_enable(1)"""
        ms = np.zeros(4)
        self._check(self._lib.scl_pgo_condensed_last_timing(self._h, _ptr(ms, c_double)), "scl_pgo_condensed_last_timing")
        return tuple(ms.tolist())

    def pgo_last_timing(self):
        """(linearize_ms, solve_ms): device time of the two stages of the last PGO call made under profile_enable(1)"""
        a, b = c_double(0.0), c_double(0.0)
        self._check(self._lib.scl_pgo_last_timing(self._h, byref(a), byref(b)), "scl_pgo_last_timing")
        return a.value, b.value

    # -- measurement ------------------------------------------------------------
    def profile_enable(self, on=True):
        """0/False off, 1/True every kernel family, 2 the SC-distance kernel only (lightest)"""
        self._check(self._lib.scl_profile_enable(self._h, int(on)), "scl_profile_enable")

    def profile_reset(self):
        self._check(self._lib.scl_profile_reset(self._h), "scl_profile_reset")

    def profile(self):
        p = SclProfile()
        self._check(self._lib.scl_profile_get(self._h, byref(p)), "scl_profile_get")
        return {name: getattr(p, name) for name, _ in SclProfile._fields_}

    def alignment_stats(self, reset=False):
        """(pairs aligned by the full-database pass, pairs whose first shift needed the exact fp64 evaluation)"""
        a, b = c_uint64(0), c_uint64(0)
        self._check(self._lib.scl_alignment_stats(self._h, byref(a), byref(b), int(bool(reset))), "scl_alignment_stats")
        return int(a.value), int(b.value)

    def survivor_stats(self, reset=False):
        """(scans through an exact pass, keyframes scored exactly for them, largest count of one scan) since the last reset"""
        q, s, m = c_uint64(0), c_uint64(0), c_uint64(0)
        self._check(self._lib.scl_survivor_stats(self._h, byref(q), byref(s), byref(m), int(bool(reset))), "scl_survivor_stats")
        return int(q.value), int(s.value), int(m.value)

    def device_name(self):
        buf = ctypes.create_string_buffer(256)
        self._check(self._lib.scl_device_name(self._h, buf, 256), "scl_device_name")
        return buf.value.decode()


class ScanContextDescriptor:
    """Python mirror of ``scan_context_descriptor : scan_descriptor`` (D.h:1304-1801).

    Constructor arguments, method names and return conventions follow the reference;
    all work is done by the GPU engine behind the C ABI.
    """

    def __init__(self, numRing=20, numSector=60, numCandidates=3, distThres=0.14, lidarHeight=1.65,
                 maxRadius=80.0, numExcludeRecent=100, treeMakingPeriod=10, searchRatio=0.1, **engine_kw):
        self.engine = ScanContextEngine(numRing, numSector, numCandidates, distThres, lidarHeight, maxRadius,
                                        numExcludeRecent, treeMakingPeriod, searchRatio, **engine_kw)

    def makeAndSaveDescriptorAndKey(self, scan, robot, index):          # D.h:25
        return self.engine.make_and_save(scan, robot, index)

    def saveDescriptorAndKey(self, descriptorMat, robot, index):       # D.h:27
        self.engine.save_from_wire(descriptorMat, robot, index)

    def detectIntraLoopClosureID(self, currentPtr):                    # D.h:29
        lid, shift, _ = self.engine.detect_intra(currentPtr)
        return lid, shift

    def detectInterLoopClosureID(self, currentPtr):                    # D.h:31
        lid, yaw, _ = self.engine.detect_inter(currentPtr)
        return lid, yaw

    def getIndex(self, key):                                           # D.h:33
        return self.engine.get_index(key)

    def getSize(self, idIn=-1):                                        # D.h:35
        return self.engine.get_size(idIn)
