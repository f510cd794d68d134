"""ctypes binding of librgbl_frontend.so (the C ABI declared in include/rgbl_frontend.h).

There is exactly one product library: the hipcc build for gfx950.  `load()` fails loudly when it is
missing or when no HIP device is usable — there is no CPU fallback.  (`bind(path)` is also used by the
test-suite to bind the CPU SIMT emulation of the same sources; the product never calls it with that.)
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "librgbl_frontend.so")

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])

RGBL_OK = 0
ERR_INVALID, ERR_NO_DEVICE, ERR_HIP, ERR_CAPACITY, ERR_OVERFLOW, ERR_EMPTY, ERR_COMM = -1, -2, -3, -4, -5, -6, -7
COMM_ID_BYTES = 128


class RgblError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("rgbl error %d: %s" % (code, msg))
        self.code = code


class ExtractorCfg(C.Structure):
    _fields_ = [("nfeatures", C.c_int), ("scale_factor", C.c_float), ("nlevels", C.c_int),
                ("ini_th_fast", C.c_int), ("min_th_fast", C.c_int), ("width", C.c_int),
                ("height", C.c_int), ("max_batch", C.c_int)]


class DepthCfg(C.Structure):
    _fields_ = [("proj", C.c_float * 12), ("min_dist", C.c_float), ("max_dist", C.c_float),
                ("mbf", C.c_float), ("method", C.c_int), ("kernel_w", C.c_int), ("kernel_h", C.c_int),
                ("kernel", C.c_uint8 * 81), ("avg_kernel_size", C.c_int), ("nn_search_radius", C.c_float),
                ("width", C.c_int), ("height", C.c_int), ("max_points", C.c_int),
                ("max_keypoints", C.c_int), ("max_batch", C.c_int)]


class KeyframeView(C.Structure):
    _fields_ = [("n", C.c_int), ("desc", C.c_void_p), ("kp_xy", C.c_void_p), ("kp_octave", C.c_void_p),
                ("kp_angle", C.c_void_p), ("uright", C.c_void_p), ("has_mappoint", C.c_void_p),
                ("n_nodes", C.c_int), ("node_id", C.c_void_p), ("node_off", C.c_void_p),
                ("node_feat", C.c_void_p), ("device", C.c_void_p)]


class TriangulationParams(C.Structure):
    _fields_ = [("F12", C.c_float * 9), ("epipole", C.c_float * 2), ("scale_factors2", C.c_void_p),
                ("level_sigma2_2", C.c_void_p), ("n_levels", C.c_int), ("only_stereo", C.c_int),
                ("coarse", C.c_int), ("check_orientation", C.c_int)]


class NewPointsKeyframe(C.Structure):
    """rgbl_new_points_keyframe (a key frame as LocalMapping::CreateNewMapPoints reads it)."""
    _fields_ = [("view", KeyframeView), ("depth", C.c_void_p), ("kp_xy_raw", C.c_void_p), ("Tcw", C.c_float * 12),
                ("Ow", C.c_float * 3), ("K", C.c_float * 4), ("mb", C.c_float), ("mbf", C.c_float),
                ("scale_factors", C.c_void_p), ("level_sigma2", C.c_void_p)]


class NewPointsParams(C.Structure):
    _fields_ = [("n_levels", C.c_int), ("ratio_factor", C.c_float), ("far_points", C.c_int), ("th_far_points", C.c_float),
                ("inertial", C.c_int), ("monocular", C.c_int), ("report_rejected", C.c_int)]


# rgbl_new_point
NEW_POINT_DTYPE = np.dtype([("neighbour", "<i4"), ("idx1", "<i4"), ("idx2", "<i4"), ("x3D", "<f4", (3,)), ("status", "u1"),
                            ("reserved", "u1", (3,))])


class PoseOptInput(C.Structure):
    """rgbl_pose_opt_input (a Frame as Optimizer::PoseOptimization reads it)."""
    _fields_ = [("n", C.c_int), ("mp_index", C.c_void_p), ("n_points", C.c_int), ("world_pos", C.c_void_p), ("pool", C.c_void_p),
                ("slot", C.c_void_p), ("kp_xy", C.c_void_p), ("kp_octave", C.c_void_p), ("uright", C.c_void_p),
                ("device", C.c_void_p), ("Tcw_q", C.c_float * 4), ("Tcw_t", C.c_float * 3), ("K", C.c_float * 4), ("bf", C.c_float),
                ("inv_level_sigma2", C.c_void_p), ("n_levels", C.c_int)]


class PoseOptDiag(C.Structure):
    _fields_ = [("iterations", C.c_int32 * 4), ("active", C.c_int32 * 4), ("chi2", C.c_double * 4), ("rounds", C.c_int32),
                ("reserved", C.c_int32), ("Tcw_q", C.c_double * 4), ("Tcw_t", C.c_double * 3)]


class PoseOptOutput(C.Structure):
    _fields_ = [("Tcw_q", C.c_float * 4), ("Tcw_t", C.c_float * 3), ("outlier", C.c_void_p), ("result", C.c_int),
                ("diag", PoseOptDiag)]


class Sim3Input(C.Structure):
    """rgbl_sim3_input (one Sim3Solver problem: the correspondences, the cameras and the drawn sample triples)."""
    _fields_ = [("n", C.c_int), ("x1c", C.c_void_p), ("x2c", C.c_void_p), ("pool", C.c_void_p), ("slot1", C.c_void_p),
                ("slot2", C.c_void_p), ("Rcw1", C.c_float * 9), ("tcw1", C.c_float * 3), ("Rcw2", C.c_float * 9),
                ("tcw2", C.c_float * 3), ("max_err1", C.c_void_p), ("max_err2", C.c_void_p), ("K1", C.c_float * 4),
                ("K2", C.c_float * 4), ("fix_scale", C.c_int), ("min_inliers", C.c_int), ("best_inliers", C.c_int),
                ("n_hyp", C.c_int), ("samples", C.c_void_p)]


class Sim3Output(C.Structure):
    _fields_ = [("selected", C.c_int), ("converged", C.c_int), ("n_inliers", C.c_int), ("iterations_run", C.c_int),
                ("T12", C.c_float * 16), ("R12", C.c_float * 9), ("t12", C.c_float * 3), ("s12", C.c_float),
                ("inlier", C.c_void_p), ("counts", C.c_void_p), ("T12_all", C.c_void_p)]


class MlpnpInput(C.Structure):
    """rgbl_mlpnp_input (one MLPnPsolver problem: the frame, the map points, the state of earlier calls and the drawn samples)."""
    _fields_ = [("n", C.c_int), ("mp_index", C.c_void_p), ("n_points", C.c_int), ("world_pos", C.c_void_p), ("pool", C.c_void_p),
                ("slot", C.c_void_p), ("kp_xy", C.c_void_p), ("kp_octave", C.c_void_p), ("device", C.c_void_p),
                ("K", C.c_float * 4), ("level_sigma2", C.c_void_p), ("n_levels", C.c_int), ("th2", C.c_float),
                ("min_inliers", C.c_int), ("best_inliers", C.c_int), ("best_mask", C.c_void_p), ("best_Tcw", C.c_float * 16),
                ("n_hyp", C.c_int), ("samples", C.c_void_p)]


class MlpnpOutput(C.Structure):
    _fields_ = [("found", C.c_int), ("no_more", C.c_int), ("n_inliers", C.c_int), ("iterations_run", C.c_int),
                ("Tcw", C.c_float * 16), ("inlier", C.c_void_p), ("best_inliers", C.c_int), ("best_mask", C.c_void_p),
                ("best_Tcw", C.c_float * 16), ("refines", C.c_int), ("counts", C.c_void_p), ("Tcw_all", C.c_void_p),
                ("gn_path", C.c_void_p)]


class TwoViewInput(C.Structure):
    """rgbl_two_view_input (one TwoViewReconstruction problem: the keys of both frames, the matches and the drawn sets)."""
    _fields_ = [("n1", C.c_int), ("n2", C.c_int), ("kp1_xy", C.c_void_p), ("kp2_xy", C.c_void_p), ("device1", C.c_void_p),
                ("device2", C.c_void_p), ("matches12", C.c_void_p), ("K", C.c_float * 4), ("sigma", C.c_float), ("n_hyp", C.c_int),
                ("samples", C.c_void_p)]


class TwoViewOutput(C.Structure):
    _fields_ = [("found", C.c_int), ("model", C.c_int), ("exit_code", C.c_int), ("SH", C.c_float), ("SF", C.c_float),
                ("best_h", C.c_int), ("best_f", C.c_int), ("H21", C.c_float * 9), ("F21", C.c_float * 9), ("R21", C.c_float * 9),
                ("t21", C.c_float * 3), ("p3d", C.c_void_p), ("triangulated", C.c_void_p), ("p3d_assigned", C.c_int),
                ("n_inliers", C.c_int), ("best_motion", C.c_int), ("aux", C.c_int), ("n_good", C.c_int * 8),
                ("parallax", C.c_float * 8), ("scores", C.c_void_p), ("models", C.c_void_p), ("inliers_h", C.c_void_p),
                ("inliers_f", C.c_void_p)]


class Sim3OptInput(C.Structure):
    """rgbl_sim3_opt_input (two key frames, the matches and the entry estimate as Optimizer::OptimizeSim3 reads them)."""
    _fields_ = [("n", C.c_int), ("mp1_index", C.c_void_p), ("match_index", C.c_void_p), ("i2", C.c_void_p),
                ("track_level2", C.c_void_p), ("n_points", C.c_int), ("bad", C.c_void_p), ("world_pos", C.c_void_p),
                ("pool", C.c_void_p), ("slot", C.c_void_p), ("Rcw1", C.c_float * 9), ("tcw1", C.c_float * 3),
                ("Rcw2", C.c_float * 9), ("tcw2", C.c_float * 3), ("kp1_xy", C.c_void_p), ("kp1_octave", C.c_void_p),
                ("device1", C.c_void_p), ("n2", C.c_int), ("kp2_xy", C.c_void_p), ("kp2_octave", C.c_void_p),
                ("device2", C.c_void_p), ("inv_level_sigma2_1", C.c_void_p), ("n_levels1", C.c_int),
                ("inv_level_sigma2_2", C.c_void_p), ("n_levels2", C.c_int), ("K1", C.c_float * 4), ("K2", C.c_float * 4),
                ("q", C.c_double * 4), ("t", C.c_double * 3), ("s", C.c_double), ("th2", C.c_float), ("fix_scale", C.c_int),
                ("all_points", C.c_int)]


class Sim3OptDiag(C.Structure):
    _fields_ = [("n_correspondences", C.c_int32), ("n_bad_mps", C.c_int32), ("n_in_kf2", C.c_int32), ("n_out_kf2", C.c_int32),
                ("n_without_mp", C.c_int32), ("n_bad", C.c_int32), ("iterations", C.c_int32 * 2), ("active", C.c_int32 * 2),
                ("chi2", C.c_double * 2), ("rounds", C.c_int32), ("reserved", C.c_int32)]


class Sim3OptOutput(C.Structure):
    _fields_ = [("result", C.c_int), ("q", C.c_double * 4), ("t", C.c_double * 3), ("s", C.c_double), ("cleared", C.c_void_p),
                ("diag", Sim3OptDiag)]


class LbaInput(C.Structure):
    """rgbl_lba_input (the vertices and edges Optimizer::LocalBundleAdjustment hands to g2o, as flat arrays)."""
    _fields_ = [("n_free", C.c_int), ("n_fixed", C.c_int), ("free_is_fixed", C.c_void_p), ("cam_q", C.c_void_p),
                ("cam_t", C.c_void_p), ("cam_K", C.c_void_p), ("cam_bf", C.c_void_p), ("n_points", C.c_int),
                ("world_pos", C.c_void_p), ("pool", C.c_void_p), ("slot", C.c_void_p), ("n_edges", C.c_int),
                ("edge_point", C.c_void_p), ("edge_cam", C.c_void_p), ("edge_obs", C.c_void_p),
                ("edge_inv_sigma2", C.c_void_p), ("max_iterations", C.c_int), ("user_lambda_init", C.c_double),
                ("stop", C.c_void_p), ("stop_after_polls", C.c_int), ("stop_byte", C.c_void_p)]


class LbaDiag(C.Structure):
    _fields_ = [("ran", C.c_int32), ("iterations", C.c_int32), ("trials", C.c_int32), ("rejected", C.c_int32),
                ("failed", C.c_int32), ("active_cams", C.c_int32), ("active_points", C.c_int32), ("polls", C.c_int32),
                ("first_chi2", C.c_double), ("last_chi2", C.c_double), ("last_lambda", C.c_double), ("cam_q", C.c_void_p),
                ("cam_t", C.c_void_p), ("point", C.c_void_p)]


class LbaOutput(C.Structure):
    _fields_ = [("cam_q", C.c_void_p), ("cam_t", C.c_void_p), ("point", C.c_void_p), ("chi2", C.c_void_p),
                ("flags", C.c_void_p), ("diag", LbaDiag)]


class BaInput(C.Structure):
    """rgbl_ba_input (the vertices and edges Optimizer::BundleAdjustment hands to g2o, as flat arrays)."""
    _fields_ = [("n_cams", C.c_int), ("cam_is_fixed", C.c_void_p), ("cam_q", C.c_void_p), ("cam_t", C.c_void_p),
                ("cam_K", C.c_void_p), ("cam_bf", C.c_void_p), ("n_points", C.c_int), ("world_pos", C.c_void_p),
                ("pool", C.c_void_p), ("slot", C.c_void_p), ("n_edges", C.c_int), ("edge_point", C.c_void_p),
                ("edge_cam", C.c_void_p), ("edge_obs", C.c_void_p), ("edge_inv_sigma2", C.c_void_p), ("robust", C.c_int),
                ("max_iterations", C.c_int), ("stop", C.c_void_p), ("stop_after_polls", C.c_int), ("stop_byte", C.c_void_p)]


class BaOutput(C.Structure):
    _fields_ = [("cam_q", C.c_void_p), ("cam_t", C.c_void_p), ("point", C.c_void_p), ("included", C.c_void_p),
                ("chi2", C.c_void_p), ("diag", LbaDiag)]


class ProjectionInput(C.Structure):
    """rgbl_projection_input (ORBmatcher::SearchByProjection(Frame&, const Frame&, th, bMono) as flat arrays)."""
    _fields_ = [("n1", C.c_int), ("valid1", C.c_void_p), ("world_pos1", C.c_void_p), ("mp_desc1", C.c_void_p),
                ("mp_observed1", C.c_void_p), ("octave1", C.c_void_p), ("angle1", C.c_void_p),
                ("n2", C.c_int), ("kp2_xy", C.c_void_p), ("kp2_octave", C.c_void_p), ("kp2_angle", C.c_void_p),
                ("uright2", C.c_void_p), ("desc2", C.c_void_p), ("grid", C.c_float * 6),
                ("Tcw_q", C.c_float * 4), ("Tcw_t", C.c_float * 3), ("Tlw_q", C.c_float * 4), ("Tlw_t", C.c_float * 3),
                ("K", C.c_float * 4), ("mb", C.c_float), ("mbf", C.c_float), ("scale_factors", C.c_void_p),
                ("n_levels", C.c_int), ("th", C.c_float), ("mono", C.c_int), ("check_orientation", C.c_int),
                ("device2", C.c_void_p)]


class KeyFrameProjectionInput(C.Structure):
    """rgbl_keyframe_projection_input (ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist))."""
    _fields_ = [("n1", C.c_int), ("valid1", C.c_void_p), ("world_pos1", C.c_void_p), ("mp_desc1", C.c_void_p),
                ("level1", C.c_void_p), ("angle1", C.c_void_p),
                ("n2", C.c_int), ("kp2_xy", C.c_void_p), ("kp2_octave", C.c_void_p), ("kp2_angle", C.c_void_p),
                ("desc2", C.c_void_p), ("occupied2", C.c_void_p), ("grid", C.c_float * 6),
                ("Tcw_q", C.c_float * 4), ("Tcw_t", C.c_float * 3), ("K", C.c_float * 4), ("scale_factors", C.c_void_p),
                ("n_levels", C.c_int), ("th", C.c_float), ("orb_dist", C.c_int), ("check_orientation", C.c_int),
                ("device2", C.c_void_p)]


class FuseInput(C.Structure):
    """rgbl_fuse_input (the per-point search of ORBmatcher::Fuse(pKF, vpMapPoints, th))."""
    _fields_ = [("n1", C.c_int), ("valid1", C.c_void_p), ("world_pos1", C.c_void_p), ("mp_desc1", C.c_void_p),
                ("level1", C.c_void_p), ("n2", C.c_int), ("kp2_xy", C.c_void_p), ("kp2_octave", C.c_void_p),
                ("uright2", C.c_void_p), ("desc2", C.c_void_p), ("grid", C.c_float * 6), ("Tcw_q", C.c_float * 4),
                ("Tcw_t", C.c_float * 3), ("K", C.c_float * 4), ("bf", C.c_float), ("scale_factors", C.c_void_p),
                ("inv_level_sigma2", C.c_void_p), ("n_levels", C.c_int), ("th", C.c_float), ("device2", C.c_void_p)]


class ProjectSearchInput(C.Structure):
    """rgbl_project_search_input (the per-point search of Fuse(pKF, Scw, ...) and SearchBySim3)."""
    _fields_ = [("n1", C.c_int), ("valid1", C.c_void_p), ("cam_pos1", C.c_void_p), ("mp_desc1", C.c_void_p),
                ("level1", C.c_void_p), ("n2", C.c_int), ("kp2_xy", C.c_void_p), ("kp2_octave", C.c_void_p),
                ("desc2", C.c_void_p), ("grid", C.c_float * 6), ("K", C.c_float * 4), ("scale_factors", C.c_void_p),
                ("n_levels", C.c_int), ("th", C.c_float), ("proj_form", C.c_int), ("max_dist", C.c_int),
                ("device2", C.c_void_p)]


class LocalPointsInput(C.Structure):
    """rgbl_local_points_input (ORBmatcher::SearchByProjection(F, vpMapPoints, th, ...) as flat arrays)."""
    _fields_ = [("n1", C.c_int), ("valid1", C.c_void_p), ("proj1", C.c_void_p), ("level1", C.c_void_p),
                ("view_cos1", C.c_void_p), ("mp_desc1", C.c_void_p), ("mp_observed1", C.c_void_p),
                ("n2", C.c_int), ("kp2_xy", C.c_void_p), ("kp2_octave", C.c_void_p), ("uright2", C.c_void_p),
                ("desc2", C.c_void_p), ("blocked2", C.c_void_p), ("grid", C.c_float * 6), ("scale_factors", C.c_void_p),
                ("n_levels", C.c_int), ("th", C.c_float), ("nnratio", C.c_float), ("device2", C.c_void_p)]


class TrackLocalInput(C.Structure):
    """rgbl_track_local_input (Tracking::SearchLocalPoints from its isInFrustum loop on: map points as host arrays or pool slots)."""
    _fields_ = [("n1", C.c_int), ("consider1", C.c_void_p), ("world_pos1", C.c_void_p), ("normal1", C.c_void_p),
                ("min_dist1", C.c_void_p), ("max_dist1", C.c_void_p), ("mp_desc1", C.c_void_p), ("pool", C.c_void_p),
                ("slot1", C.c_void_p), ("mp_observed1", C.c_void_p),
                ("n2", C.c_int), ("kp2_xy", C.c_void_p), ("kp2_octave", C.c_void_p), ("uright2", C.c_void_p),
                ("desc2", C.c_void_p), ("blocked2", C.c_void_p), ("grid", C.c_float * 6), ("scale_factors", C.c_void_p),
                ("n_levels", C.c_int), ("th", C.c_float), ("nnratio", C.c_float), ("device2", C.c_void_p),
                ("Rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("Ow", C.c_float * 3), ("K", C.c_float * 4),
                ("mbf", C.c_float), ("log_scale_factor", C.c_float), ("viewing_cos_limit", C.c_float),
                ("far_points", C.c_int), ("th_far_points", C.c_float)]


class MapRefreshInput(C.Structure):
    """rgbl_map_refresh_input (MapPoint::UpdateNormalAndDepth / ComputeDistinctiveDescriptors from resident key frames)."""
    _fields_ = [("n_points", C.c_int), ("slot", C.c_void_p), ("world_pos", C.c_void_p), ("obs_off", C.c_void_p),
                ("obs_kf", C.c_void_p), ("obs_feat", C.c_void_p), ("ref_kf", C.c_void_p), ("ref_level", C.c_void_p),
                ("n_kfs", C.c_int), ("kf_frame", C.c_void_p), ("kf_center", C.c_void_p), ("kf_bad", C.c_void_p),
                ("scale_factors", C.c_void_p), ("n_levels", C.c_int), ("do_normal", C.c_int), ("do_descriptor", C.c_int)]


class MapRefreshOutput(C.Structure):
    """rgbl_map_refresh_output: what the MapPoint objects need to stay in step (every pointer nullable)."""
    _fields_ = [("normal", C.c_void_p), ("min_dist", C.c_void_p), ("max_dist", C.c_void_p), ("best_obs", C.c_void_p),
                ("desc", C.c_void_p), ("status", C.c_void_p)]


# rgbl_frustum_record: what Frame::isInFrustum leaves in a MapPoint
FRUSTUM_DTYPE = np.dtype([("proj_x", "<f4"), ("proj_y", "<f4"), ("proj_xr", "<f4"), ("depth", "<f4"), ("view_cos", "<f4"),
                          ("level", "<i4")])


class InitializationInput(C.Structure):
    """rgbl_initialization_input (ORBmatcher::SearchForInitialization as flat arrays)."""
    _fields_ = [("n1", C.c_int), ("kp1_octave", C.c_void_p), ("kp1_angle", C.c_void_p), ("desc1", C.c_void_p),
                ("n2", C.c_int), ("kp2_xy", C.c_void_p), ("kp2_octave", C.c_void_p), ("kp2_angle", C.c_void_p),
                ("desc2", C.c_void_p), ("grid", C.c_float * 6), ("window_size", C.c_int), ("nnratio", C.c_float),
                ("check_orientation", C.c_int)]


class FeederCfg(C.Structure):
    """rgbl_feeder_cfg (host-fed batches, orb_slam3_rgbl_amd/feed.py)."""
    _fields_ = [("channels", C.c_int), ("blue_first", C.c_int), ("max_batch", C.c_int), ("max_points", C.c_int),
                ("max_points_batch", C.c_longlong), ("slots", C.c_int), ("K", C.c_float * 4), ("dist", C.c_float * 5),
                ("n_dist", C.c_int)]


class FeederResults(C.Structure):
    """rgbl_feeder_results: host (rgbl_feeder_collect) or device (rgbl_feeder_device_outputs) pointers of one batch."""
    _fields_ = [("batch", C.c_int), ("cap", C.c_int), ("kp", C.c_void_p), ("desc", C.c_void_p), ("n", C.c_void_p),
                ("mono", C.c_void_p), ("depth", C.c_void_p), ("uright", C.c_void_p), ("kpun_xy", C.c_void_p)]


class KfdbQueryInput(C.Structure):
    """rgbl_kfdb_query_input (the BowVector side of KeyFrameDatabase::Detect*Candidates)."""
    _fields_ = [("n_words", C.c_int), ("word_id", C.c_void_p), ("word_val", C.c_void_p), ("n_excluded", C.c_int),
                ("excluded_kf", C.c_void_p), ("min_words_floor", C.c_int)]


class KfdbQueryOutput(C.Structure):
    """rgbl_kfdb_query_output (lKFsSharingWords with mn*Words and the scores)."""
    _fields_ = [("cap", C.c_int), ("share_kf", C.c_void_p), ("share_words", C.c_void_p), ("share_score", C.c_void_p),
                ("scored", C.c_void_p), ("n_share", C.c_int), ("max_common_words", C.c_int), ("min_common_words", C.c_int)]


# name -> (restype, argtypes); every symbol of include/rgbl_frontend.h
_V, _I, _F, _Z = C.c_void_p, C.c_int, C.c_float, C.c_size_t
SYMBOLS = {
    "rgbl_last_error": (C.c_char_p, []),
    "rgbl_backend": (C.c_char_p, []),
    "rgbl_device_count": (_I, []),
    "rgbl_extractor_create": (_I, [C.POINTER(ExtractorCfg), _I, C.POINTER(_V)]),
    "rgbl_extractor_destroy": (None, [_V]),
    "rgbl_extractor_tables": (_I, [_V, _V, _V, _V, _V, _V, _V]),
    "rgbl_extractor_max_keypoints": (_I, [_V]),
    "rgbl_extract": (_I, [_V, _V, _I, _I, _I, _I, _I, _V, _V, _I, C.POINTER(_I), C.POINTER(_I)]),
    "rgbl_extract_begin": (_I, [_V, _V, _I, _I, _I, _I, _I]),
    "rgbl_extract_cancel": (_I, [_V]),
    "rgbl_extract_batch": (_I, [_V, _V, _I, _I, _I, _I, _Z, _I, _I, _V, _V, _I, _V, _V]),
    "rgbl_extract_batch_device": (_I, [_V, _V, _I, _I, _I, _I, _Z, _I, _I, _V, _V, _I, _V, _V]),
    "rgbl_extractor_sync": (_I, [_V]),
    "rgbl_extractor_level_size": (_I, [_V, _I, C.POINTER(_I), C.POINTER(_I)]),
    "rgbl_extractor_get_level": (_I, [_V, _I, _I, _I, _I, _V, _I]),
    "rgbl_extractor_get_candidates": (_I, [_V, _I, _I, _V, _I, C.POINTER(_I)]),
    "rgbl_cvt_gray_batch_device": (_I, [_V, _V, _I, _I, _I, _I, _I, _I, _Z, _V, _I, _Z]),
    "rgbl_extract_color": (_I, [_V, _V, _I, _I, _I, _I, _I, _I, _I, _V, _V, _I, C.POINTER(_I), C.POINTER(_I), _V, _I]),
    "rgbl_rectifier_create": (_I, [_I, _I, _I, _I, _I, _V, _V, _I, C.POINTER(_V)]),
    "rgbl_rectifier_destroy": (None, [_V]),
    "rgbl_rectifier_info": (_I, [_V, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), C.POINTER(_I),
                                 C.POINTER(C.c_longlong)]),
    "rgbl_remap_batch_device": (_I, [_V, _V, _V, _I, _I, _I, _Z, _V, _I, _Z]),
    "rgbl_remap": (_I, [_V, _V, _I, _I, _V, _I]),
    "rgbl_extract_rectified": (_I, [_V, _V, _V, _I, _I, _I, _I, _I, _I, _I, _V, _V, _I, C.POINTER(_I), C.POINTER(_I), _V, _I]),
    "rgbl_resizer_create": (_I, [_I, _I, _I, _I, _I, C.POINTER(_V)]),
    "rgbl_resizer_destroy": (None, [_V]),
    "rgbl_resizer_info": (_I, [_V, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), C.POINTER(C.c_longlong)]),
    "rgbl_resize_batch_device": (_I, [_V, _V, _V, _I, _I, _I, _Z, _V, _I, _Z]),
    "rgbl_resize": (_I, [_V, _V, _I, _I, _V, _I]),
    "rgbl_extract_resized": (_I, [_V, _V, _V, _I, _I, _I, _I, _I, _I, _I, _V, _V, _I, C.POINTER(_I), C.POINTER(_I), _V, _I]),
    "rgbl_stereo_matches": (_I, [_V, _V, _V, _V, _I, _V, _V, _I, _F, _F, _V, _V]),
    "rgbl_stereo_matches_batch_device": (_I, [_V, _V, _I, _V, _V, _V, _V, _V, _V, _I, _F, _F, _V, _V]),
    "rgbl_extractor_debug_stamps": (_I, [_V, _V, _I]),
    "rgbl_selftest_wrappers": (_I, [_I, _I, C.c_uint]),
    "rgbl_extractor_set_stream": (_I, [_V, _V]),
    "rgbl_extractor_profile": (_I, [_V, _I]),
    "rgbl_extractor_profile_read": (_I, [_V, _V, _V, _V, _I]),
    "rgbl_extractor_profile_samples": (_I, [_V, _I, _V, _I]),
    "rgbl_depth_create": (_I, [C.POINTER(DepthCfg), _I, C.POINTER(_V)]),
    "rgbl_depth_destroy": (None, [_V]),
    "rgbl_projection_matrix": (None, [_V, _V, _V]),
    "rgbl_structuring_element": (_I, [_I, _I, _I, _V]),
    "rgbl_depth_compute_xyzi": (_I, [_V, _V, _I, _I, _I, _V, _V, _I, _V, _V, _V, _V]),
    "rgbl_depth_project_xyzi_batch_device": (_I, [_V, _V, _I, _I, _Z, _I, _I, _V]),
    "rgbl_depth_project_xyzi_varlen_batch_device": (_I, [_V, _V, _V, _I, _I, _I, _I, _V]),
    "rgbl_depth_compute": (_I, [_V, _V, _I, _I, _I, _I, _V, _V, _I, _V, _V, _V, _V]),
    "rgbl_depth_prefetch": (_I, [_V, _V, _I, _I, _I, _I]),
    "rgbl_depth_prefetch_xyzi": (_I, [_V, _V, _I, _I, _I]),
    "rgbl_depth_prefetch_cancel": (_I, [_V]),
    "rgbl_depth_batch_device": (_I, [_V, _V, _I, _I, _I, _Z, _I, _I, _V, _V, _I, _V, _V, _V, _V]),
    "rgbl_depth_project_batch_device": (_I, [_V, _V, _I, _I, _I, _Z, _I, _I, _V]),
    "rgbl_depth_gather_batch_device": (_I, [_V, _I, _I, _I, _V, _V, _I, _V, _V, _V]),
    "rgbl_depth_sync": (_I, [_V]),
    "rgbl_depth_stream": (_V, [_V]),
    "rgbl_undistort_points": (_I, [_V, _V, _I, _V, _V, _I, _V]),
    "rgbl_undistort_keypoints_batch_device": (_I, [_V, _V, _V, _I, _I, _V, _V, _I, _V]),
    "rgbl_extractor_stream": (_V, [_V]),
    "rgbl_extractor_aux_stream": (_V, [_V]),
    "rgbl_matcher_stream": (_V, [_V]),
    "rgbl_stream_wait": (_I, [_V, _V]),
    "rgbl_pack_records_device": (_I, [_V, _V, _V, _V, _V, _V, _I, _I, C.c_longlong, C.c_longlong, _V, _V, _V]),
    "rgbl_comm_available": (_I, []),
    "rgbl_comm_unique_id": (_I, [_V]),
    "rgbl_comm_create": (_I, [_V, _I, _I, _I, C.POINTER(_V)]),
    "rgbl_comm_destroy": (None, [_V]),
    "rgbl_comm_info": (_I, [_V, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), C.POINTER(_I)]),
    "rgbl_gather_create": (_I, [_V, _I, _I, _I, _I, _V, C.POINTER(_V)]),
    "rgbl_gather_destroy": (None, [_V]),
    "rgbl_gather_stream": (_V, [_V]),
    "rgbl_gather_set_loopback": (_I, [_V, _I]),
    "rgbl_gather_pack": (_I, [_V, _I, _V, _V, _V, _V, _V, _V, _I, _V]),
    "rgbl_gather_exchange": (_I, [_V, _I]),
    "rgbl_gather_sync": (_I, [_V]),
    "rgbl_gather_result": (_I, [_V, _I, C.POINTER(_V), C.POINTER(_V), C.POINTER(C.c_longlong)]),
    "rgbl_gather_copy_result": (_I, [_V, _I, _V, C.c_longlong]),
    "rgbl_event_create": (_I, [C.POINTER(_V)]),
    "rgbl_event_destroy": (None, [_V]),
    "rgbl_event_record": (_I, [_V, _V]),
    "rgbl_event_wait": (_I, [_V, _V]),
    "rgbl_stream_create": (_I, [C.POINTER(_V), _I]),
    "rgbl_stream_create_on": (_I, [_I, C.POINTER(_V), _I]),
    "rgbl_stream_destroy": (None, [_V]),
    "rgbl_depth_set_stream": (_I, [_V, _V]),
    "rgbl_depth_set_sparse": (_I, [_V, _I]),
    "rgbl_depth_profile": (_I, [_V, _I]),
    "rgbl_depth_profile_read": (_I, [_V, _V, _V, _V, _I]),
    "rgbl_depth_profile_samples": (_I, [_V, _I, _V, _I]),
    "rgbl_matcher_create": (_I, [_I, C.POINTER(_V)]),
    "rgbl_matcher_destroy": (None, [_V]),
    "rgbl_matcher_sync": (_I, [_V]),
    "rgbl_matcher_set_stream": (_I, [_V, _V]),
    "rgbl_matcher_profile": (_I, [_V, _I]),
    "rgbl_matcher_profile_read": (_I, [_V, _V, _V, _V, _I]),
    "rgbl_matcher_profile_samples": (_I, [_V, _I, _V, _I]),
    "rgbl_descriptor_distance": (_I, [_V, _V]),
    "rgbl_matcher_acquire": (_I, [_I, C.POINTER(_V)]),
    "rgbl_matcher_release": (None, [_V]),
    "rgbl_matcher_pool_size": (_I, []),
    "rgbl_matcher_pool_clear": (_I, []),
    "rgbl_hamming_bf": (_I, [_V, _V, _I, _V, _I, _V, _V, _V]),
    "rgbl_stereo_fisheye_matches": (_I, [_V, _V, _I, _I, _V, _I, _I, _V, _V, _V]),
    "rgbl_hamming_bf_batch_device": (_I, [_V, _V, _V, _I, _V, _V, _I, _V, _V, _V]),
    "rgbl_search_triangulation": (_I, [_V, C.POINTER(KeyframeView), C.POINTER(KeyframeView),
                                       C.POINTER(TriangulationParams), _V, C.POINTER(_I)]),
    "rgbl_triangulate_matches": (_I, [_V, C.POINTER(NewPointsKeyframe), C.POINTER(NewPointsKeyframe), C.POINTER(NewPointsParams),
                                      _I, _V, _V, _V]),
    "rgbl_triangulate_matches_host": (_I, [C.POINTER(NewPointsKeyframe), C.POINTER(NewPointsKeyframe), C.POINTER(NewPointsParams),
                                           _I, _V, _V, _V]),
    "rgbl_create_new_map_points": (_I, [_V, C.POINTER(NewPointsKeyframe), _I, _V, _V, _V, C.POINTER(NewPointsParams), _V, _I,
                                        C.POINTER(_I), _V, _V]),
    "rgbl_pose_optimization": (_I, [_V, C.POINTER(PoseOptInput), C.POINTER(PoseOptOutput)]),
    "rgbl_pose_optimization_batch": (_I, [_V, _I, _V, _V]),
    "rgbl_pose_optimization_host": (_I, [C.POINTER(PoseOptInput), C.POINTER(PoseOptOutput)]),
    "rgbl_sim3_ransac": (_I, [_V, C.POINTER(Sim3Input), C.POINTER(Sim3Output)]),
    "rgbl_sim3_ransac_batch": (_I, [_V, _I, _V, _V]),
    "rgbl_sim3_ransac_host": (_I, [C.POINTER(Sim3Input), C.POINTER(Sim3Output)]),
    "rgbl_mlpnp_ransac": (_I, [_V, C.POINTER(MlpnpInput), C.POINTER(MlpnpOutput)]),
    "rgbl_mlpnp_ransac_batch": (_I, [_V, _I, _V, _V]),
    "rgbl_mlpnp_ransac_host": (_I, [C.POINTER(MlpnpInput), C.POINTER(MlpnpOutput)]),
    "rgbl_two_view_reconstruct": (_I, [_V, C.POINTER(TwoViewInput), C.POINTER(TwoViewOutput)]),
    "rgbl_two_view_reconstruct_batch": (_I, [_V, _I, _V, _V]),
    "rgbl_two_view_reconstruct_host": (_I, [C.POINTER(TwoViewInput), C.POINTER(TwoViewOutput)]),
    "rgbl_optimize_sim3": (_I, [_V, C.POINTER(Sim3OptInput), C.POINTER(Sim3OptOutput)]),
    "rgbl_optimize_sim3_batch": (_I, [_V, _I, _V, _V]),
    "rgbl_optimize_sim3_host": (_I, [C.POINTER(Sim3OptInput), C.POINTER(Sim3OptOutput)]),
    "rgbl_local_bundle_adjustment": (_I, [_V, C.POINTER(LbaInput), C.POINTER(LbaOutput)]),
    "rgbl_local_bundle_adjustment_host": (_I, [C.POINTER(LbaInput), C.POINTER(LbaOutput)]),
    "rgbl_bundle_adjustment": (_I, [_V, C.POINTER(BaInput), C.POINTER(BaOutput)]),
    "rgbl_bundle_adjustment_host": (_I, [C.POINTER(BaInput), C.POINTER(BaOutput)]),
    "rgbl_search_by_bow": (_I, [_V, _V, _V, _F, _I, _V, C.POINTER(_I)]),
    "rgbl_search_by_bow_rig": (_I, [_V, _V, _V, _I, _F, _I, _V, C.POINTER(_I)]),
    "rgbl_search_by_bow_keyframes": (_I, [_V, _V, _V, _F, _I, _V, C.POINTER(_I)]),
    "rgbl_search_by_projection": (_I, [_V, _V, _V, C.POINTER(_I)]),
    "rgbl_search_local_points": (_I, [_V, _V, _V, C.POINTER(_I)]),
    "rgbl_map_points_create": (_I, [_I, _I, C.POINTER(_V)]),
    "rgbl_map_points_destroy": (None, [_V]),
    "rgbl_map_points_reserve": (_I, [_V, _I]),
    "rgbl_map_points_capacity": (_I, [_V]),
    "rgbl_map_points_update": (_I, [_V, _I, _V, _V, _V, _V, _V, _V]),
    "rgbl_map_points_download": (_I, [_V, _I, _V, _V, _V, _V, _V, _V]),
    "rgbl_map_points_refresh": (_I, [_V, _V, C.POINTER(MapRefreshInput), C.POINTER(MapRefreshOutput)]),
    "rgbl_frustum_cull": (_I, [_V, _V, _V, _V, C.POINTER(_I)]),
    "rgbl_track_local_points": (_I, [_V, _V, _V, _V, C.POINTER(_I), _V, C.POINTER(_I)]),
    "rgbl_search_for_initialization": (_I, [_V, _V, _V, _V, C.POINTER(_I)]),
    "rgbl_fuse_search": (_I, [_V, _V, _V, _V]),
    "rgbl_project_search": (_I, [_V, _V, _V, _V]),
    "rgbl_search_by_projection_sim3": (_I, [_V, _V, _V, _V, C.POINTER(_I)]),
    "rgbl_distinctive_descriptors": (_I, [_V, _V, _V, _I, _V]),
    "rgbl_search_by_projection_keyframe": (_I, [_V, _V, _V, C.POINTER(_I)]),
    "rgbl_vocabulary_load_text": (_I, [C.c_char_p, _I, C.POINTER(_V)]),
    "rgbl_vocabulary_create": (_I, [_I, _I, _V, _V, _V, _V, _V, _I, C.POINTER(_V)]),
    "rgbl_vocabulary_destroy": (None, [_V]),
    "rgbl_vocabulary_info": (_I, [_V, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), C.POINTER(_I)]),
    "rgbl_bow_transform": (_I, [_V, _V, _I, _I, _V, _V, _I, C.POINTER(_I), _V, _V, _V, _I, C.POINTER(_I)]),
    "rgbl_bow_descend_batch_device": (_I, [_V, _V, _V, _V, _I, _I, _I, _V, _V, _V]),
    "rgbl_fundamental": (None, [_V, _V, _V, _V, _V]),
    "rgbl_device_frame_create": (_I, [_I, _I, C.POINTER(_V)]),
    "rgbl_device_frame_destroy": (None, [_V]),
    "rgbl_device_frame_upload": (_I, [_V, _I, _V, _V, _V, _V]),
    "rgbl_device_frame_capture": (_I, [_V, _V, _I, _I, _V, _V, _V, _I]),
    "rgbl_device_frame_set_feature_vector": (_I, [_V, _I, _V, _V]),
    "rgbl_device_frame_size": (_I, [_V]),
    "rgbl_device_frame_set_grid": (_I, [_V, _V]),
    "rgbl_device_frame_download": (_I, [_V, _V, _V, _V, _V]),
    "rgbl_feeder_create": (_I, [C.POINTER(FeederCfg), _V, _V, C.POINTER(_V)]),
    "rgbl_feeder_destroy": (None, [_V]),
    "rgbl_feeder_acquire": (_I, [_V, C.POINTER(_I)]),
    "rgbl_feeder_image": (_I, [_V, _I, _I, C.POINTER(_V)]),
    "rgbl_feeder_scan": (_I, [_V, _I, _I, _I, C.POINTER(_V)]),
    "rgbl_feeder_submit": (_I, [_V, _I, _I]),
    "rgbl_feeder_collect": (_I, [_V, _I, C.POINTER(FeederResults)]),
    "rgbl_feeder_device_outputs": (_I, [_V, _I, C.POINTER(FeederResults), C.POINTER(_V)]),
    "rgbl_feeder_pinned_bytes": (C.c_longlong, [_V]),
    "rgbl_bow_transform_frame": (_I, [_V, _V, _I, _V, _V, _I, C.POINTER(_I), _V, _V, _V, _I, C.POINTER(_I)]),
    "rgbl_kfdb_create": (_I, [_I, _I, C.POINTER(_V)]),
    "rgbl_kfdb_destroy": (None, [_V]),
    "rgbl_kfdb_add": (_I, [_V, C.c_int64, C.c_int32, _I, _V, _V]),
    "rgbl_kfdb_erase": (_I, [_V, C.c_int64]),
    "rgbl_kfdb_clear": (_I, [_V]),
    "rgbl_kfdb_clear_map": (_I, [_V, C.c_int32]),
    "rgbl_kfdb_set_map": (_I, [_V, C.c_int64, C.c_int32]),
    "rgbl_kfdb_size": (_I, [_V, C.POINTER(_I), C.POINTER(C.c_longlong)]),
    "rgbl_kfdb_arena_info": (_I, [_V, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(_I), C.POINTER(_I)]),
    "rgbl_kfdb_query": (_I, [_V, C.POINTER(KfdbQueryInput), C.POINTER(KfdbQueryOutput)]),
    "rgbl_kfdb_query_batch": (_I, [_V, _I, _V, _V, _V, _V, _V, _V, _I, _V, _V, _V, _V, _V, _V, _V]),
    "rgbl_kfdb_profile": (_I, [_V, _I]),
    "rgbl_kfdb_profile_read": (_I, [_V, _V, _V, _V, _I]),
}


def bind(path):
    """dlopen `path` and attach the prototypes of every symbol in include/rgbl_frontend.h."""
    lib = C.CDLL(path)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export it
        fn.restype = res
        fn.argtypes = args
    return lib


_lib = None


def load():
    """The product library. Raises if it has not been built (run __graft_entry__.build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RgblError(ERR_NO_DEVICE, "%s not built; run `python -c 'import __graft_entry__ as g; g.build()'` "
                                           "(there is no CPU fallback)" % LIB_PATH)
        _lib = bind(LIB_PATH)
    return _lib


def check(lib, rc):
    if rc != RGBL_OK:
        raise RgblError(rc, lib.rgbl_last_error().decode("utf-8", "replace"))
    return rc


def ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def read_profile(lib, fn, handle):
    names = (C.c_char_p * 32)()
    ms = (C.c_double * 32)()
    cnt = (C.c_long * 32)()
    n = fn(handle, C.cast(names, C.c_void_p), C.cast(ms, C.c_void_p), C.cast(cnt, C.c_void_p), 32)
    return {names[i].decode(): (ms[i], cnt[i]) for i in range(min(n, 32))}


def read_profile_samples(lib, fn_read, fn_samples, handle):
    """{kernel: [every launch's duration in ms, launch order]} since profiling was switched on."""
    names = (C.c_char_p * 32)()
    n = fn_read(handle, C.cast(names, C.c_void_p), None, None, 32)
    out = {}
    for i in range(min(n, 32)):
        k = fn_samples(handle, i, None, 0)
        buf = (C.c_float * max(k, 1))()
        k = fn_samples(handle, i, C.cast(buf, C.c_void_p), k)
        out[names[i].decode()] = [float(buf[j]) for j in range(k)]
    return out
