"""ctypes binding of libopd_hip.so — the only way the package reaches the GPU.

There is NO CPU fallback: if the shared library is missing (not built) or no HIP device is visible, the calls raise.
The declarations mirror ``include/opd_detr.h`` one to one.
"""

from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libopd_hip.so")
TEST_LIB_PATH = os.path.join(_HERE, "libopd_hip_test.so")   # the same objects + csrc/opd_*test*_api.cpp: tests/ and tools/ only

OPD_PIXELS_U8_BGR_HWC = 0
OPD_PIXELS_F32_NCHW = 1
OPD_MEM_HOST = 0
OPD_MEM_DEVICE = 1
OPD_MEM_HOST_PIXELS_DEVICE_OUT = 2
OPD_FLAG_NO_GRAPH = 1
OPD_FLAG_MULTI_STREAM = 2
OPD_REID_MODEL_CLIP = 0
OPD_REID_MODEL_OSNET = 1
OPD_TRACK_FEAT_NONE, OPD_TRACK_FEAT_ENCODER, OPD_TRACK_FEAT_COLOR, OPD_TRACK_FEAT_REID = 0, 1, 2, 3   # feature_kind of opd_detr_detect_frames_track
OPD_FLAG_BF16 = 4
OPD_FLOOR_HOMOGRAPHY, OPD_FLOOR_PWA, OPD_FLOOR_TPS = 0, 1, 2
OPD_FLOOR_VALID, OPD_FLOOR_WITHIN, OPD_FLOOR_EXTRAPOLATED = 1, 2, 4
OPD_FLOOR_MAX_POINTS, OPD_FLOOR_MAX_TRIANGLES, OPD_FLOOR_MAX_ZONES, OPD_FLOOR_MAX_VERTICES = 256, 512, 64, 64
OPD_COMM_ID_BYTES = 128
OPD_OK, OPD_EINVAL, OPD_EIO, OPD_ESCHEMA, OPD_EHIP, OPD_ENOMEM, OPD_ESTATE = 0, -1, -2, -3, -4, -5, -6   # include/opd_detr.h


class OpdConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("max_batch", C.c_int32), ("max_height", C.c_int32),
                ("max_width", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32 * 3)]


class OpdKernelStat(C.Structure):   # opd_kernel_stat (include/opd_detr.h)
    _fields_ = [("name", C.c_char * 96), ("launches", C.c_int32), ("ms", C.c_float), ("flops", C.c_double)]


class OpdDet(C.Structure):
    _fields_ = [("x1", C.c_float), ("y1", C.c_float), ("x2", C.c_float), ("y2", C.c_float), ("score", C.c_float),
                ("label", C.c_int32), ("query_index", C.c_int32), ("frame", C.c_int32)]


class OpdTileDet(C.Structure):   # opd_tile_det (48 bytes): a merged detection of a tiled frame, frame pixels
    _fields_ = [("x", C.c_double), ("y", C.c_double), ("w", C.c_double), ("h", C.c_double), ("score", C.c_float), ("label", C.c_int32),
                ("query_index", C.c_int32), ("tile", C.c_int32)]


class OpdTileParams(C.Structure):   # opd_tile_params (40 bytes)
    _fields_ = [("struct_size", C.c_int32), ("person_label", C.c_int32), ("tile_nms_threshold", C.c_float), ("pad", C.c_float),
                ("merge_nms_threshold", C.c_double), ("merge_threshold", C.c_double), ("edge_tolerance", C.c_double)]


class OpdModelInfo(C.Structure):
    _fields_ = [("depths", C.c_int32 * 4), ("d_model", C.c_int32), ("heads", C.c_int32), ("ffn_dim", C.c_int32),
                ("encoder_layers", C.c_int32), ("decoder_layers", C.c_int32), ("num_queries", C.c_int32),
                ("num_classes_plus1", C.c_int32), ("max_batch", C.c_int32), ("max_height", C.c_int32),
                ("max_width", C.c_int32), ("device_ordinal", C.c_int32), ("weight_bytes_device", C.c_int64),
                ("workspace_bytes_device", C.c_int64)]


class OpdReidConfig(C.Structure):   # opd_reid_config (include/opd_detr.h)
    _fields_ = [("struct_size", C.c_int32), ("max_crops", C.c_int32), ("flags", C.c_int32), ("model", C.c_int32), ("reserved", C.c_int32 * 4)]


class OpdReidModelInfo(C.Structure):   # opd_reid_model_info
    _fields_ = [("feature_dim", C.c_int32), ("tokens", C.c_int32), ("hidden", C.c_int32), ("layers", C.c_int32), ("heads", C.c_int32),
                ("mlp_dim", C.c_int32), ("patch", C.c_int32), ("max_crops", C.c_int32), ("device_ordinal", C.c_int32),
                ("model", C.c_int32), ("weight_bytes_device", C.c_int64), ("workspace_bytes_device", C.c_int64)]


class OpdFlowConfig(C.Structure):   # opd_flow_config (zeros = the defaults of cv2.calcOpticalFlowPyrLK as the reference calls it)
    _fields_ = [("max_h", C.c_int), ("max_w", C.c_int), ("max_points", C.c_int), ("win", C.c_int), ("max_level", C.c_int),
                ("max_iter", C.c_int), ("epsilon", C.c_float), ("min_eig_threshold", C.c_float)]


class OpdTileStages(C.Structure):   # opd_tile_stages (56 bytes): the feature, floor and track stages of opd_detr_detect_tiled_stages
    _fields_ = [("struct_size", C.c_int32), ("feature_kind", C.c_int32), ("features", C.c_void_p), ("floor", C.c_void_p), ("floor_out", C.c_void_p),
                ("trackers", C.c_void_p), ("track_ids", C.c_void_p), ("n_featured", C.c_void_p)]


class OpdTileReidStages(C.Structure):   # opd_tile_reid_stages (80 bytes): the Re-ID, floor and track stages of opd_detr_detect_tiled_reid
    _fields_ = [("struct_size", C.c_int32), ("slots", C.c_int32), ("reid", C.c_void_p), ("features", C.c_void_p), ("slot_map", C.c_void_p), ("n_person", C.c_void_p),
                ("floor", C.c_void_p), ("floor_out", C.c_void_p), ("trackers", C.c_void_p), ("track_ids", C.c_void_p), ("n_featured", C.c_void_p)]


class OpdTileHybrid(C.Structure):   # opd_tile_hybrid (40 bytes): the hybrid trackers and the floor stage of opd_detr_detect_tiled_hybrid
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32), ("trackers", C.c_void_p), ("track_ids", C.c_void_p), ("floor", C.c_void_p), ("floor_out", C.c_void_p)]


class OpdFloorConfig(C.Structure):   # opd_floor_config: everything is copied at creation
    _fields_ = [("method", C.c_int32), ("n_points", C.c_int32), ("n_triangles", C.c_int32), ("n_zones", C.c_int32), ("has_distortion", C.c_int32),
                ("allow_overlap", C.c_int32), ("width_px", C.c_int32), ("height_px", C.c_int32), ("H", C.c_double * 9),
                ("scale_x_mm_per_px", C.c_double), ("scale_y_mm_per_px", C.c_double), ("intrinsics", C.c_double * 4), ("distortion", C.c_double * 5),
                ("tps_affine", C.c_double * 6), ("points", C.c_void_p), ("triangles", C.c_void_p), ("affine", C.c_void_p), ("tps_weights", C.c_void_p),
                ("zone_vertices", C.c_void_p), ("zone_offsets", C.c_void_p), ("zone_priority", C.c_void_p)]


class OpdFloorRec(C.Structure):   # opd_floor_rec (48 bytes)
    _fields_ = [("px", C.c_double * 2), ("mm", C.c_double * 2), ("zone_mask", C.c_uint64), ("triangle", C.c_int32), ("flags", C.c_uint32)]


class OpdFloorModelInfo(C.Structure):   # opd_floor_model_info
    _fields_ = [(n, C.c_int32) for n in ("method", "n_points", "n_triangles", "n_zones", "n_edges", "has_distortion", "allow_overlap", "device_ordinal")]


class OpdTrackConfig(C.Structure):   # opd_track_config (64 bytes): zeros = the reference's defaults
    _fields_ = [("struct_size", C.c_int32), ("max_tracks", C.c_int32), ("max_dets", C.c_int32), ("feature_dim", C.c_int32), ("max_age", C.c_int32),
                ("min_hits", C.c_int32), ("iou_threshold", C.c_double), ("appearance_weight", C.c_double), ("motion_weight", C.c_double),
                ("max_position_distance", C.c_double), ("high_conf_threshold", C.c_double)]


class OpdTrackRec(C.Structure):   # opd_track_rec (48 bytes)
    _fields_ = [("track_id", C.c_int32), ("age", C.c_int32), ("hits", C.c_int32), ("time_since_update", C.c_int32), ("x", C.c_float * 4),
                ("box", C.c_float * 4)]


class OpdTrackStatus(C.Structure):   # opd_track_status
    _fields_ = [(n, C.c_int32) for n in ("max_tracks", "max_dets", "feature_dim", "max_age", "min_hits", "device_ordinal", "n_tracks", "next_id",
                                         "last_launches", "last_waits")]


class OpdLwtConfig(C.Structure):   # opd_lwt_config (72 bytes): zeros = the reference's defaults
    _fields_ = [("struct_size", C.c_int32), ("max_tracks", C.c_int32), ("max_dets", C.c_int32), ("max_age", C.c_int32), ("use_optical_flow", C.c_int32),
                ("reserved", C.c_int32 * 3), ("iou_threshold", C.c_double), ("flow", OpdFlowConfig)]


class OpdLwtRec(C.Structure):   # opd_lwt_rec (40 bytes)
    _fields_ = [("track_id", C.c_int32), ("reserved", C.c_int32), ("bbox", C.c_double * 4)]


class OpdLwtTrack(C.Structure):   # opd_lwt_track (168 bytes)
    _fields_ = [("track_id", C.c_int32), ("age", C.c_int32), ("hits", C.c_int32), ("time_since_update", C.c_int32), ("x_is_float32", C.c_int32),
                ("reserved", C.c_int32), ("bbox", C.c_double * 4), ("center", C.c_double * 2), ("x", C.c_double * 4), ("P", C.c_float * 16)]


class OpdLwtStatus(C.Structure):   # opd_lwt_status
    _fields_ = [(n, C.c_int32) for n in ("max_tracks", "max_dets", "max_age", "use_optical_flow", "device_ordinal", "n_tracks", "next_id", "n_points",
                                         "last_launches", "last_waits")] + [("iou_threshold", C.c_double)]


# name -> (restype, argtypes): every symbol include/opd_detr.h declares
API = {
    "opd_detr_create": (C.c_int, [C.POINTER(OpdConfig), C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]),
    "opd_detr_destroy": (None, [C.c_void_p]),
    "opd_detr_clone": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "opd_detr_info": (C.c_int, [C.c_void_p, C.POINTER(OpdModelInfo)]),
    "opd_detr_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                   C.c_void_p, C.c_void_p]),
    "opd_detr_forward_ragged": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "opd_detr_forward_resized": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 3),
    "opd_detr_resize_u8": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p]),
    "opd_detr_detect_resized": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_float, C.POINTER(OpdDet), C.POINTER(C.c_int32)]),
    "opd_detr_detect_frames": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)] + [C.c_int] * 6 + [C.c_float, C.POINTER(OpdDet), C.POINTER(C.c_int32)]),
    "opd_detr_detect_frames_features": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)] + [C.c_int] * 5 + [C.c_float, C.c_int, C.POINTER(OpdDet), C.POINTER(C.c_int32),
                                                   C.POINTER(C.c_float)]),
    "opd_detr_detect_frames_color": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)] + [C.c_int] * 5 + [C.c_float, C.c_int, C.POINTER(OpdDet), C.POINTER(C.c_int32),
                                                C.POINTER(C.c_float)]),
    "opd_detr_postprocess": (C.c_int, [C.c_void_p, C.c_float, C.c_void_p, C.POINTER(OpdDet), C.POINTER(C.c_int32)]),
    "opd_detr_detect": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                  C.c_void_p, C.POINTER(OpdDet), C.POINTER(C.c_int32)]),
    "opd_detr_detect_ragged": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                         C.c_float, C.c_void_p, C.POINTER(OpdDet), C.POINTER(C.c_int32)]),
    "opd_detr_detect_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p,
                                        C.POINTER(OpdDet), C.POINTER(C.c_int32), C.POINTER(C.c_int)]),
    "opd_detr_wait": (C.c_int, [C.c_void_p, C.c_int]),
    "opd_person_nms": (C.c_int, [C.POINTER(OpdDet), C.c_int, C.c_int, C.c_float]),
    "opd_person_nms_batch": (C.c_int, [C.POINTER(OpdDet), C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_float]),
    "opd_detr_set_nms": (C.c_int, [C.c_void_p, C.c_int, C.c_float]),
    "opd_detr_nms_records": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float]),
    # frames, n_frames, h, w, tiles_yxhw, n_tiles, H, W, threshold, params, out, counts
    "opd_detr_detect_tiled": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float,
                                        C.POINTER(OpdTileParams), C.POINTER(OpdTileDet), C.POINTER(C.c_int32)]),
    "opd_detr_detect_tiled_stages": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float,
                                               C.POINTER(OpdTileParams), C.POINTER(OpdTileStages), C.POINTER(OpdTileDet), C.POINTER(C.c_int32)]),
    "opd_detr_detect_tiled_reid": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float,
                                             C.POINTER(OpdTileParams), C.POINTER(OpdTileReidStages), C.POINTER(OpdTileDet), C.POINTER(C.c_int32)]),
    # frames, n_frames, h, w, tiles_yxhw, n_tiles, tile_HW, threshold, params, stages (nullable), out, counts
    "opd_detr_detect_tiled_ragged": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_float,
                                               C.POINTER(OpdTileParams), C.POINTER(OpdTileStages), C.POINTER(OpdTileDet), C.POINTER(C.c_int32)]),
    # frames, n_frames, h, w, tiles_yxhw, n_tiles, tile_HW, threshold, params, stages, out, counts
    "opd_detr_detect_tiled_ragged_reid": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_float,
                                                    C.POINTER(OpdTileParams), C.POINTER(OpdTileReidStages), C.POINTER(OpdTileDet), C.POINTER(C.c_int32)]),
    # frames, n_frames, h, w, tiles_yxhw, n_tiles, H, W, tile_HW (nullable), threshold, params, hybrid block, out, counts
    "opd_detr_detect_tiled_hybrid": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_float,
                                               C.POINTER(OpdTileParams), C.POINTER(OpdTileHybrid), C.POINTER(OpdTileDet), C.POINTER(C.c_int32)]),
    # tracker, frames, is_key, F, h, w, tiles_yxhw, n_tiles, H, W, tile_HW (nullable), threshold, params, out, counts, track_ids, recs_out, capacity, rec_counts, frames_done
    "opd_detr_detect_tiled_sequence_hybrid": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                        C.c_void_p, C.c_float, C.POINTER(OpdTileParams), C.POINTER(OpdTileDet), C.POINTER(C.c_int32), C.c_void_p,
                                                        C.POINTER(OpdLwtRec), C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    # recs, tile_counts, n_frames, n_tiles, stride, tiles_yxhw, h, w, params, out, counts
    "opd_detr_merge_tiles": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                       C.POINTER(OpdTileParams), C.POINTER(OpdTileDet), C.POINTER(C.c_int32)]),
    "opd_host_alloc": (C.c_int, [C.c_size_t, C.POINTER(C.c_void_p)]),
    "opd_host_free": (None, [C.c_void_p]),
    "opd_similarity_matrix": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                        C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p]),
    "opd_detr_roi_features": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "opd_color_features": (C.c_int, [C.c_int, C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "opd_detr_attention_map": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "opd_detr_set_profiling": (C.c_int, [C.c_void_p, C.c_int]),
    "opd_detr_stage_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "opd_detr_kernel_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "opd_detr_kernel_table": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "opd_comm_available": (C.c_int, []),
    "opd_comm_unique_id": (C.c_int, [C.c_void_p]),
    "opd_comm_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "opd_comm_attach": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "opd_comm_destroy": (None, [C.c_void_p]),
    "opd_comm_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "opd_comm_begin": (C.c_int, [C.c_void_p, C.c_int]),
    "opd_comm_detect": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p]),
    "opd_comm_buffers": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "opd_comm_exchange": (C.c_int, [C.c_void_p]),
    "opd_comm_wait": (C.c_int, [C.c_void_p, C.POINTER(OpdDet), C.POINTER(C.c_int32)]),
    "opd_reid_create": (C.c_int, [C.POINTER(OpdReidConfig), C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]),
    "opd_reid_destroy": (None, [C.c_void_p]),
    "opd_reid_info": (C.c_int, [C.c_void_p, C.POINTER(OpdReidModelInfo)]),
    "opd_reid_extract": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                   C.c_void_p]),
    "opd_detr_detect_frames_reid": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)] + [C.c_int] * 5 + [C.c_float, C.c_int, C.c_int, C.POINTER(OpdDet),
                                               C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]),
    "opd_flow_create": (C.c_int, [C.POINTER(OpdFlowConfig), C.c_int, C.POINTER(C.c_void_p)]),
    "opd_flow_destroy": (None, [C.c_void_p]),
    "opd_flow_set_reference": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "opd_flow_track": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "opd_floor_create": (C.c_int, [C.POINTER(OpdFloorConfig), C.c_int, C.POINTER(C.c_void_p)]),
    "opd_floor_destroy": (None, [C.c_void_p]),
    "opd_floor_info": (C.c_int, [C.c_void_p, C.POINTER(OpdFloorModelInfo)]),
    "opd_floor_transform": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "opd_floor_transform_points": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "opd_floor_classify": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "opd_track_create": (C.c_int, [C.POINTER(OpdTrackConfig), C.c_int, C.POINTER(C.c_void_p)]),
    "opd_track_destroy": (None, [C.c_void_p]),
    "opd_track_reset": (C.c_int, [C.c_void_p]),
    "opd_track_info": (C.c_int, [C.c_void_p, C.POINTER(OpdTrackStatus)]),
    "opd_track_update": (C.c_int, [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_void_p]),
    # boxes, foot, confidence, features, has_feature, feat_mem_kind, counts, F, out_ids, frames_done
    "opd_track_update_sequence": (C.c_int, [C.c_void_p] * 6 + [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "opd_track_update_streams": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "opd_track_get": (C.c_int, [C.c_void_p, C.POINTER(OpdTrackRec), C.c_int, C.POINTER(C.c_int)]),
    "opd_detr_detect_frames_track": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)] + [C.c_int] * 5 + [C.c_float, C.c_int, C.c_int, C.c_int,
                                                C.POINTER(OpdDet), C.POINTER(C.c_int32), C.c_void_p, C.c_void_p]),
    "opd_detr_detect_sequence_track": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)] + [C.c_int] * 5 + [C.c_float, C.c_int, C.c_int, C.c_int,
                                                  C.POINTER(OpdDet), C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_void_p]),
    "opd_detr_detect_streams_track": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.POINTER(C.c_void_p)] + [C.c_int] * 5 +
                                      [C.c_float, C.c_int, C.c_int, C.c_int, C.POINTER(OpdDet), C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_void_p]),
    "opd_assign": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "opd_lwt_create": (C.c_int, [C.POINTER(OpdLwtConfig), C.c_int, C.POINTER(C.c_void_p)]),
    "opd_lwt_destroy": (None, [C.c_void_p]),
    "opd_lwt_reset": (C.c_int, [C.c_void_p]),
    "opd_lwt_info": (C.c_int, [C.c_void_p, C.POINTER(OpdLwtStatus)]),
    "opd_lwt_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "opd_lwt_interpolate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(OpdLwtRec), C.c_int, C.POINTER(C.c_int)]),
    "opd_lwt_interpolate_sequence": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(OpdLwtRec), C.c_int,
                                              C.POINTER(C.c_int32)]),
    "opd_detr_detect_frames_hybrid": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)] + [C.c_int] * 5 + [C.c_float, C.c_int, C.POINTER(OpdDet),
                                                 C.POINTER(C.c_int32), C.c_void_p]),
    "opd_detr_detect_sequence_hybrid": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p] + [C.c_int] * 5 + [C.c_float, C.c_int, C.POINTER(OpdDet),
                                                   C.POINTER(C.c_int32), C.c_void_p, C.POINTER(OpdLwtRec), C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "opd_lwt_get": (C.c_int, [C.c_void_p, C.POINTER(OpdLwtTrack), C.c_int, C.POINTER(C.c_int)]),
    "opd_detr_detect_frames_floor": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)] + [C.c_int] * 5 + [C.c_float, C.c_int, C.POINTER(OpdDet), C.POINTER(C.c_int32),
                                                C.c_void_p]),
    "opd_last_error": (C.c_char_p, []),
    "opd_version": (C.c_char_p, []),
}

# test hooks (csrc/opd_test_api.cpp: kernels; opd_test_bench_api.cpp: tools/ timing and traces; opd_test_model_api.cpp: host helpers and
# handle switches); not part of the boundary
TEST_API = {
    "opd_test_conv_gemm": (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 15),
    "opd_test_gemm_splitk_ln": (C.c_int, [C.c_void_p] * 8 + [C.c_int] * 3),
    "opd_test_gemm_k256": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 5),
    "opd_test_gemm_ln": (C.c_int, [C.c_void_p] * 8 + [C.c_int] * 2),
    "opd_test_bench_gemm_ln": (C.c_int, [C.c_int] * 4 + [C.POINTER(C.c_float)]),
    "opd_test_gemm_ln_deep": (C.c_int, [C.c_void_p] * 7 + [C.c_int] + [C.c_void_p] * 3 + [C.c_int] * 3),
    "opd_test_set_heads2": (C.c_int, [C.c_int]),
    "opd_test_set_heads_spare_rows": (C.c_int, [C.c_int]),
    "opd_test_enc_ffn": (C.c_int, [C.c_void_p] * 9 + [C.c_int] + [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p] * 2 + [C.c_int] * 2 + [C.c_void_p] * 5 + [C.c_int]),
    "opd_test_bench_enc_ffn": (C.c_int, [C.c_int] * 6 + [C.POINTER(C.c_float)]),
    "opd_test_bench_conv": (C.c_int, [C.c_int] * 11 + [C.POINTER(C.c_float)]),
    "opd_test_trace_btail": (C.c_int, [C.c_int] * 6 + [C.POINTER(C.c_ulonglong), C.c_int, C.POINTER(C.c_int)]),
    "opd_test_trace_conv": (C.c_int, [C.c_int] * 10 + [C.POINTER(C.c_ulonglong), C.c_int, C.POINTER(C.c_int)]),
    "opd_test_btail": (C.c_int, [C.c_void_p] * 10 + [C.c_int] * 6),
    "opd_test_bench_btail": (C.c_int, [C.c_int] * 8 + [C.POINTER(C.c_float)]),
    "opd_test_bench_btail_sc2": (C.c_int, [C.c_int] * 6 + [C.POINTER(C.c_float)]),
    "opd_test_btail_repeat": (C.c_int, [C.c_void_p] * 8 + [C.c_int] * 6 + [C.POINTER(C.c_int)]),
    "opd_test_attention": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_float]),
    "opd_test_layernorm": (C.c_int, [C.c_void_p] * 5 + [C.c_int]),
    "opd_test_maxpool": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 6),
    "opd_test_preprocess_u8": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 5 + [C.c_void_p]),
    "opd_test_attention_masked": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_float, C.c_void_p, C.c_int]),
    "opd_test_stem2": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 5),
    "opd_test_stem_pool": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 7),
    "opd_test_set_fuse_stem_pool": (C.c_int, [C.c_void_p, C.c_int]),
    "opd_test_set_pos_shadow": (C.c_int, [C.c_void_p, C.c_int]),
    "opd_test_stem_pool_u8": (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 3),
    "opd_test_set_fuse_btail": (C.c_int, [C.c_void_p, C.c_int]),
    "opd_test_set_fuse_gemm_ln": (C.c_int, [C.c_void_p, C.c_int]),
    "opd_test_f32_to_f16": (C.c_uint16, [C.c_float]),
    "opd_test_f16_to_f32": (C.c_float, [C.c_uint16]),
    "opd_test_normalise_key": (C.c_int, [C.c_char_p, C.c_char_p, C.c_int]),
    "opd_test_inspect_checkpoint": (C.c_int, [C.c_char_p, C.POINTER(C.c_int32)]),
    "opd_test_resize_coeffs": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]),
    "opd_test_valid_prefix": (C.c_int, [C.c_int] * 3),
    "opd_test_trunk_plan": (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_int, C.c_void_p]),
    "opd_test_trunk_plan_one_launch": (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_void_p, C.c_int]),
    "opd_test_transformer_plan": (C.c_int, [C.c_void_p] + [C.c_int] * 7 + [C.c_void_p, C.c_void_p, C.c_int]),
    "opd_test_sine_pos_embed": (C.c_int, [C.c_int] * 5 + [C.c_void_p]),
    "opd_test_conv_dual": (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 13),
    "opd_test_btail_sc": (C.c_int, [C.c_void_p] * 11 + [C.c_int] * 3),
    "opd_test_btail_sc2": (C.c_int, [C.c_void_p] * 11 + [C.c_int] * 4),
    "opd_test_btail_chain": (C.c_int, [C.c_void_p] * 13 + [C.c_int] * 4),
    "opd_test_bench_attention": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 6 + [C.c_float, C.c_int, C.POINTER(C.c_float)]),
    "opd_test_trace_attention": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 6 + [C.c_float, C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "opd_test_heads": (C.c_int, [C.c_void_p] * 13 + [C.c_int] * 2),
    "opd_test_postprocess": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_float, C.c_void_p, C.c_void_p]),
    "opd_test_roi_features": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 3 + [C.c_void_p]),
    "opd_test_set_conv_flags": (C.c_int, [C.c_int]),
    "opd_test_set_gemm_ln_kloop": (C.c_int, [C.c_int]),
    "opd_test_set_encffn_wprefetch": (C.c_int, [C.c_int]),
    "opd_test_set_pos_frames": (C.c_int, [C.c_int]),
    "opd_test_set_repeat": (C.c_int, [C.c_int]),
    "opd_test_repeat_result": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "opd_test_repeat_selftest": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "opd_test_conv_splitk": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 13),
    "opd_test_reduce_act16": (C.c_int, [C.c_void_p, C.c_int, C.c_longlong, C.c_longlong, C.c_int, C.c_void_p]),
    "opd_test_gemm_alt": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 5),
    "opd_test_gemm_frame_bias": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 7),
    "opd_test_reduce_ln_pos": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int] * 2 + [C.c_void_p] * 3 + [C.c_int]),
    "opd_test_set_graph_guard": (C.c_int, [C.c_int]),
    "opd_test_set_alloc_poison": (C.c_int, [C.c_int]),
    "opd_test_check_redzones": (C.c_int, [C.c_void_p]),
    "opd_test_set_taps": (C.c_int, [C.c_void_p, C.c_int]),
    "opd_test_read_taps": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_char_p, C.c_int]),
    "opd_test_round_f16_diffused": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "opd_test_dec_qkv": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int] * 2 + [C.c_void_p] * 4),
    "opd_test_dec_self": (C.c_int, [C.c_void_p] * 10 + [C.c_int, C.c_int, C.c_float, C.c_void_p]),
    "opd_test_attention_map": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 3 + [C.c_float, C.c_void_p, C.c_int, C.c_void_p]),
    "opd_test_attention_split": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_float, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "opd_test_dec_cross_out": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p]),
    "opd_test_dec_ffn": (C.c_int, [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p]),
    "opd_test_bench_dec": (C.c_int, [C.c_int] * 6 + [C.POINTER(C.c_float)]),
    "opd_test_heads_fused": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 13 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "opd_test_set_elem_bf16": (C.c_int, [C.c_int]),
    "opd_test_set_btail_res_regs": (C.c_int, [C.c_int]),
    "opd_test_stem_reduce": (C.c_int, [C.c_void_p] * 10 + [C.c_int] * 4),
    "opd_test_trace_dec_self": (C.c_int, [C.c_int, C.c_int, C.c_void_p]),
    # Re-ID hooks (csrc/opd_reid_test_api.cpp)
    "opd_test_reid_geometry": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "opd_test_reid_coeffs": (C.c_int, [C.c_int] * 4 + [C.c_void_p, C.c_void_p, C.c_int]),
    "opd_test_reid_lut": (C.c_int, [C.c_void_p]),
    "opd_test_reid_pixels_host": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 3 + [C.c_void_p]),
    "opd_test_reid_pixels": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                       C.c_void_p]),
    "opd_test_reid_attention": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 3),
    "opd_test_reid_layernorm": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 3),
    "opd_test_reid_gemm": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 3),
    "opd_test_reid_l2norm": (C.c_int, [C.c_void_p] + [C.c_int] * 2),
    # OSNet hooks (csrc/opd_osnet_test_api.cpp)
    "opd_test_osnet_lut": (C.c_int, [C.c_void_p]),
    "opd_test_osnet_pixels_host": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "opd_test_osnet_stem": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 2),
    "opd_test_osnet_gemm": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_int, C.c_void_p] + [C.c_int] * 6),
    "opd_test_osnet_dwconv": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 7),
    "opd_test_osnet_gate": (C.c_int, [C.c_void_p] * 7 + [C.c_int] * 4),
    "opd_test_osnet_avgpool2": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 4),
    "opd_test_osnet_head": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 3),
    "opd_test_reid_kernel_table": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                             C.POINTER(OpdKernelStat), C.c_int, C.POINTER(C.c_int)]),
    # crop-planner hooks (csrc/opd_crop_test_api.cpp): model, boxes, n, H, W, geom, meta, src_off, bx, by, ch, cv, cap
    "opd_test_crop_plan_device": (C.c_int, [C.c_int, C.c_void_p] + [C.c_int] * 3 + [C.c_void_p] * 7 + [C.c_int]),
    "opd_test_crop_plan_host": (C.c_int, [C.c_int, C.c_void_p] + [C.c_int] * 3 + [C.c_void_p] * 7 + [C.c_int]),
    "opd_test_crop_plan_staged": (C.c_int, [C.c_int, C.c_void_p] + [C.c_int] * 3 + [C.c_void_p] * 7 + [C.c_int]),
    # suppression hook (csrc/opd_nms_test_api.cpp): the device kernel's algorithm on the host; dets, counts, n_frames, stride, label, threshold
    "opd_test_nms_plan_host": (C.c_int, [C.POINTER(OpdDet), C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_float]),
    # tiled-detection hooks (csrc/opd_tile_test_api.cpp): opd_detr_merge_tiles's arguments without the handle, on the host; the tile resize kernel
    # alone: frames, n_frames, h, w, tiles_yxhw, n_tiles, oh, ow, out
    "opd_test_tile_merge_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                           C.POINTER(OpdTileParams), C.POINTER(OpdTileDet), C.POINTER(C.c_int32)]),
    "opd_test_tile_resize": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    # ... and the one for tiles of several sizes: frames, n_frames, h, w, tiles_yxhw, n_tiles, tile_HW, H, W, out (the canvas, read first)
    "opd_test_tile_resize_ragged": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    # stage kernels of a tiled call on merged records of the caller (csrc/opd_tile_stages_test_api.cpp): device, frames, n_frames, h, w, merged, counts, S,
    # floor, with_rows, color, floor_out, boxes, foot, has, feat, n_out
    "opd_test_tile_stages": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # the Re-ID stage of a tiled call on merged records of the caller (csrc/opd_tile_reid_test_api.cpp): device, reid, frames, n_frames, h, w, merged, counts, S,
    # slots, slot_map, rec, n_person, geom, rows, boxes, foot, has, feat, n_out
    "opd_test_tile_reid": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 10),
    # optical-flow hook (csrc/opd_flow_test_api.cpp)
    "opd_flow_test_level": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    # floor-map hook (csrc/opd_floor_test_api.cpp)
    "opd_floor_test_tables": (C.c_int, [C.POINTER(OpdFloorConfig), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int)]),
    # tracker hooks (csrc/opd_track_test_api.cpp)
    "opd_track_test_matrices": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "opd_track_test_state": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p]),
    # device, records, n, Q, D, frame, rows_kind, rows, n_rows, slot_map, n_person, slots, capacity, boxes, foot, has, feat, n_out
    "opd_track_test_ingest": (C.c_int, [C.c_int, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5),
    # app, iou, comb [T][N], T, N, hits [T], conf [N], min_hits, high_conf, n_free, then for the kernel and for the host: matches [min(T, N)][2], n_matches, new_dets [N],
    # n_new, unmatched [T], n_unmatched
    "opd_track_test_assoc": (C.c_int, [C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_int] + [C.c_void_p] * 12),
    # the schedule of a streams call: camera_of [F], F, C -> out [capacity] as [steps][C] frame indices (-1: none), *steps.  No device.
    "opd_track_test_streams_schedule": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    # track_assoc_multi_kernel, C cameras in ONE launch, next to the host's associate() per camera: device, C, T [C], N [C], n_free [C], the cameras' app / iou / comb,
    # hits and conf one behind the other, min_hits, high_conf; per side matches, new detections and unmatched tracks at the offsets of max(min(T, N), 1),
    # max(N, 1) and max(T, 1) rows a camera, each with its counts [C]
    "opd_track_test_assoc_multi": (C.c_int, [C.c_int, C.c_int] + [C.c_void_p] * 8 + [C.c_int, C.c_double] + [C.c_void_p] * 12),
    # the same inputs, iters -> mean milliseconds of the kernel and of the host's associate()
    "opd_track_test_bench_assoc": (C.c_int, [C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_int,
                                              C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    # hybrid-tracker hook (csrc/opd_lwt_test_api.cpp): handle, next_xy, status, records, capacity, count
    # the ingest launch of the fused hybrid detect call (csrc/opd_lwt_ingest_test_api.cpp): device, records, n, Q, boxes, n_out
    "opd_lwt_test_ingest": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    # ... and of the fused hybrid TILED call (csrc/opd_lwt_ingest_merged_test_api.cpp): device, merged records, n, S, boxes, n_out
    "opd_lwt_test_ingest_merged": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "opd_test_lwt_interpolate_scripted": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(OpdLwtRec), C.c_int, C.POINTER(C.c_int)]),
}

_lib: Optional[C.CDLL] = None
_lib_has_hooks = False


def load_library(test_hooks: bool = False) -> C.CDLL:
    """dlopen libopd_hip.so (built in-tree by ``csrc/build.py``) and attach prototypes.  Raises if it is missing.

    ``test_hooks=True`` (tests/ and tools/ only; also ``OPD_TEST_HOOKS=1`` in the environment) loads ``libopd_hip_test.so`` instead:
    the same objects plus the ``opd_test_*`` hooks of ``csrc/opd_*test*_api.cpp``.  One process uses ONE of the two (the hooks flip
    process-wide switches of the library they live in), so asking for the hooks after the product library has been loaded raises."""
    global _lib, _lib_has_hooks
    test_hooks = test_hooks or os.environ.get("OPD_TEST_HOOKS") == "1"
    if _lib is not None:
        if test_hooks and not _lib_has_hooks:
            raise RuntimeError("the product library is already loaded in this process; load the test build first "
                               "(_capi.load_library(test_hooks=True) or OPD_TEST_HOOKS=1)")
        return _lib
    path = TEST_LIB_PATH if test_hooks else LIB_PATH
    if not os.path.exists(path):
        raise RuntimeError(
            f"HIP extension not built: {path} is missing (run `python -c 'import __graft_entry__ as g; g.build()'`). "
            "This package has no CPU fallback.")
    lib = C.CDLL(path)
    for table in (API, TEST_API) if test_hooks else (API,):
        for name, (res, args) in table.items():
            fn = getattr(lib, name)  # AttributeError here = the library does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
    _lib, _lib_has_hooks = lib, test_hooks
    return lib


def last_error() -> str:
    return load_library().opd_last_error().decode("utf-8", "replace")


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what} failed (code {rc}): {last_error()}")
