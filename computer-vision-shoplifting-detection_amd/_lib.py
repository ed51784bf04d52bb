"""ctypes binding of include/mi355_yolo.h (libmi355yolo.so).

There is no CPU fallback: if the shared library has not been built (``python -m cvsd_amd.build``)
importing this module's symbols raises, and every engine call needs a visible MI355X.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# MI355_YOLO_LIB: load another build of the same ABI (kernel experiments: tools/ab_build.sh); the product never sets it
LIB_PATH = os.environ.get("MI355_YOLO_LIB") or os.path.join(HERE, "libmi355yolo.so")
MAX_KPT_FLOATS = 51


class Mi355Error(RuntimeError):
    pass


class Opts(C.Structure):
    _fields_ = [("struct_size", C.c_int), ("batch_chunk", C.c_int), ("half", C.c_int), ("fast_act", C.c_int), ("autotune", C.c_int),
                ("streams", C.c_int), ("flags", C.c_int), ("obj_feats", C.c_int), ("plan_dir", C.c_char_p), ("plan_cache_dir", C.c_char_p)]


# mi355_opts.flags (include/mi355_yolo.h)
OPT_NO_FUSE_UPSAMPLE, OPT_NO_FUSE_1X1, OPT_NO_FUSE_TAIL, OPT_NO_GROUPS = 0x01, 0x02, 0x04, 0x08
OPT_NO_MEM_REUSE, OPT_HIP_GRAPH, OPT_NO_DIRECT_ROWS, OPT_NO_PASS_TUNE = 0x10, 0x20, 0x40, 0x80
OPT_NO_SPARSE_BOX = 0x100
# launch-plan files shipped with the package: the tuned choices of the benchmarked workloads on MI355X (plans/README.md)
PLAN_DIR = os.path.join(HERE, "plans")


class Det(C.Structure):
    _fields_ = [("x1", C.c_float), ("y1", C.c_float), ("x2", C.c_float), ("y2", C.c_float), ("conf", C.c_float),
                ("cls", C.c_int), ("anchor_idx", C.c_int), ("kpt", C.c_float * MAX_KPT_FLOATS)]


class ModelInfo(C.Structure):
    _fields_ = [("task", C.c_int), ("nc", C.c_int), ("nkpt", C.c_int), ("kdim", C.c_int), ("reg_max", C.c_int),
                ("n_levels", C.c_int), ("strides", C.c_int * 4), ("n_convs", C.c_int), ("n_ops", C.c_int),
                ("n_buffers", C.c_int), ("n_params", C.c_longlong), ("macs_640", C.c_longlong),
                ("family", C.c_char * 8), ("scale", C.c_char), ("pad_", C.c_char * 7)]


class Timing(C.Structure):
    _fields_ = [("total_ms", C.c_float), ("conv_ms", C.c_float), ("stem_ms", C.c_float), ("pool_ms", C.c_float),
                ("upsample_ms", C.c_float), ("letterbox_ms", C.c_float), ("decode_ms", C.c_float),
                ("nms_ms", C.c_float), ("conv_launches", C.c_int), ("frames", C.c_int)]


class YuvFrame(C.Structure):
    """mi355_yuv_frame: one NV12 / I420 frame by plane pointers (NV12: u = the interleaved UV plane, v = NULL)"""
    _fields_ = [("y", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p), ("height", C.c_int), ("width", C.c_int),
                ("y_stride", C.c_int), ("uv_stride", C.c_int), ("format", C.c_int), ("reserved", C.c_int)]


class TileOpts(C.Structure):
    """mi355_tile_opts: the tile grid (pixels) and the merge of a tiled predict call"""
    _fields_ = [("struct_size", C.c_int), ("tile_h", C.c_int), ("tile_w", C.c_int), ("overlap_y_px", C.c_int), ("overlap_x_px", C.c_int),
                ("full_frame", C.c_int), ("metric", C.c_int), ("thr", C.c_float)]


class MotionOpts(C.Structure):
    """mi355_motion_opts: the block grid and the thresholds of a motion gate"""
    _fields_ = [("struct_size", C.c_int), ("block", C.c_int), ("level", C.c_float), ("min_blocks", C.c_int), ("max_skip", C.c_int)]


class MotionFrame(C.Structure):
    """mi355_motion_frame: one camera's frame of a tick (bytes_per_pixel 3: BGR, 1: a Y plane)"""
    _fields_ = [("data", C.c_void_p), ("height", C.c_int), ("width", C.c_int), ("row_stride", C.c_int), ("bytes_per_pixel", C.c_int)]


class RenderFrame(C.Structure):
    """mi355_render_frame: one BGR source frame of a render call (host memory, or memory of the call's GPU)"""
    _fields_ = [("data", C.c_void_p), ("height", C.c_int), ("width", C.c_int), ("row_stride", C.c_int), ("on_device", C.c_int)]


class RenderOut(C.Structure):
    """mi355_render_out: where the rendered copy of a frame goes"""
    _fields_ = [("data", C.c_void_p), ("row_stride", C.c_int), ("on_device", C.c_int)]


class CropSpec(C.Structure):
    """mi355_crop_spec: the size (0, 0: native), fit and fill of a crop call"""
    _fields_ = [("struct_size", C.c_int), ("height", C.c_int), ("width", C.c_int), ("fit", C.c_int), ("fill", C.c_int)]


class JpegOut(C.Structure):
    """mi355_jpeg_out: host memory for one JPEG stream, and the length the call reports"""
    _fields_ = [("data", C.c_void_p), ("capacity", C.c_int64), ("length", C.c_int64)]


class JpegStream(C.Structure):
    """mi355_jpeg_stream: one JPEG stream in host memory; the call reports where its entropy stage ran"""
    _fields_ = [("data", C.c_void_p), ("length", C.c_int64), ("entropy_used", C.c_int), ("entropy", C.c_int)]


class JpegSyncState(C.Structure):
    """mi355_jpeg_sync_state: the true entry state of one subsequence (entropy="sync")"""
    _fields_ = [("segment", C.c_int), ("byte", C.c_uint32), ("bit", C.c_int), ("j", C.c_int), ("k", C.c_int), ("block", C.c_uint32)]


class JpegSyncStats(C.Structure):
    _fields_ = [("nsub", C.c_int), ("nseq", C.c_int), ("rounds_local", C.c_int), ("rounds_global", C.c_int)]


class JpegStreamInfo(C.Structure):
    """mi355_jpeg_stream_info"""
    _fields_ = [("height", C.c_int), ("width", C.c_int), ("components", C.c_int), ("subsampling", C.c_int), ("restart_interval", C.c_int),
                ("segments", C.c_int), ("blocks", C.c_int64)]


RENDER_WORDS, RENDER_MAX_PRIMS, RENDER_MAX_FRAMES = 8, 16384, 256      # MI355_RENDER_*
JPEG_ENTROPY = {"auto": 0, "gpu": 1, "host": 2, "sync": 3}                       # MI355_JPEG_ENTROPY_*
CROP_FIT = {"stretch": 0, "pad": 1}                                              # MI355_CROP_*
JPEG_420, JPEG_444 = 420, 444           # MI355_JPEG_*
MOTION_MAX_CAMERAS = 64                 # MI355_MOTION_MAX_CAMERAS
TILE_IOS, TILE_IOU = 0, 1               # MI355_TILE_IOS / MI355_TILE_IOU
TILE_MAX_ENTRIES, TILE_MAX_CANDIDATES = 64, 65536
PIX_NV12, PIX_I420 = 1, 2               # MI355_PIX_*
DET_WORDS = C.sizeof(Det) // 4          # 58 32-bit words per row
POSE_F32, POSE_F64 = 0, 1               # MI355_POSE_F32 / MI355_POSE_F64: the element type of a pose array
_P = C.POINTER
_u8p, _f32p, _i32p = _P(C.c_uint8), _P(C.c_float), _P(C.c_int)

# symbol -> (restype, argtypes); every function declared in include/mi355_yolo.h
SIGNATURES = {
    "mi355_last_error": (C.c_char_p, []),
    "mi355_yolo_create": (C.c_int, [C.c_char_p, C.c_int, _P(Opts), _P(C.c_void_p)]),
    "mi355_yolo_create_from_memory": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, _P(Opts), _P(C.c_void_p)]),
    "mi355_yolo_destroy": (None, [C.c_void_p]),
    "mi355_yolo_info": (C.c_int, [C.c_void_p, _P(ModelInfo)]),
    "mi355_yolo_infer": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                   _i32p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, _i32p]),
    "mi355_yolo_infer_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                          _i32p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, _i32p]),
    "mi355_yolo_infer_device_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                                _i32p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mi355_yolo_infer_multi": (C.c_int, [C.c_void_p, C.c_void_p, _i32p, _i32p, _i32p, C.c_int, C.c_int, C.c_float, C.c_float,
                                         _i32p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, _i32p]),
    "mi355_yolo_raw_head_multi": (C.c_int, [C.c_void_p, C.c_void_p, _i32p, _i32p, _i32p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                            _i32p, _i32p]),
    "mi355_yolo_infer_yuv": (C.c_int, [C.c_void_p, _P(YuvFrame), C.c_int, C.c_int, C.c_float, C.c_float, _i32p, C.c_int, C.c_int, C.c_int,
                                       C.c_void_p, C.c_int, _i32p]),
    "mi355_yolo_infer_yuv_device_async": (C.c_int, [C.c_void_p, _P(YuvFrame), C.c_int, C.c_float, C.c_float, _i32p, C.c_int, C.c_int, C.c_int,
                                                    C.c_void_p, C.c_void_p, C.c_void_p]),
    "mi355_op_yuv_to_bgr": (C.c_int, [C.c_int, _P(YuvFrame), C.c_int, _P(C.c_void_p)]),
    "mi355_tile_grid": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, _i32p]),
    "mi355_yolo_infer_tiled": (C.c_int, [C.c_void_p, C.c_void_p, _i32p, _i32p, _i32p, C.c_int, C.c_int, _P(TileOpts), C.c_float, C.c_float,
                                         _i32p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, _i32p, C.c_void_p]),
    "mi355_yolo_infer_tiled_yuv": (C.c_int, [C.c_void_p, _P(YuvFrame), C.c_int, C.c_int, _P(TileOpts), C.c_float, C.c_float, _i32p, C.c_int,
                                             C.c_int, C.c_int, C.c_void_p, C.c_int, _i32p, C.c_void_p]),
    "mi355_op_tile_merge": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    "mi355_yolo_stream": (C.c_void_p, [C.c_void_p]),
    "mi355_yolo_sync": (C.c_int, [C.c_void_p]),
    "mi355_yolo_raw_head": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                      _i32p, _i32p]),
    "mi355_yolo_plan_info": (C.c_int, [C.c_void_p, _P(C.c_ulonglong), _i32p, _i32p, _P(C.c_longlong), _P(C.c_longlong)]),
    "mi355_memory_plan": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P(C.c_longlong),
                                    _P(C.c_longlong), C.c_int, _i32p, _P(C.c_longlong), _P(C.c_longlong)]),
    "mi355_memory_plan_ex": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P(C.c_longlong),
                                       _P(C.c_longlong), C.c_int, _i32p, _P(C.c_longlong), _P(C.c_longlong), _i32p]),
    "mi355_yolo_feat_dim": (C.c_int, [C.c_void_p, _i32p]),
    "mi355_yolo_last_feats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "mi355_op_obj_feats": (C.c_int, [C.c_int, _P(C.c_void_p), _i32p, C.c_int, C.c_int, C.c_int, _i32p, _i32p, C.c_int, C.c_int, C.c_void_p]),
    "mi355_yolo_set_profiling": (C.c_int, [C.c_void_p, C.c_int]),
    "mi355_yolo_last_timing": (C.c_int, [C.c_void_p, _P(Timing)]),
    "mi355_yolo_sparse_stats": (C.c_int, [C.c_void_p, _P(C.c_longlong)]),
    "mi355_op_dwconv2d": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                    C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]),
    "mi355_op_psa_attention": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mi355_op_decode": (C.c_int, [C.c_int, _P(C.c_void_p), _i32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                  C.c_void_p, C.c_void_p, _i32p]),
    "mi355_op_sparse_box": (C.c_int, [C.c_int, _P(C.c_void_p), _i32p, C.c_int, C.c_int, C.c_void_p, C.c_float, _i32p, C.c_int, C.c_int,
                                      C.c_int, C.c_int, C.c_void_p, _i32p]),
    "mi355_op_sppf_pools": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                      C.c_int, C.c_int]),
    "mi355_op_upsample2x": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                      C.c_int]),
    "mi355_op_conv2d": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                  C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, _i32p]),
    "mi355_op_conv2d_f16": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, _i32p]),
    "mi355_op_conv2d_subrange": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                           C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, _i32p, _i32p]),
    "mi355_op_conv1x1_upcat": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_int, C.c_int, C.c_void_p, C.c_int, _i32p]),
    "mi355_op_conv1x1_upcat_f16": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                             C.c_int, C.c_int, C.c_void_p, C.c_int, _i32p]),
    "mi355_op_conv2d_fused": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                        C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, _i32p]),
    "mi355_op_c2f_tail": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                    C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, _i32p]),
    "mi355_op_conv2d_fused_f16": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                            C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, _i32p]),
    "mi355_op_conv2d_group": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                        C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, _i32p, _i32p,
                                        C.c_void_p, C.c_void_p, C.c_int]),
    "mi355_bench_conv2d": (C.c_int, [C.c_int] * 12 + [_f32p, _i32p, C.c_char_p, C.c_int]),
    "mi355_bench_conv2d_f16": (C.c_int, [C.c_int] * 12 + [_f32p, _i32p, C.c_char_p, C.c_int]),
    "mi355_plan_query": (C.c_int, [C.c_int] * 13 + [_i32p, C.c_int, _i32p]),
    "mi355_plan_query_tiles": (C.c_int, [C.c_int] * 13 + [_i32p, C.c_int, _i32p]),
    "mi355_gmc_pyr_lk": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                                   C.c_double, C.c_void_p, C.c_void_p]),
    "mi355_gmc_pyr_lk_device": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_double, C.c_double, C.c_void_p, C.c_void_p]),
    "mi355_gmc_prepare_device": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_double,
                                           C.c_void_p, C.c_void_p, C.c_void_p]),
    "mi355_gmc_order_corners": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mi355_gmc_affine_partial": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_int, C.c_ulonglong, C.c_void_p,
                                           C.c_void_p]),
    "mi355_gmc_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "mi355_gmc_destroy": (None, [C.c_void_p]),
    "mi355_gmc_step_begin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p,
                                       C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double]),
    "mi355_gmc_step_finish": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mi355_gmc_pending_frame": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), _i32p, _i32p]),
    "mi355_tracker_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "mi355_tracker_destroy": (None, [C.c_void_p]),
    "mi355_tracker_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]),
    "mi355_tracker_create_ex": (C.c_int, [C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "mi355_tracker_update_feats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]),
    "mi355_tracker_track_feat": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "mi355_tracker_last_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "mi355_tracker_state": (C.c_int, [C.c_void_p, _i32p, _i32p, _i32p, _i32p]),
    "mi355_tracker_tracks": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "mi355_kalman_initiate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "mi355_kalman_predict": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mi355_kalman_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "mi355_kalman_warp": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "mi355_lapjv": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p]),
    "mi355_gmc_prepare_host": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p,
                                         C.c_void_p]),
    "mi355_gmc_track_begin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "mi355_gmc_track_finish": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mi355_gmc_track_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mi355_gmc_batch_frames": (C.c_int, [C.c_void_p, C.c_ulonglong, C.c_int, C.POINTER(C.c_void_p), _i32p, _i32p, _i32p, C.POINTER(C.c_longlong)]),
    "mi355_gmc_batch_seq": (C.c_ulonglong, [C.c_void_p]),
    "mi355_gmc_track_reset": (C.c_int, [C.c_void_p]),
    "mi355_gmc_track_state": (C.c_int, [C.c_void_p, _i32p, _i32p, _i32p, C.c_void_p, C.c_void_p, C.c_int]),
    "mi355_gmc_multi_create": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "mi355_gmc_multi_destroy": (None, [C.c_void_p]),
    "mi355_gmc_multi_begin": (C.c_int, [C.c_void_p, C.c_void_p, _i32p, _i32p, C.c_int]),
    "mi355_gmc_multi_finish": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mi355_gmc_multi_frames": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mi355_gmc_multi_reset": (C.c_int, [C.c_void_p, C.c_int]),
    "mi355_gmc_multi_state": (C.c_int, [C.c_void_p, C.c_int, _i32p, _i32p, _i32p, C.c_void_p, C.c_void_p, C.c_int]),
    "mi355_op_stem": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                C.c_int, C.c_int, C.c_void_p]),
    "mi355_op_stem_f16": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                    C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mi355_letterbox_shape": (C.c_int, [C.c_int, C.c_int, C.c_int, _i32p, _i32p]),
    "mi355_op_letterbox": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mi355_letterbox_geometry": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _i32p, _P(C.c_double)]),
    "mi355_op_letterbox_multi": (C.c_int, [C.c_int, C.c_void_p, _i32p, _i32p, _i32p, C.c_int, C.c_int, C.c_void_p]),
    "mi355_shopformer_create": (C.c_int, [C.c_char_p, C.c_size_t, C.c_int, _P(C.c_void_p)]),
    "mi355_shopformer_destroy": (None, [C.c_void_p]),
    "mi355_shopformer_info": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mi355_shopformer_score": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mi355_shopformer_score_device_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mi355_shopformer_score_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "mi355_shopformer_score_ex_device_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "mi355_shopformer_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "mi355_shopformer_decode_device_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "mi355_shopformer_decoder_info": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mi355_pose_windows": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mi355_shopformer_score_poses": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "mi355_motion_gate_create": (C.c_int, [C.c_int, C.c_int, _P(MotionOpts), _P(C.c_void_p)]),
    "mi355_motion_gate_destroy": (None, [C.c_void_p]),
    "mi355_motion_gate_update": (C.c_int, [C.c_void_p, _P(_P(MotionFrame)), C.c_int, _i32p, _i32p]),
    "mi355_motion_gate_mask": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, _i32p, _i32p]),
    "mi355_motion_gate_reset": (C.c_int, [C.c_void_p, C.c_int]),
    "mi355_op_motion_grid": (C.c_int, [C.c_int, _P(MotionFrame), C.c_int, C.c_int, _P(C.c_void_p)]),
    "mi355_render": (C.c_int, [C.c_int, _P(RenderFrame), C.c_int, _P(C.c_void_p), _i32p, _P(RenderOut), C.c_void_p, _f32p]),
    "mi355_yolo_render": (C.c_int, [C.c_void_p, _P(RenderFrame), C.c_int, _P(C.c_void_p), _i32p, _P(RenderOut), _f32p]),
    "mi355_yolo_last_frames": (C.c_int, [C.c_void_p, _P(RenderFrame), C.c_int, _i32p]),
    "mi355_crops": (C.c_int, [C.c_int, _P(RenderFrame), C.c_int, _P(C.c_void_p), _i32p, _P(CropSpec), _P(RenderOut), C.c_void_p, _f32p]),
    "mi355_yolo_crops": (C.c_int, [C.c_void_p, _P(RenderFrame), C.c_int, _P(C.c_void_p), _i32p, _P(CropSpec), _P(RenderOut), _f32p]),
    "mi355_jpeg_bound": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "mi355_jpeg_encode": (C.c_int, [C.c_int, _P(RenderFrame), C.c_int, C.c_int, C.c_int, _P(JpegOut), C.c_void_p, _f32p]),
    "mi355_yolo_encode": (C.c_int, [C.c_void_p, _P(RenderFrame), C.c_int, C.c_int, C.c_int, _P(JpegOut), _f32p]),
    "mi355_op_jpeg_coefficients": (C.c_int, [C.c_int, _P(RenderFrame), C.c_int, C.c_int, C.c_int, _P(C.c_void_p)]),
    "mi355_jpeg_info": (C.c_int, [C.c_void_p, C.c_int64, _P(JpegStreamInfo)]),
    "mi355_jpeg_decode": (C.c_int, [C.c_int, _P(JpegStream), C.c_int, C.c_int, _P(RenderOut), _i32p, C.c_void_p, _f32p]),
    "mi355_yolo_decode": (C.c_int, [C.c_void_p, _P(JpegStream), C.c_int, C.c_int, _P(RenderOut), _i32p, _f32p]),
    "mi355_op_jpeg_decode_coefficients": (C.c_int, [C.c_int, _P(JpegStream), C.c_int, C.c_int, _P(C.c_void_p), _i32p]),
    "mi355_op_jpeg_sync": (C.c_int, [C.c_int, _P(JpegStream), C.c_int, C.c_int, C.c_void_p, _i32p, _P(JpegSyncState), C.c_int, _P(JpegSyncStats)]),
    "mi355_op_nms": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, _i32p,
                               C.c_int, C.c_int, C.c_void_p, C.c_int, _i32p]),
    "mi355_op_nms_ex": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, _i32p,
                                  C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p]),
}

_lib = None


def lib() -> C.CDLL:
    """Load libmi355yolo.so (once). Raises Mi355Error if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise Mi355Error(f"{LIB_PATH} is missing: build the HIP extension first "
                             f"(python -m cvsd_amd.build, or __graft_entry__.build()). There is no CPU fallback.")
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = res, args
        _lib = handle
    return _lib


def check(rc: int) -> None:
    if rc != 0:
        msg = lib().mi355_last_error().decode(errors="replace")
        if rc == -2:
            raise FileNotFoundError(msg)
        if rc in (-1, -3):
            raise ValueError(msg)
        raise Mi355Error(f"mi355 error {rc}: {msg}")
