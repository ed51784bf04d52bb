/*
 * mi355_yolo.h -- C ABI of the MI355X-native YOLO detect/pose engine (libmi355yolo.so).
 *
 * This is the drop-in boundary for the ONE hot path of
 * cthadeufaria/computer-vision-shoplifting-detection: the per-frame Ultralytics call made at
 *   /root/reference/model.py:18   self.model = YOLO("./models/yolov5mu.pt")
 *   /root/reference/model.py:38   self.model.track(frame, persist=True, show=False, classes=[0], verbose=False)
 *   /root/reference/model.py:40   results[0].boxes
 * (driven per decoded frame by /root/reference/preprocess.py:38-47).  The arithmetic behind those
 * calls lives in the un-vendored ultralytics==8.3.225 (requirements.txt:121); each entry point below
 * names the Ultralytics function it replaces.  Plain pointers and sizes only: no torch / numpy /
 * C++ types cross this boundary.  The Python facade (cvsd_amd.YOLO) binds it with ctypes; see
 * INTEGRATION.md for the stub a reference maintainer would add.
 *
 * Conventions
 *   - every function returns 0 (MI355_OK) or a negative MI355_E* code; mi355_last_error() returns a
 *     thread-local message for the last failure on the calling thread.
 *   - the caller owns every input/output buffer; the engine owns device memory, its HIP stream and
 *     its weight copies.  One handle = one device = one in-order stream; infer calls on one handle
 *     are NOT re-entrant (the reference is single-threaded; Ultralytics serialises predict with a lock).
 *   - zero detections is not an error: the image's count is 0.
 */
#ifndef MI355_YOLO_H
#define MI355_YOLO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI355_OK            0
#define MI355_EINVAL       -1   /* bad argument (null pointer, non-positive size, capacity too small ...) */
#define MI355_EIO          -2   /* weights file missing / unreadable */
#define MI355_EFORMAT      -3   /* not a .mi355w file, or unsupported version / program */
#define MI355_EHIP         -4   /* a HIP runtime call failed (message has the hipError string) */
#define MI355_ENOMEM       -5

#define MI355_TASK_DETECT   0
#define MI355_TASK_POSE     1
#define MI355_MAX_KPT_FLOATS 51   /* 17 keypoints x (x, y, conf) */

typedef struct mi355_yolo mi355_yolo;   /* opaque engine handle */

/* Engine options; zero-initialise and set struct_size = sizeof(mi355_opts). 0 / NULL means "default".  A caller built against an
 * earlier header (smaller struct_size) keeps working: fields beyond its struct_size take their defaults.
 * Every behaviour-changing knob of the engine is here; the MI355_* environment variables listed in INTEGRATION.md section 5 are
 * A/B overrides for kernel experiments (tools/), not configuration. */
#define MI355_OPT_NO_FUSE_UPSAMPLE  0x01   /* always launch the nearest-2x upsample kernel (never read through the consuming 1x1 conv) */
#define MI355_OPT_NO_FUSE_1X1       0x02   /* never run a Conv3x3 -> Conv1x1 pair as one launch */
#define MI355_OPT_NO_FUSE_TAIL      0x04   /* never run a C2f tail (last Bottleneck conv + C2f.cv2) as one launch */
#define MI355_OPT_NO_GROUPS         0x08   /* no grouped launches / step schedule in the latency-bound regime (<= 5 frames per pass) */
#define MI355_OPT_NO_MEM_REUSE      0x10   /* one region per graph tensor instead of the liveness-shared arena */
#define MI355_OPT_HIP_GRAPH         0x20   /* replay stem..decode of a chunk as a hipGraph (measured slower on ROCm 7.2; off) */
#define MI355_OPT_NO_DIRECT_ROWS    0x40   /* small calls: copy rows to the host instead of writing them from the NMS kernel */
#define MI355_OPT_NO_PASS_TUNE      0x80   /* autotuner: skip the whole-pass re-check of fusion / group decisions */
#define MI355_OPT_NO_SPARSE_BOX     0x100  /* fp32: always compute the head's box branch at every anchor (never at the NMS candidates only) */
typedef struct mi355_opts {
    int struct_size;
    int batch_chunk;      /* frames pushed through the net per pass (default 64); larger batches are looped */
    int half;             /* 1 = Ultralytics' half=True (engine/predictor.py: model.half(), im.half()): activations (the /255
                           * input included) and weights stored as fp16, fp32 accumulate / bias / SiLU, head logits, decode and NMS in fp32.
                           * Results then differ from the fp32 path by fp16 rounding (not a bit-exact mode). */
    int fast_act;         /* fp32 path only. 0 (default): the canonical SiLU x / (1 + exp(-x)) with a reproducible exp and IEEE division --
                           * results are bit-identical to oracle/det_oracle.c.  1: v_exp_f32 / v_rcp_f32 SiLU in the conv epilogues (as the
                           * half path has it): ~1e-6 relative per activation, NOT bit-exact, tolerance-tested against float64. */
    int autotune;         /* candidate launch plans timed per conv when a shape is first seen: 0 = default (32; 28 for half), -1 = off
                           * (the planner's static guess), n > 0 = n */
    int streams;          /* HIP streams the ops of a pass of >= 6 frames are dealt to along the dependency DAG: 0 = default (4), 1 = one */
    int flags;            /* MI355_OPT_* */
    int obj_feats;        /* 1 = every blocking infer call also produces one appearance embedding per kept row, read from the Detect head's
                           * own input maps (Ultralytics' with_reid / model: auto; mi355_yolo_last_feats below).  0 (default): nothing of it
                           * exists -- launches, arena offsets and rows are those of an engine that never heard of it.  Was `reserved`. */
    const char* plan_dir;        /* read-only directory of SHIPPED launch-plan files (cvsd_amd/plans): looked up first, so that every process
                                  * on the same GPU model runs the same launch sequence without timing anything.  NULL = none */
    const char* plan_cache_dir;  /* writable directory where freshly timed choices are kept (and found again): NULL = ~/.cache/mi355yolo,
                                  * "" = do not persist */
} mi355_opts;

/* One post-NMS detection, coordinates in ORIGINAL-image pixels (after scale_boxes / scale_coords).
 * Replaces one row of Results.boxes.data (+ Results.keypoints.data) -- ultralytics/engine/results.py. */
typedef struct mi355_det {
    float x1, y1, x2, y2;
    float conf;
    int   cls;
    int   anchor_idx;                      /* index of the source anchor in [0, A): P3 row-major, then P4, then P5 */
    float kpt[MI355_MAX_KPT_FLOATS];       /* pose only: x, y, conf per keypoint; zeros for detect models */
} mi355_det;

typedef struct mi355_model_info {
    int task;             /* MI355_TASK_* */
    int nc;               /* number of classes */
    int nkpt, kdim;       /* keypoint shape (17, 3) for pose, (0, 0) for detect */
    int reg_max;          /* 16 */
    int n_levels;
    int strides[4];       /* 8, 16, 32 */
    int n_convs, n_ops, n_buffers;
    long long n_params;   /* fused parameter count incl. the 16 DFL weights (what Ultralytics' model.info() prints) */
    long long macs_640;   /* multiply-accumulates of all convs for one 640x640 frame */
    char family[8];       /* "v8" | "v5u" */
    char scale;           /* 'n','s','m','l','x' */
    char pad_[7];
} mi355_model_info;

/* Timing of the last infer call on this handle (HIP events on the engine's own stream). */
typedef struct mi355_timing {
    float total_ms;       /* preprocess .. NMS, device time, whole call */
    float conv_ms;        /* sum over the implicit-GEMM conv launches (the dominant kernel) */
    float stem_ms, pool_ms, upsample_ms, letterbox_ms, decode_ms, nms_ms;
    int   conv_launches;
    int   frames;
} mi355_timing;

const char* mi355_last_error(void);

/* YOLO(path) -- ultralytics/engine/model.py:Model.__init__ + nn/tasks.py load + autobackend fuse.
 * `weights_path` is a .mi355w file (fused weights + op program, written by cvsd_amd.weights). */
int  mi355_yolo_create(const char* weights_path, int device_id, const mi355_opts* opts, mi355_yolo** out);
/* Same, from an in-memory image of the file (what a rank receives from the RCCL weight broadcast). */
int  mi355_yolo_create_from_memory(const void* blob, size_t nbytes, int device_id, const mi355_opts* opts,
                                   mi355_yolo** out);
void mi355_yolo_destroy(mi355_yolo* h);
int  mi355_yolo_info(const mi355_yolo* h, mi355_model_info* info);

/* model(frames, conf=, iou=, classes=, max_det=, imgsz=) -- engine/predictor.py:stream_inference:
 * LetterBox + BGR->RGB + /255 (preprocess), the fused conv graph (nn/tasks.py:_predict_once), Detect/Pose
 * decode (nn/modules/head.py), utils/nms.py:non_max_suppression, utils/ops.py:scale_boxes/scale_coords.
 *   bgr_nhwc           n frames of h x w x 3 uint8, BGR (cv2 layout), HOST memory; consecutive rows are
 *                      row_stride_bytes apart (0 = w*3) and consecutive frames h*row_stride_bytes apart
 *   conf, iou          thresholds (Ultralytics predict defaults 0.25 / 0.7; .track() uses conf 0.1)
 *   classes,n_classes  keep only detections whose best class is listed (NULL / 0 = all)   [classes=[0] at model.py:38]
 *   max_det            at most this many rows per image (default 300)
 *   imgsz              letterbox target (default 640; rectangular "auto" padding to a multiple of 32)
 *   out_rows           [n * out_capacity_per_image] rows, image i at out_rows + i*out_capacity_per_image,
 *                      confidence-descending (the NMS keep order)
 *   out_counts         [n] rows written per image
 */
int  mi355_yolo_infer(mi355_yolo* h, const uint8_t* bgr_nhwc, int n, int height, int width, int row_stride_bytes,
                      float conf, float iou, const int* classes, int n_classes, int max_det, int imgsz,
                      mi355_det* out_rows, int out_capacity_per_image, int* out_counts);
/* One call over n frames that need not share a size (several cameras at different resolutions) -- BasePredictor.pre_transform:
 * when every frame has the same (h, w) the rect letterbox of mi355_yolo_infer is used (same rows as that call on the stacked
 * frames); otherwise every frame is letterboxed to the square imgsz x imgsz canvas (LetterBox auto=False) and its rows are scaled
 * back against its own shape (utils/ops.py:scale_boxes / scale_coords).
 *   frames[i]          frame i, heights[i] x widths[i] x 3 uint8 BGR; rows row_strides[i] bytes apart (row_strides NULL or
 *                      row_strides[i] == 0: widths[i]*3).  frames_on_device = 0: HOST memory (packed chunk by chunk into pinned
 *                      staging, one host-to-device copy per chunk); 1: memory of the engine's device.
 *   other arguments    as mi355_yolo_infer; out_rows / out_counts in frame order. */
int  mi355_yolo_infer_multi(mi355_yolo* h, const uint8_t* const* frames, const int* heights, const int* widths,
                            const int* row_strides, int frames_on_device, int n, float conf, float iou, const int* classes,
                            int n_classes, int max_det, int imgsz, mi355_det* out_rows, int out_capacity_per_image,
                            int* out_counts);
/* Same with the frames already resident in DEVICE memory (dense n x h x w x 3); outputs still go to host. */
int  mi355_yolo_infer_device(mi355_yolo* h, const uint8_t* bgr_nhwc_dev, int n, int height, int width,
                             float conf, float iou, const int* classes, int n_classes, int max_det, int imgsz,
                             mi355_det* out_rows, int out_capacity_per_image, int* out_counts);

/* Asynchronous device-output form (multi-GPU pipelines: the per-rank rows are gathered over RCCL straight from HBM while the
 * next batch computes; replaces the reference's per-frame `results[0].boxes` hand-over, model.py:40, for a whole shard).
 * Frames AND outputs live in DEVICE memory owned by the caller; nothing crosses PCIe and the call returns as soon as the work
 * is enqueued on the engine's stream:
 *   rows_dev    [n * max_det] rows, PACKED in frame order: frame 0's counts[0] rows, then frame 1's, ...
 *   counts_dev  [n] rows kept per frame;   total_dev [1] = sum(counts) = number of valid packed rows
 * The buffers are valid once the stream has passed this call: wait with mi355_yolo_sync(), or order another HIP stream
 * behind mi355_yolo_stream() (a hipStream_t; e.g. torch.cuda.ExternalStream).  The next infer call on the handle waits for
 * a pending asynchronous one before it reuses the engine's scratch, so callers double-buffer the output buffers only. */
int  mi355_yolo_infer_device_async(mi355_yolo* h, const uint8_t* bgr_nhwc_dev, int n, int height, int width,
                                   float conf, float iou, const int* classes, int n_classes, int max_det, int imgsz,
                                   mi355_det* rows_dev, int* counts_dev, int* total_dev);
void* mi355_yolo_stream(mi355_yolo* h);
int  mi355_yolo_sync(mi355_yolo* h);

/* ---- 4:2:0 YUV frames, as video decoders emit them -----------------------------------------------------------
 * NV12 and I420 frames are converted to BGR on the GPU, by one launch per chunk in front of the letterbox / stem, into the dense BGR
 * staging buffer those kernels already read: every later kernel runs unchanged, on the bytes cv2.cvtColor with COLOR_YUV2BGR_NV12 /
 * COLOR_YUV2BGR_I420 would have handed to mi355_yolo_infer (BT.601 limited range, 20-bit fixed point, one chroma sample per 2x2 block
 * of Y, no chroma interpolation):
 *     uu = U - 128;  vv = V - 128;  yy = max(0, Y - 16) * 1220542
 *     R = sat_u8((yy + (1 << 19) + 1673527 * vv) >> 20)
 *     G = sat_u8((yy + (1 << 19) - 852492 * vv - 409993 * uu) >> 20)          (>> arithmetic: floor for negative sums)
 *     B = sat_u8((yy + (1 << 19) + 2116026 * uu) >> 20)
 * A frame is three plane pointers: decoders pad rows and do not keep planes adjacent.
 *   y           [height][y_stride] bytes
 *   u, v        NV12: u = the interleaved plane [height/2][uv_stride] holding U,V,U,V..., v = NULL (not read)
 *               I420: u and v = separate planes [height/2][uv_stride], width/2 samples each
 *   height, width    even and positive;  y_stride >= width;  uv_stride >= width (NV12), >= width/2 (I420); strides in bytes
 *   format      MI355_PIX_NV12 or MI355_PIX_I420;  reserved = 0
 * Every entry point below checks all frames before anything runs and refuses with MI355_EINVAL (the message names the field): a null
 * y or u, a null v of an I420 frame, an odd or non-positive height or width, a stride smaller than its row, an unknown format.
 * A frame whose width is a multiple of 16 and whose plane bases and strides are multiples of 16 bytes (8 for I420 chroma) is converted
 * 16 pixels x 2 rows per lane with 16-byte accesses (every real video size); any other frame one 2x2 block per lane, by bytes. */
#define MI355_PIX_NV12 1
#define MI355_PIX_I420 2
typedef struct mi355_yuv_frame {
    const uint8_t* y; const uint8_t* u; const uint8_t* v;   /* NV12: u = the interleaved UV plane, v = NULL */
    int height, width, y_stride, uv_stride, format, reserved;
} mi355_yuv_frame;
/* mi355_yolo_infer_multi on YUV frames: n frames that need not share a size or a format.  All frames the same (h, w): the rect
 * letterbox, the rows are those of mi355_yolo_infer on the converted stack; otherwise the square canvas with per-frame scale-back.
 *   frames_on_device = 0   the planes are HOST memory: packed row by row (padding is not uploaded) into pinned staging, one
 *                          host-to-device copy per chunk on the copy stream while the previous chunk's kernels run -- 1.5 bytes per
 *                          pixel instead of the 3 of a BGR frame
 *   frames_on_device = 1   the planes are memory of the engine's device (a decoder's surfaces), converted from where they are
 *   other arguments        as mi355_yolo_infer; the conversion's time is part of mi355_timing.letterbox_ms */
int  mi355_yolo_infer_yuv(mi355_yolo* h, const mi355_yuv_frame* frames, int frames_on_device, int n, float conf, float iou,
                          const int* classes, int n_classes, int max_det, int imgsz,
                          mi355_det* out_rows, int out_capacity_per_image, int* out_counts);
/* mi355_yolo_infer_device_async on YUV frames: planes in DEVICE memory, all n frames the same (h, w) (formats may differ); nothing
 * crosses PCIe except the n frame descriptors, and the call returns once the work is enqueued. */
int  mi355_yolo_infer_yuv_device_async(mi355_yolo* h, const mi355_yuv_frame* frames, int n, float conf, float iou,
                                       const int* classes, int n_classes, int max_det, int imgsz,
                                       mi355_det* rows_dev, int* counts_dev, int* total_dev);
/* The conversion alone, for parity tests: planes and outputs are HOST memory, bgr_out[i] = dense height_i * width_i * 3 bytes.
 * device_id >= 0 runs the kernel on planes uploaded with the caller's strides and base alignment (modulo 16), so a frame takes the
 * path it would take in place; the device copy of every output is followed by guard bytes, and the call fails with MI355_EHIP when
 * the launch changed one.  device_id = -1 runs the same per-block routine in a host loop and touches no GPU. */
int  mi355_op_yuv_to_bgr(int device_id, const mi355_yuv_frame* frames, int n, uint8_t* const* bgr_out);

/* ---- tiled predict for high-resolution frames --------------------------------------------------------------------
 * A frame is cut into overlapping tiles, every tile (and, with full_frame, the frame itself) runs through ONE detector pass as an entry
 * of the mixed-shape call above, and the per-entry rows are merged per frame on the GPU; only the merged rows come back.
 *
 * Tile grid, pure integer arithmetic.  Along an axis of length L with tile t and overlap o pixels (0 <= o < t): positions start at
 * p_0 = 0 and advance by t - o; a position is kept while p + t < L; the first position with p + t >= L is the last one and is replaced
 * by max(0, L - t); every tile's extent on that axis is min(t, L).  Tiles are listed row-major (y outer, x inner).
 *   mi355_tile_grid   host only.  out_xywh[4 * i ..] = x, y, w, h of tile i (out_xywh may be NULL to query *count); cap counts tiles;
 *                     MI355_EINVAL: a non-positive size, an overlap outside [0, tile), more tiles than cap.
 *
 * Entry list of a call: for each frame in order its tiles, then the frame itself when full_frame is set: E = T + 1 (or T) entries per
 * frame.  The concatenated list is treated exactly as mi355_yolo_infer_multi treats n frames: all entries of one shape -> the rect
 * canvas, otherwise the square one; every entry has its own NMS (conf, iou, classes, max_det) and is scaled back to its own pixels.
 *
 * Merge, per source frame, fp32 (FP contraction off).  Candidates: every kept row of the frame's entries.  Row r of entry e with origin
 * (ox, oy) (the full frame: (0, 0)) is shifted: x1 + (float)ox, y1 + (float)oy, x2 + (float)ox, y2 + (float)oy, and with kdim >= 2 each
 * keypoint's x and y likewise (one fp32 add each); keypoint confidence, conf, cls and anchor_idx pass through as bits.  Order: ascending
 * key (~conf_bits << 32) | (e * max_det + r), i.e. descending conf, ties by ascending slot.  Greedy in that order: a candidate dies iff
 * an earlier KEPT candidate of the same cls has metric > thr, with w = max(0, min(x2) - max(x1)), h likewise, inter = w * h (rounded to
 * fp32), area = (x2 - x1) * (y2 - y1) on the shifted coordinates,
 *   MI355_TILE_IOS   inter / min(area_i, area_j)        (min(a, b) = a < b ? a : b)
 *   MI355_TILE_IOU   inter / (area_i + area_j - inter)
 * 0 / 0 is NaN and NaN > thr is false: a zero-area box neither suppresses nor is suppressed.  The merge stops after max_det kept rows.
 * Capacity of the merge kernel: E <= MI355_TILE_MAX_ENTRIES entries per frame and E * max_det <= MI355_TILE_MAX_CANDIDATES candidates
 * per frame; beyond either the calls below refuse with MI355_EINVAL before any launch.
 *
 *   mi355_yolo_infer_tiled   frames / heights / widths / row_strides / frames_on_device / n and conf .. imgsz as mi355_yolo_infer_multi.
 *        HOST frames are uploaded ONCE each, ahead of the first chunk, into a device buffer of the engine (rows width * 3 apart); the
 *        entries are descriptors into that copy -- or into the caller's device frames -- (pointer offset + the parent's row stride),
 *        nothing else is copied.  The entry rows stay on the device; ONE merge launch behind the last chunk's NMS.
 *        out_rows [n][cap] merged rows in frame pixels, kept order; anchor_idx = the anchor within the entry's own canvas;
 *        out_counts [n]; out_tile_idx [n][cap] (or NULL) = entry index of every row within its frame (T = the full frame).
 *        An engine with obj_feats runs the call unchanged and produces no features for it.
 *   mi355_yolo_infer_tiled_yuv   the same on NV12 / I420 frames: all n frames are converted first (one launch) into the engine's dense
 *        BGR buffer, which the tiles are then cut from.
 *   mi355_op_tile_merge   the merge alone (parity tests): rows [n_frames][entries][max_det] (58 words each), counts [n_frames][entries],
 *        origins [n_frames][entries][2] = ox, oy; kdim 0, 2 or 3: floats j < (51 / kdim) * kdim of kpt[] are keypoints.  out_rows
 *        [n_frames][max_det], out_counts [n_frames], out_tile_idx [n_frames][max_det]; slots at or beyond the count keep the caller's
 *        bits.  Host memory in and out.  device = -1 runs the same per-frame routine on the host and touches no GPU. */
#define MI355_TILE_IOS 0
#define MI355_TILE_IOU 1
#define MI355_TILE_MAX_ENTRIES 64
#define MI355_TILE_MAX_CANDIDATES 65536
typedef struct mi355_tile_opts {
    int struct_size;                    /* sizeof(mi355_tile_opts) */
    int tile_h, tile_w;                 /* >= 32 */
    int overlap_y_px, overlap_x_px;     /* 0 <= overlap < tile */
    int full_frame;                     /* 1: the frame itself is the last entry of its list */
    int metric;                         /* MI355_TILE_IOS / MI355_TILE_IOU */
    float thr;                          /* in [0, 1] */
} mi355_tile_opts;
int  mi355_tile_grid(int height, int width, int tile_h, int tile_w, int overlap_y_px, int overlap_x_px, int* out_xywh, int cap, int* count);
int  mi355_yolo_infer_tiled(mi355_yolo* h, const uint8_t* const* frames, const int* heights, const int* widths, const int* row_strides,
                            int frames_on_device, int n, const mi355_tile_opts* tile, float conf, float iou, const int* classes,
                            int n_classes, int max_det, int imgsz, mi355_det* out_rows, int cap, int* out_counts, int* out_tile_idx);
int  mi355_yolo_infer_tiled_yuv(mi355_yolo* h, const mi355_yuv_frame* frames, int frames_on_device, int n, const mi355_tile_opts* tile,
                                float conf, float iou, const int* classes, int n_classes, int max_det, int imgsz, mi355_det* out_rows,
                                int cap, int* out_counts, int* out_tile_idx);
int  mi355_op_tile_merge(int device, const mi355_det* rows, const int* counts, const int* origins, int n_frames, int entries, int max_det,
                         int kdim, int metric, float thr, mi355_det* out_rows, int* out_counts, int* out_tile_idx);

/* The decoded pre-NMS head tensor, exactly the layout Detect/Pose.forward returns: out[n][4+nc+nk][A] fp32
 * (xywh in letterboxed pixels, sigmoid class scores, decoded keypoints).  For parity tests.
 * out may be NULL to query *out_channels / *out_anchors for the given frame size. */
int  mi355_yolo_raw_head(mi355_yolo* h, const uint8_t* bgr_nhwc, int n, int height, int width, int row_stride_bytes,
                         int imgsz, float* out, int* out_channels, int* out_anchors);

/* mi355_yolo_raw_head for the frames of mi355_yolo_infer_multi: out[n][4+nc+nk][A] with A the anchors of the canvas (imgsz x imgsz
 * for frames of different sizes).  out may be NULL to query *out_channels / *out_anchors. */
int  mi355_yolo_raw_head_multi(mi355_yolo* h, const uint8_t* const* frames, const int* heights, const int* widths,
                               const int* row_strides, int frames_on_device, int n, int imgsz, float* out, int* out_channels,
                               int* out_anchors);

/* ---- object features: the detector's own appearance embedding per kept row -----------------------------------------
 * DetectionPredictor.get_obj_feats (ultralytics/engine/predictor.py, fed by a forward pre-hook on Detect; botsort.yaml with_reid: True,
 * model: auto): with C_l the channels of the three Detect inputs and s = min(C_l), a row whose anchor a lies on level l (g = C_l / s) gets
 *     e[j] = mean(x_l[a, j*g .. j*g + g - 1]),  j = 0 .. s-1
 * in fp32: acc = x[0]; acc += x[r] for ascending r; e = acc / (float)g, IEEE division (g = 1 copies the bits); with half = 1 the stored
 * fp16 values are widened to fp32 first.  An engine created with mi355_opts.obj_feats = 1 keeps the three maps alive until the chunk's
 * NMS has run (they share arena bytes with no other buffer) and enqueues ONE gather launch per chunk behind NMS.  Creation fails with
 * MI355_EFORMAT when the program's three Detect-input slices cannot be found, or their channel counts are not multiples of the smallest.
 *   mi355_yolo_feat_dim     *dim = s, or 0 when the option is off
 *   mi355_yolo_last_feats   out[n][capacity_per_image][dim] float32, parallel to out_rows of the LAST blocking infer call on the handle
 *                           (mi355_yolo_infer, _infer_device, _infer_multi, _infer_yuv): row r of image i belongs to out_rows row r of image i;
 *                           rows at or beyond that call's out_counts[i] are not written.  n must be that call's n.  MI355_EINVAL when the
 *                           last call produced none: the option is off, no call yet, the call failed, or it was one of the *_device_async
 *                           forms -- those run unchanged and produce no features. */
int  mi355_yolo_feat_dim(const mi355_yolo* h, int* dim);
int  mi355_yolo_last_feats(const mi355_yolo* h, float* out, int capacity_per_image, int n);

/* Launch plans of the shape last run: plan_hash identifies the candidate lists AND the choice per conv (two runs with the same
 * hash launch the same kernels with the same grids); source 0 = static guess (autotune off), 1 = this process's memory,
 * 2 = this machine's plan cache, 3 = timed now, 4 = shipped plan file (opts.plan_dir); launches = kernel launches of one pass (stem .. last conv; decode and NMS follow);
 * activation_bytes = device memory held by the activation arena (buffers whose lifetimes cannot overlap under any legal
 * schedule share bytes), activation_bytes_unshared = what one region per graph tensor would take.  Any out pointer may be NULL. */
int  mi355_yolo_plan_info(const mi355_yolo* h, unsigned long long* plan_hash, int* source, int* launches,
                          long long* activation_bytes, long long* activation_bytes_unshared);
/* Host-only: where the activation buffers of a weight image would live for n frames of height x width per pass (byte offsets
 * into the engine's arena and sizes, per program buffer, in .mi355w buffer order) -- the liveness-based placement the engine
 * uses, computed without a device.  reuse = 0: one region per buffer.  For the memory planner's unit tests. */
int  mi355_memory_plan(const void* blob, size_t nbytes, int n, int height, int width, int imgsz, int half, int reuse,
                       long long* offsets, long long* sizes, int cap, int* n_buffers, long long* arena_bytes,
                       long long* unshared_bytes);
/* The same with the option mi355_opts.obj_feats: 1 places the three Detect-input buffers on bytes of their own; detect_bufs (or NULL)
 * receives their program buffer indices, one per head level.  obj_feats = 0 gives exactly mi355_memory_plan's results. */
int  mi355_memory_plan_ex(const void* blob, size_t nbytes, int n, int height, int width, int imgsz, int half, int reuse, int obj_feats,
                          long long* offsets, long long* sizes, int cap, int* n_buffers, long long* arena_bytes,
                          long long* unshared_bytes, int* detect_bufs);
/* Per-kernel-kind timing costs two HIP events per launch; off by default (total_ms is always measured). */
int  mi355_yolo_set_profiling(mi355_yolo* h, int on);
int  mi355_yolo_last_timing(const mi355_yolo* h, mi355_timing* t);
/* Statistics of the sparse box branch (waits for the engine's stream): out[0] = 1 when the current shape runs it (else minus the reason: 1 no such head / half / switched off, 2 below the
 * frames-per-pass threshold or hipGraph, 3 / 4 the shape's tuned plan of cv2.i.1 / cv2.i.0 is not a kernel the gated dense fall-back exists for), out[1] = passes that
 * enqueued it so far, out[2] = those in which a position list overflowed and the dense box branch ran instead, out[3..5] / out[6..8] =
 * dilated / candidate positions per head level in the last pass, out[9] = that pass's overflow flag. */
int  mi355_yolo_sparse_stats(mi355_yolo* h, long long* out10);

/* ---- single-operator entry points (host pointers; used by the parity tests to isolate a kernel) -------- */

/* Fused conv + bias (+SiLU) (+residual), NHWC fp32 -- ultralytics/nn/modules/conv.py:Conv.forward_fuse.
 * x[n][h][w][cin] dense, w_oihw[cout][cin][k][k], bias[cout], residual (or NULL) and y dense [n][ho][wo][cout];
 * k in {1,3}, stride in {1,2}, pad = k/2.  plan_index selects one of the engine's candidate launch plans (tile shape,
 * wave arrangement, v1 / v2 staging; 0 = the default guess, taken modulo the number of candidates, which is returned
 * through n_plans when non-NULL): every plan must give the same bits. */
int  mi355_op_conv2d(int device_id, const float* x, int n, int h, int w, int cin, const float* w_oihw,
                     const float* bias, int cout, int k, int stride, int silu, const float* residual, float* y,
                     int plan_index, int* n_plans);
/* The 3x3 / stride 1 fp32 operator launched over the cout tiles [t0, last] of its conv alone (tiles of 16 couts, 0 < t0 < tiles): the way
 * the engine launches the class couts of a merged cv2.i.0 + cv3.i.0 head conv in a pass that runs the sparse box branch.  The
 * candidate plans are those the planner offers when told the sub-range's length.  y[n][h][w][cout] comes in filled by the caller: couts
 * >= 16 * t0 are overwritten and must equal mi355_op_conv2d's, bit for bit, for every plan_index; couts < 16 * t0 must come back as they
 * were.  tile (or NULL) receives the MI355_PLAN_TILE_FIELDS ints of the launch that ran (see mi355_plan_query_tiles). */
int  mi355_op_conv2d_subrange(int device_id, const float* x, int n, int h, int w, int cin, const float* w_oihw, const float* bias,
                              int cout, int silu, int t0, float* y, int plan_index, int* n_plans, int* tile);
/* The same operator on the half=True path: x, w and residual are rounded to fp16 (nearest-even) on the way in, the
 * kernel accumulates in fp32 and rounds y to fp16 once (out_f32 = 1: y is written as fp32, as for the head's final
 * convs); y is handed back as fp32 values. */
int  mi355_op_conv2d_f16(int device_id, const float* x, int n, int h, int w, int cin, const float* w_oihw,
                         const float* bias, int cout, int k, int stride, int silu, const float* residual, float* y,
                         int out_f32, int plan_index, int* n_plans);
/* Pointwise conv over the channel concatenation of a nearest-2x upsampled half-resolution tensor and a full-resolution one, with the
 * upsample fused into the conv's read side, as the engine runs the neck's Upsample -> Concat -> C2f.cv1 (fp32; ultralytics
 * nn/modules: nn.Upsample(None, 2, "nearest"), Concat, C2f.cv1): x_half[n][h/2][w/2][up_c] (up_c a multiple of 16),
 * x_skip[n][h][w][skip_c], w[cout][up_c + skip_c][1][1] -> y[n][h][w][cout].  Must equal mi355_op_conv2d on the materialised
 * concatenation, bit for bit, for every plan_index. */
int  mi355_op_conv1x1_upcat(int device_id, const float* x_half, const float* x_skip, int n, int h, int w, int up_c, int skip_c,
                            const float* w_oihw, const float* bias, int cout, int silu, float* y, int plan_index, int* n_plans);
/* The same on the half=True path (operands rounded to fp16 on the way in, fp32 accumulation, y rounded to fp16 once): must equal
 * mi355_op_conv2d_f16 on the materialised concatenation, bit for bit, for every plan_index. */
int  mi355_op_conv1x1_upcat_f16(int device_id, const float* x_half, const float* x_skip, int n, int h, int w, int up_c, int skip_c,
                                const float* w_oihw, const float* bias, int cout, int silu, float* y, int plan_index, int* n_plans);
/* Conv3x3 (stride 1|2, pad 1) + bias + SiLU -> Conv1x1 + bias (+SiLU if silu2) run as ONE fused launch, the way the engine runs
 * a 3x3 conv whose only reader is a pointwise conv (the first conv's output never leaves the chip).  x[n][h][w][cin],
 * w1[c1][cin][3][3], b1[c1], w2[c2][c1][1][1], b2[c2] -> y[n][h/stride][w/stride][c2]; must equal the two convs run separately,
 * bit for bit, for every plan_index. */
int  mi355_op_conv2d_fused(int device_id, const float* x, int n, int h, int w, int cin, const float* w1_oihw, const float* b1,
                           int c1, int stride, const float* w2_oihw, const float* b2, int c2, int silu2, float* y,
                           int plan_index, int* n_plans);
/* The tail of a C2f block as ONE fused launch (fp32): the last Bottleneck's second conv, y1 = SiLU(conv3x3(x) + b1) + residual,
 * and C2f.cv2 over the concatenation, y = SiLU(conv1x1(cat(lead, y1)) + b2) -- lead[n][h][w][lead_c] are the earlier slices of
 * the block's concat buffer (lead_c a multiple of 16, as is c1), w2[c2][lead_c + c1][1][1]; residual (or NULL) [n][h][w][c1].
 * Must equal mi355_op_conv2d (3x3, residual) followed by mi355_op_conv2d (1x1 on the concatenation), bit for bit, for every plan. */
int  mi355_op_c2f_tail(int device_id, const float* x, int n, int h, int w, int cin, const float* w1_oihw, const float* b1, int c1,
                       const float* residual, const float* lead, int lead_c, const float* w2_oihw, const float* b2, int c2,
                       float* y, int plan_index, int* n_plans);
/* The same fused pair on the half=True path (operands rounded to fp16 on the way in, the intermediate image rounded to fp16 as the
 * unfused launch would have stored it, fp32 accumulation; out_f32 = 1: y written as fp32, as for the head's final convs): must
 * equal mi355_op_conv2d_f16 of the 3x3 conv followed by mi355_op_conv2d_f16 of the 1x1, bit for bit, for every plan_index. */
int  mi355_op_conv2d_fused_f16(int device_id, const float* x, int n, int h, int w, int cin, const float* w1_oihw, const float* b1,
                               int c1, int stride, const float* w2_oihw, const float* b2, int c2, int silu2, float* y, int out_f32,
                               int plan_index, int* n_plans);
/* Two independent convs of one input x[n][h][w][cin] (weights wa / wb, SiLU, no residual) as ONE grouped launch -- the way the
 * engine runs independent convs of one step of the op DAG in the latency-bound regime (the head branches beside the neck).
 * plan_a / plan_b pick among each conv's candidate plans whose kernel instance is on the group kernel's menu (their counts come
 * back through n_menu_a / n_menu_b); ya / yb must equal mi355_op_conv2d of each conv alone, bit for bit, for every pair.
 * cout2_a > 0: conv a is a 3x3 conv with a pointwise conv w2a[cout2_a][cout_a][1][1] / b2a (no activation) fused behind it, as in
 * mi355_op_conv2d_fused, and ya holds that pointwise conv's output [n][h/stride_a][w/stride_a][cout2_a]. */
int  mi355_op_conv2d_group(int device_id, const float* x, int n, int h, int w, int cin, const float* wa, const float* ba,
                           int cout_a, int k_a, int stride_a, const float* wb, const float* bb, int cout_b, int k_b,
                           int stride_b, float* ya, float* yb, int plan_a, int plan_b, int* n_menu_a, int* n_menu_b,
                           const float* w2a, const float* b2a, int cout2_a);
/* Device-resident timing of one conv launch plan on random data (diagnostics / tuning): average milliseconds over
 * `iters` back-to-back launches of candidate plan `plan_index`; plan_desc (optional) receives a description. */
int  mi355_bench_conv2d(int device_id, int n, int h, int w, int cin, int cout, int k, int stride, int silu, int residual,
                        int plan_index, int iters, float* avg_ms, int* n_plans, char* plan_desc, int plan_desc_len);
int  mi355_bench_conv2d_f16(int device_id, int n, int h, int w, int cin, int cout, int k, int stride, int silu,
                            int residual, int plan_index, int iters, float* avg_ms, int* n_plans, char* plan_desc,
                            int plan_desc_len);
/* Host-only query of the launch planner (nothing is launched or allocated): the kernel version of every candidate launch
 * plan for a conv of this shape over buffers with these pixel strides (elements); versions[i] = 1 conv_igemm (LDS-staged),
 * 3 streaming pointwise, 4 pipelined pointwise, 6 split-K, + 100 when the plan carries the fused pointwise stage
 * (f2_cout > 0).  res_cs = 0: no residual.  For the planner's unit tests (address-range guards). */
int  mi355_plan_query(int n, int h, int w, int cin, int cout, int k, int stride, int src_cs, int dst_cs, int res_cs,
                      int f2_cout, int f2_dst_cs, int half, int* versions, int cap, int* n_plans);
/* The same query with every candidate's launch geometry: tiles[9 * i ..] = version (as above), PT (pixel tiles of 16 per wave), CT
 * (cout tiles per wave), WP (waves along pixels), TW, TH (output tile), G (cout groups a wave walks), grid.x, grid.y.  A block of
 * the LDS-staged kernels covers WP * PT * 16 pixels.  cap counts candidates (9 ints each). */
#define MI355_PLAN_TILE_FIELDS 9
int  mi355_plan_query_tiles(int n, int h, int w, int cin, int cout, int k, int stride, int src_cs, int dst_cs, int res_cs,
                            int f2_cout, int f2_dst_cs, int half, int* tiles, int cap, int* n_plans);
/* HOST computation (no GPU): pyramidal Lucas-Kanade optical flow of n points between two gray uint8 frames [height][width] --
 * the cv2.calcOpticalFlowPyrLK step of BoT-SORT's global motion compensation (ultralytics/trackers/utils/gmc.py, reached
 * from /root/reference/model.py:38).  win x win windows (odd), max_level + 1 pyramid levels, at most max_iters iterations or
 * |step| <= eps, points whose window's minimum eigenvalue is below min_eig or which leave the frame get status 0.
 * pts / next_pts: [n][2] (x, y).  Returns 0, or -1 on a bad argument. */
int  mi355_gmc_pyr_lk(const uint8_t* prev, const uint8_t* cur, int height, int width, const float* pts, int n, int win,
                      int max_level, int max_iters, double eps, double min_eig, float* next_pts, uint8_t* status);
/* The same on GPU `device` (csrc/gmc_kernels.hip: one wavefront per point, float64, pyramids built on the GPU; host buffers in and
 * out).  On the host the 1000-corner budget costs 10-27 ms per frame -- thirty times the detector pass -- so model.track() hands
 * its tracker the engine's device.  Results agree with the host routine to rounding (window sums are associated differently).
 * win <= 21 (the default window) and a pyramid of at most 8 planes: a plane and max_level for which the host routine builds more (more
 * than 7 halvings that stay larger than the window) are a bad argument.  Returns 0, -1 (bad argument) or -2 (HIP error). */
int  mi355_gmc_pyr_lk_device(int device, const uint8_t* prev, const uint8_t* cur, int height, int width, const float* pts, int n, int win,
                             int max_level, int max_iters, double eps, double min_eig, float* next_pts, uint8_t* status);
/* Frame preparation of the same motion compensation on GPU `device`: BGR frame -> gray plane of oh x ow (cv2.cvtColor(BGR2GRAY) +
 * cv2.resize(INTER_LINEAR) in their fixed-point arithmetic; xtab / ytab = per output column / row {source index, tap 0, tap 1} with
 * 11-bit taps, unused when oh x ow is the frame size), the float32 min-eigenvalue map of cv2.goodFeaturesToTrack (3x3 Sobel, 3x3
 * block) and the 0/1 mask of the corners it keeps (quality threshold against the map's maximum, 3x3 non-maximum suppression,
 * border excluded); the caller orders the kept corners by strength.  Host buffers in and out.  0, -1 (bad argument), -2 (HIP error). */
int  mi355_gmc_prepare_device(int device, const uint8_t* bgr, int height, int width, int oh, int ow, const int* xtab, const int* ytab,
                              double quality, uint8_t* gray_out, float* eig_out, uint8_t* ok_out);
/* One motion-compensation step as two calls, so that it runs BESIDE the detector pass on a stream of its own: model.track() enqueues
 * the step for a frame before the detector runs on it and collects it when the tracker asks for the warp.  The object keeps the
 * previous frame's pyramid on the device.  step_begin = mi355_gmc_prepare_device of `bgr` plus, when n_prev > 0, Lucas-Kanade tracking
 * of prev_pts from the previous step's plane into this one (that step must have prepared a plane of the same oh x ow); it returns at
 * once and reads nothing of its arguments afterwards.  step_finish waits and fills gray / eig / ok [oh * ow] and, when the step had
 * points, next_pts [n_prev][2] and status [n_prev].  One step may be pending per object.  0, -1 (bad argument / order), -2 (HIP). */
/* The two small host stages behind the GPU step, as gmc.py states them in numpy: goodFeaturesToTrack's ordering of the kept corners
 * (strongest first, raster order among equals, at most max_corners; returns the count written to xy_out [max_corners][2]) and
 * cv2.estimateAffinePartial2D (RANSAC over 2-point similarities + refit; src / dst float64 [n][2]; returns 1 and fills H_out [6] and
 * inliers_out [n] (may be NULL), 0 when no transform was found, -1 on bad arguments; draws from its own seeded generator). */
int  mi355_gmc_order_corners(const float* eig, const uint8_t* ok, int height, int width, int max_corners, float* xy_out);
int  mi355_gmc_affine_partial(const double* src, const double* dst, int n, double threshold, double confidence, int max_iters,
                              unsigned long long seed, double* H_out, uint8_t* inliers_out);
typedef struct mi355_gmc mi355_gmc;
int  mi355_gmc_create(int device, mi355_gmc** out);
void mi355_gmc_destroy(mi355_gmc* g);
int  mi355_gmc_step_begin(mi355_gmc* g, const uint8_t* bgr, int height, int width, int oh, int ow, const int* xtab, const int* ytab,
                          double quality, const float* prev_pts, int n_prev, int win, int max_level, int max_iters, double eps, double min_eig);
int  mi355_gmc_step_finish(mi355_gmc* g, uint8_t* gray_out, float* eig_out, uint8_t* ok_out, float* next_pts, uint8_t* status);
/* The pending step's frame as it sits on the device (dense BGR [height][width][3]; valid until the next step_begin / track_begin): the
 * detector pass of the same frame reads this copy through mi355_yolo_infer_device instead of uploading the frame a second time, which is
 * also what lets the two overlap on the GPU (model.track, /root/reference/model.py:38).  Blocks the host until the upload has landed. */
int  mi355_gmc_pending_frame(mi355_gmc* g, const uint8_t** dev_bgr, int* height, int* width);
/* ---- the tracker behind model.track (/root/reference/model.py:38-46), host C++ (csrc/tracker_host.cpp) -------------------------------------
 * Ultralytics' default botsort.yaml tracker, one call per frame: BYTETracker.update's two-stage association on IoU cost fused with the
 * detection score, KalmanFilterXYWH, STrack.multi_gmc's warp of the predicted states, lap.lapjv(extend_cost=True, cost_limit=thresh).
 *   det       [n][6] float32 rows x1, y1, x2, y2, conf, cls (Results.boxes.data of the frame, conf >= 0.1 under .track)
 *   warp      6 doubles, row-major 2 x 3: the camera motion since the previous frame (GMC.apply), or NULL = none
 *   out_rows  [cap][8] float32 rows x1, y1, x2, y2, id, score, cls, idx (idx = row of det); the box is the Kalman state
 * mi355_tracker_update returns the number of confirmed tracks (rows beyond cap are not written), or -1 on a bad argument.  It must be
 * called on EVERY frame, empty ones included (frame counter, lost-track ageing against track_buffer 30). */
typedef struct mi355_tracker mi355_tracker;
int  mi355_tracker_create(int frame_rate, mi355_tracker** out);
void mi355_tracker_destroy(mi355_tracker* t);
int  mi355_tracker_update(mi355_tracker* t, const float* det, int n, const double* warp, float* out_rows, int cap);
int  mi355_tracker_last_rows(const mi355_tracker* t, float* out_rows, int cap);   /* the rows of the last update again (count returned) */
int  mi355_tracker_state(const mi355_tracker* t, int* frame_id, int* ids_issued, int* n_tracked, int* n_lost);
/* which = 0: tracked (confirmed or awaiting confirmation), 1: lost.  Rows of 16 doubles: id, state (1 tracked, 2 lost, 3 removed),
 * confirmed, frame of birth, last matched frame, score, cls, idx, mean[8] = cx cy w h + velocities.  Returns the count. */
int  mi355_tracker_tracks(const mi355_tracker* t, int which, double* out, int cap);
/* BoT-SORT's appearance half (botsort.yaml with_reid: True, model: auto; trackers/bot_sort.py:BOTrack, BOTSORT.get_dists,
 * matching.py:embedding_distance).  The embeddings come from the detector itself (mi355_opts.obj_feats, mi355_yolo_last_feats).
 *   a detection handed a feature f holds curr_feat = f / ||f||; a track's smooth_feat is the first curr_feat it absorbs and after every
 *   later match (any of the three stages, re-activation included) 0.9 * smooth + 0.1 * curr in fp32, brought back to unit length
 *   stages 1 and 3 (the ones that fuse the score): d = IoU cost; mask = d > 1 - proximity_thresh (before the fusion); d = fuse_score(d);
 *   emb = max(0, cosine distance(smooth_feat, curr_feat)) / 2; emb[emb > 1 - appearance_thresh] = 1; emb[mask] = 1; d = min(d, emb).
 *   Stage 2 stays plain IoU.
 * Reductions (norm, dot) run in ascending index over the fp32 values widened to float64, in a float64 accumulator; the norm is rounded
 * to fp32 once before the division, the cosine distance stays float64.  Deviations from Ultralytics: a zero-norm feature stays zeros and
 * its embedding cost is 1 (numpy: NaN), as is that of a track that has absorbed no feature yet; the 50-entry `features` deque, which
 * Ultralytics writes and never reads, is not kept.
 *   cfg       struct_size = sizeof(mi355_tracker_cfg); NULL = mi355_tracker_create.  feat_dim 0 = fixed by the first update that brings
 *             features; a threshold of 0 = its botsort.yaml default (0.5 / 0.8)
 *   feats     NULL, or [n][dim] float32, row i belonging to det row i.  NULL on a with_reid tracker is Ultralytics' `encoder is None`:
 *             that frame associates on IoU alone and no smooth_feat changes.  On a tracker without with_reid feats is not read.
 * mi355_tracker_track_feat (tests): the smooth_feat of live or lost track `track_id` -> the number of floats written (0: the track has
 * absorbed no feature), -1: no such track or dim too small.  mi355_tracker_create / mi355_tracker_update behave exactly as before. */
typedef struct mi355_tracker_cfg {
    int struct_size;
    int with_reid;
    int feat_dim;
    int reserved;
    double proximity_thresh, appearance_thresh;
} mi355_tracker_cfg;
int  mi355_tracker_create_ex(int frame_rate, const mi355_tracker_cfg* cfg, mi355_tracker** out);
int  mi355_tracker_update_feats(mi355_tracker* t, const float* det, int n, const float* feats, int dim, const double* warp, float* out_rows,
                                int cap);
int  mi355_tracker_track_feat(const mi355_tracker* t, int track_id, float* smooth_out, int dim);
/* The pieces, for known-answer tests: the filter on (mean[8], cov[8][8] row-major) in place, and the assignment solver --
 * lap.lapjv(cost [n_rows][n_cols], extend_cost=True, cost_limit): x_out[i] = column of row i or -1, y_out[j] = row of column j or -1. */
int  mi355_kalman_initiate(const double* z_xywh, double* mean, double* cov);
int  mi355_kalman_predict(double* mean, double* cov);
int  mi355_kalman_update(double* mean, double* cov, const double* z_xywh);
int  mi355_kalman_warp(double* mean, double* cov, const double* warp);
int  mi355_lapjv(const double* cost, int n_rows, int n_cols, double cost_limit, int* x_out, int* y_out);
/* Host form of mi355_gmc_prepare_device (csrc/gmc_host.cpp): the same expressions in the same order, hence the same plane and corners. */
int  mi355_gmc_prepare_host(const uint8_t* bgr, int height, int width, int oh, int ow, const int* xtab, const int* ytab, double quality,
                            uint8_t* gray_out, float* eig_out, uint8_t* ok_out);
/* The whole step of GMC.apply_sparseoptflow (ultralytics/trackers/utils/gmc.py) on the object, which keeps the previous frame's plane and
 * ordered corners: track_begin enqueues frame preparation + Lucas-Kanade from the previous frame's corners (downscale 2 is Ultralytics'),
 * track_finish collects, orders the new corners, estimates the partial affine transform (RANSAC over the tracked pairs when more than 4
 * survive) and writes the 2 x 3 matrix, translation in frame pixels (the identity on a first frame / too few points).  An object made by
 * mi355_gmc_create(-1) runs every stage in host C++ and never touches a GPU.  track_state: the previous frame as held (tests). */
int  mi355_gmc_track_begin(mi355_gmc* g, const uint8_t* bgr, int height, int width, int downscale);
int  mi355_gmc_track_finish(mi355_gmc* g, double* H_out);
/* n consecutive frames in ONE call (a batched sweep holds a detector batch's frames before the tracker needs their warps): all n frame
 * preparations as one set of launches, all n Lucas-Kanade steps as one launch, corner ordering and RANSAC on host threads.  H_out [n][6] is
 * bit for bit what n track_begin / track_finish steps return; the object's previous frame is continued from and left behind. */
int  mi355_gmc_track_batch(mi355_gmc* g, const uint8_t* const* frames, int n, int height, int width, int downscale, double* H_out);
/* The frames a mi355_gmc_track_batch call (on another thread, or returned) has uploaded, for the detector pass of the same batch to read in
 * place: waits up to timeout_ms for an upload numbered above after_seq (= mi355_gmc_batch_seq taken before that call was started), then
 * frame f is at dev + f * stride on the object's GPU (dense BGR; stride == height * width * 3 when that is a multiple of 16).  Valid until
 * the next mi355_gmc_track_batch on the object.  0 = ok, 1 = nothing new within the timeout (cvsd_amd/sweep.py: the production sweep of
 * /root/reference/preprocess.py:36-47). */
unsigned long long mi355_gmc_batch_seq(mi355_gmc* g);
int  mi355_gmc_batch_frames(mi355_gmc* g, unsigned long long after_seq, int timeout_ms, const uint8_t** dev, int* n, int* height, int* width,
                            long long* stride);
int  mi355_gmc_track_reset(mi355_gmc* g);
int  mi355_gmc_track_state(const mi355_gmc* g, int* oh, int* ow, int* n_pts, uint8_t* gray_out, float* pts_out, int pts_cap);
/* Several cameras, one motion-compensation step per tick (csrc/gmc_kernels.hip): n_cameras independent GMC states in one object.  A tick is
 * ONE launch per stage for all cameras that delivered a frame, whatever their sizes (per-camera descriptors on the device, uploaded only
 * when their bytes change; the tick's frames staged in pinned memory and uploaded once); every camera's 2 x 3 matrix, previous plane and
 * corners are bit for bit those of a mi355_gmc object of its own fed the same frames.  device -1: every stage in host C++, no GPU touched.
 *   begin   frames[i] = camera i's BGR frame [heights[i]][widths[i]][3], NULL = camera absent this tick (its state is kept); enqueues on the
 *           object's stream and returns; corner ordering + RANSAC per camera run on at most min(present, 8) worker threads from then on
 *   finish  joins them; H_out [n_cameras][6], rows of absent cameras untouched.  Every begin is followed by exactly one finish.
 *   frames  the pending tick's frames on the device (dense BGR, 256-byte aligned starts; NULL = absent) after one event wait: the detector
 *           pass of the tick reads them in place (mi355_yolo_infer_multi, frames_on_device = 1).  Valid until the next begin.
 *   reset   forgets camera `camera`'s previous frame (-1: all).  A camera whose frame size changes restarts like a mi355_gmc object.
 *   state   camera's previous frame as held (tests), as mi355_gmc_track_state.
 * 0 = ok, -1 = bad argument or call out of order, -2 = HIP error. */
typedef struct mi355_gmc_multi mi355_gmc_multi;
int  mi355_gmc_multi_create(int device, int n_cameras, mi355_gmc_multi** out);
void mi355_gmc_multi_destroy(mi355_gmc_multi* g);
int  mi355_gmc_multi_begin(mi355_gmc_multi* g, const uint8_t* const* frames, const int* heights, const int* widths, int downscale);
int  mi355_gmc_multi_finish(mi355_gmc_multi* g, double* H_out);
int  mi355_gmc_multi_frames(mi355_gmc_multi* g, const uint8_t** dev_frames);
int  mi355_gmc_multi_reset(mi355_gmc_multi* g, int camera);
int  mi355_gmc_multi_state(const mi355_gmc_multi* g, int camera, int* oh, int* ow, int* n_pts, uint8_t* gray_out, float* pts_out, int pts_cap);

/* ---- motion gate: which cameras of a tick changed since their last detector pass ------------------------------------
 * Integer arithmetic only (csrc/motion_grid.h; the kernel of csrc/motion_kernels.hip and its host twin give the same numbers).
 *   luma      of a BGR pixel (bytes_per_pixel 3): (1868 B + 9617 G + 4899 R + 8192) >> 14, the luma of the motion compensation;
 *             of a Y-plane pixel (bytes_per_pixel 1): its byte.
 *   grid      gh = ceil(height / block) by gw = ceil(width / block) blocks of block x block pixels (edge blocks are partial);
 *             S[b] = uint32 sum of the luma of block b's pixels, P[b] = their number.
 *   changed   block b is flagged when 16 |S_cur[b] - S_ref[b]| > level_q P[b], level_q = floor(16 level + 0.5); a camera without a
 *             reference has every block flagged.  A camera's `changed` is its number of flagged blocks.
 *   moving    a present camera moves when it has no reference (first frame, after a reset, height / width / bytes_per_pixel differ from
 *             its previous frame's), when changed >= min_blocks, or when it has been static for max_skip consecutive present ticks.
 *             A moving camera's current grid becomes its reference (two buffers per camera swap roles) and its static run restarts; a
 *             static camera keeps its reference -- slow drift adds up until it trips -- and its run grows by one.
 *   absent    a NULL frame descriptor: the camera's state is untouched; moving = 0, changed = -1.
 * Options: block 8, 16 or 32; level in [0, 255]; min_blocks >= 0 (0: every present camera moves); max_skip < 0: never forced.  A NULL
 * options pointer means block 16, level 2, min_blocks 4, max_skip 30.  At most MI355_MOTION_MAX_CAMERAS cameras.
 *   create   device >= 0: a stream of its own on that GPU; -1: the host twin, which touches no GPU.
 *   update   frames[i] = camera i's descriptor or NULL.  frames_on_device = 0: host memory, staged with the caller's row pitch and base
 *            alignment (modulo 16) and uploaded once per call on the gate's stream, in front of the launch.  frames_on_device = 1: memory
 *            of the gate's GPU, read in place -- the caller orders the call behind whatever wrote the frames (the pointers of
 *            mi355_gmc_multi_frames come back behind an event wait for that upload).  ONE launch for all present cameras, one copy of the
 *            per-strip counts into pinned memory, one stream wait.  Rows whose address is 16-byte aligned are read with 16-byte loads,
 *            4-byte aligned ones with 4-byte loads, others by bytes.  moving[n_cameras], changed[n_cameras] are written for every camera.
 *   mask     camera's flag grid of its last present tick: flags_out [gh][gw] (may be NULL to query gh, gw; both 0 before its first frame).
 *   reset    forgets camera's reference and static run (-1: every camera's).
 *   mi355_op_motion_grid   the sums alone (parity tests): n host frames -> sums_out[i] = uint32 [gh_i][gw_i].
 * MI355_EINVAL before any launch: a block, level or min_blocks outside the above, n_cameras outside [1, 64], a non-positive height or
 * width, bytes_per_pixel other than 1 or 3, a row_stride smaller than a row, a frame of 2 GiB or more, device frames for a host gate. */
#define MI355_MOTION_MAX_CAMERAS 64
typedef struct mi355_motion_opts {
    int struct_size;                    /* sizeof(mi355_motion_opts) */
    int block;                          /* 8, 16 or 32 */
    float level;                        /* mean luma change of a block that counts, in [0, 255] */
    int min_blocks;                     /* changed blocks that make a camera move */
    int max_skip;                       /* static present ticks after which the detector is forced; < 0: never */
} mi355_motion_opts;
typedef struct mi355_motion_frame {
    const uint8_t* data;                /* first pixel */
    int height, width, row_stride;      /* row_stride in bytes, >= width * bytes_per_pixel */
    int bytes_per_pixel;                /* 3: BGR, 1: the Y plane of an NV12 / I420 frame */
} mi355_motion_frame;
typedef struct mi355_motion_gate mi355_motion_gate;
int  mi355_motion_gate_create(int device, int n_cameras, const mi355_motion_opts* opts, mi355_motion_gate** out);
void mi355_motion_gate_destroy(mi355_motion_gate* g);
int  mi355_motion_gate_update(mi355_motion_gate* g, const mi355_motion_frame* const* frames, int frames_on_device, int* moving, int* changed);
int  mi355_motion_gate_mask(mi355_motion_gate* g, int camera, uint8_t* flags_out, int cap, int* gh, int* gw);
int  mi355_motion_gate_reset(mi355_motion_gate* g, int camera);
int  mi355_op_motion_grid(int device, const mi355_motion_frame* frames, int n, int block, uint32_t* const* sums_out);

/* ---- evidence frames: boxes, labels, skeletons and mosaics drawn into a COPY of a frame --------------------------------
 * A small rasteriser in integer arithmetic (csrc/render_raster.h; the kernels of csrc/render_kernels.hip and their host twin give the
 * same bytes).  Out of place: the source is only read.  BGR in, BGR out, solid colours, no blending.
 * A primitive is MI355_RENDER_WORDS int32: {type, a, b, c, d, size, colour, 0}, colour = B | G << 8 | R << 16.  Pixel (px, py) is a
 * point; a rectangle a, b, c, d = x0, y0, x1, y1 holds x0 <= px <= x1 and y0 <= py <= y1 (x1 < x0 or y1 < y0: empty).
 *   MOSAIC  rectangle, size B in {4, 8, 16, 32}: a covered pixel takes, per channel, (2 S + N) / (2 N) (integer division) of the SOURCE
 *           frame's B x B block holding it -- blocks aligned to the frame's origin, S the sum and N the number of the block's pixels
 *           inside the frame (the whole block, not the rectangle's part of it).
 *   RECT    rectangle, size t: the rectangle without the rectangle shrunk by t on every side.
 *   FILL    rectangle.
 *   LINE    A = (a, b), B = (c, d), size t: pixels within t / 2 of the segment.  With u = (p - A) . (B - A): u <= 0 -> 4 |p - A|^2 <= t^2;
 *           u >= |B - A|^2 -> 4 |p - B|^2 <= t^2; else 4 cross(B - A, p - A)^2 <= t^2 |B - A|^2.  A = B is a disc of diameter t.
 *   DISC    centre (a, b), size r: (px - a)^2 + (py - b)^2 <= r^2.
 *   GLYPH   top-left (a, b), c = character (0-9 # . : % - space), size = scale: a 5 x 7 bitmap, each bit a scale x scale square.
 * Order: the mosaics first, in ascending index, every one reading the source; then the others in ascending index, the last writer wins.
 * Everything is clipped to the frame; primitives partly or wholly outside it are legal.
 * Ranges: |coordinate| <= 2^20, height and width <= 16384, t in 1 .. 255, r in 0 .. 2^20, scale in 1 .. 64, at most
 * MI355_RENDER_MAX_PRIMS primitives per frame (300 boxes x (mosaic + box + 11 of a label + 19 limbs + 17 joints) fit) and
 * MI355_RENDER_MAX_FRAMES frames per call.  Anything else -- one primitive too many included -- is MI355_EINVAL with a message naming
 * the limit, before a byte of any output is written: nothing is ever dropped silently.
 *   mi355_render   device >= 0: that GPU; -1: the host twin (host memory only), which touches no GPU.  frames[i] / outs[i]: host memory
 *            (staged with the caller's pitch and address modulo 16, one upload per frame) or memory of that GPU (on_device = 1, read /
 *            written in place; the caller orders the call behind whatever wrote the frames).  prims[i] = n_prims[i] host records.  All
 *            frames of a call, whatever their sizes and pitches, take one memset of the bins and two launches on `stream` (NULL: the
 *            null stream); the call returns when they and the copies have finished.  Of an output only the height x width x 3 pixel bytes
 *            are written.  launch_ms (or NULL) receives the device time from the memset to the end of the draw launch. */
#define MI355_RENDER_WORDS      8
#define MI355_RENDER_MAX_PRIMS  16384
#define MI355_RENDER_MAX_FRAMES 256
#define MI355_RENDER_MOSAIC 1
#define MI355_RENDER_RECT   2
#define MI355_RENDER_FILL   3
#define MI355_RENDER_LINE   4
#define MI355_RENDER_DISC   5
#define MI355_RENDER_GLYPH  6
typedef struct mi355_render_frame {
    const uint8_t* data;                /* first pixel of a BGR frame */
    int height, width, row_stride;      /* row_stride in bytes, >= 3 * width */
    int on_device;                      /* 1: memory of the call's GPU */
} mi355_render_frame;
typedef struct mi355_render_out {
    uint8_t* data;                      /* height x width BGR pixels of the frame it answers */
    int row_stride;
    int on_device;
} mi355_render_out;
int  mi355_render(int device, const mi355_render_frame* frames, int n, const int32_t* const* prims, const int* n_prims,
                  const mi355_render_out* outs, void* stream, float* launch_ms);
/* The same call on an engine handle: its stream, and scratch that is kept between calls.  frames = NULL renders THE FRAMES OF THE
 * HANDLE'S LAST BLOCKING INFER CALL from where that call left them on the device, so a host or YUV frame is not uploaded (or converted)
 * twice: the staging slot of mi355_yolo_infer / _multi / _yuv, the one copy of a tiled call, or the caller's own device memory (which
 * the caller keeps alive and unchanged).  They stay there until the handle's next infer or raw_head call.  The staging area holds two
 * chunks (mi355_opts.batch_chunk frames each), so of a host or YUV call of more than two chunks only the last two chunks' frames
 * remain; mi355_yolo_last_frames says which (data = NULL: gone) and the call refuses a NULL `frames` when one is gone -- the
 * caller then passes descriptors of the frames again.  The asynchronous device-output calls record nothing.  n must be the last call's
 * number of frames (a tiled call: of its source frames). */
int  mi355_yolo_render(mi355_yolo* h, const mi355_render_frame* frames, int n, const int32_t* const* prims, const int* n_prims,
                       const mi355_render_out* outs, float* launch_ms);
int  mi355_yolo_last_frames(mi355_yolo* h, mi355_render_frame* frames_out, int cap, int* n);

/* ---- person crops: rectangles cut out of BGR frames, copied or resampled to one size ----------------------------------
 * Integer arithmetic on the device (csrc/crop_resize.h; the kernel of csrc/crop_kernels.hip and its host twin give the same bytes).
 * rects[i] = n_rects[i] host records of four int32 (x1, y1, x2, y2) in pixels of frames[i]: the crop is frame[y1:y2, x1:x2].
 * 0 <= x1, x2 <= width and 0 <= y1, y2 <= height; x2 <= x1 or y2 <= y1 is an EMPTY rectangle, which is legal.
 *   spec->height == 0 and spec->width == 0   native: crop k is a plain copy, (y2 - y1) x (x2 - x1) pixels; an empty rectangle writes
 *            nothing (its output pointer may be NULL).
 *   spec->height, spec->width > 0            every crop has that size.  MI355_CROP_STRETCH: cv2.resize(crop, (width, height),
 *            INTER_LINEAR) in OpenCV's 11-bit fixed point, the taps clamped at the CROP's edges.  MI355_CROP_PAD: the crop is scaled by
 *            r = min(height / ch, width / cw) to round-half-even(side * r) (at least 1) and centred as Ultralytics' LetterBox(auto=False)
 *            centres it, the rest is spec->fill.  An empty rectangle gives a crop of spec->fill.
 * outs: one record per rectangle, all frames' rectangles in frame order (n_rects[0] + ... + n_rects[n - 1] records), host memory or
 * memory of the call's GPU; of an output only the crop's pixel bytes are written.
 *   mi355_crops   device >= 0: that GPU; -1: the host twin (host memory only), which touches no GPU.  frames[i]: host memory (the rows
 *            its rectangles span are uploaded, once) or memory of that GPU (on_device = 1, read in place).  All crops of a call, whatever
 *            their frames and sizes, take ONE launch on `stream`; the call returns when it and the copies have finished.  Nothing
 *            outside a rectangle is read.  launch_ms (or NULL): the launch's device time.
 *   mi355_yolo_crops   the same on an engine handle: its stream, scratch kept between calls; frames = NULL cuts the frames of the
 *            handle's last blocking infer call where that call left them (mi355_yolo_render's rules on which copies are alive).
 * A null pointer, a rectangle with a negative coordinate or one beyond its frame, a size that is not positive (other than 0 x 0), an
 * unknown fit, a fill outside 0 .. 255, a frame or output of 2 GiB or more, or device memory with device = -1 is MI355_EINVAL with a
 * message naming the argument, before a byte of any output is written. */
#define MI355_CROP_STRETCH 0
#define MI355_CROP_PAD     1
#define MI355_CROP_MAX_RECTS 65536      /* per call */
typedef struct mi355_crop_spec {
    int struct_size;                    /* sizeof(mi355_crop_spec) */
    int height, width;                  /* 0, 0: native */
    int fit;                            /* MI355_CROP_* */
    int fill;                           /* 0 .. 255, every channel */
} mi355_crop_spec;
int  mi355_crops(int device, const mi355_render_frame* frames, int n, const int32_t* const* rects, const int* n_rects,
                 const mi355_crop_spec* spec, const mi355_render_out* outs, void* stream, float* launch_ms);
int  mi355_yolo_crops(mi355_yolo* h, const mi355_render_frame* frames, int n, const int32_t* const* rects, const int* n_rects,
                      const mi355_crop_spec* spec, const mi355_render_out* outs, float* launch_ms);

/* ---- evidence frames as JPEG: a BGR frame in, a baseline JFIF stream out ------------------------------------------------
 * Integer arithmetic throughout (csrc/jpeg_codec.h; the kernels of csrc/jpeg_kernels.hip and their host twin give the same bytes).
 * The stream: SOI, APP0 (JFIF 1.01, no thumbnail), DQT (luminance), DQT (chrominance), SOF0, DHT x 4 (DC 0, AC 0, DC 1, AC 1), DRI, SOS,
 * entropy-coded data, EOI.  Baseline sequential DCT, 8 bits, components Y (1), Cb (2), Cr (3); MI355_JPEG_420: Y 2x2 and chroma 1x1,
 * 16 x 16 MCUs, six blocks per MCU (Y0 Y1 / Y2 Y3, Cb, Cr); MI355_JPEG_444: 8 x 8 MCUs of three blocks.  Height and width 1 .. 65535.
 *   tables   Annex K.1 / K.2 scaled by the IJG rule: s = 5000 / q for q < 50, else 200 - 2 q; step = (base * s + 50) / 100 clamped to
 *            1 .. 255; quality q in 1 .. 100.  Huffman: the four typical tables of Annex K.3, no optimisation pass.
 *   restart  the restart interval is the number of MCUs of one MCU row: every MCU row is a segment with DC predictors starting at 0,
 *            its last byte padded with 1-bits, 0x00 behind every 0xFF data byte, and RSTm, m = row mod 8, between it and the next (none
 *            behind the last).  The rows are independent, which is what lets a GPU code them side by side.
 *   pixels   Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, Cb = (-11059 R - 21709 G + 32768 B + 8421375) >> 16,
 *            Cr = (32768 R - 27439 G - 5329 B + 8421375) >> 16.  The frame is extended to whole MCUs by repeating its last column and
 *            row; 4:2:0 chroma is (a + b + c + d + 2) >> 2 of the four Cb (Cr) values; level shift -128; forward DCT: the
 *            Loeffler-Ligtenberg-Moschytz factorisation in 13-bit fixed point, rows then columns (jpeg_fdct_1d), giving 8 x the
 *            coefficient; quantisation (|c| + 4 step) / (8 step) with the sign restored (round half away from zero); zigzag order.
 *   capacity mi355_jpeg_bound(height, width, subsampling): no stream of such a frame is longer, whatever the pixels and the quality --
 *            640 for the header + 416 per 8 x 8 block (1660 bits: the longest DC code and category, 63 x the longest AC code and
 *            category; twice that for stuffing) + 2 per MCU row + 2.  outs[i].capacity must be at least that: there is no truncation path.
 * Out-of-range quality, an unknown subsampling, a zero or > 65535 dimension or a capacity below the bound is MI355_EINVAL with a message
 * naming the field, before a byte of any output is written.
 *   mi355_jpeg_encode   device >= 0: that GPU; -1: the host twin (host memory only), which touches no GPU.  frames[i]: host memory (one
 *            upload per frame) or memory of that GPU (on_device = 1, read in place).  outs[i].data: HOST memory; the call sets
 *            outs[i].length.  All frames of a call, whatever their sizes and pitches, take three launches on `stream`; the call returns
 *            when they and the copies have finished.  Only the streams' bytes cross the bus.  launch_ms (or NULL): the launches' device time.
 *   mi355_yolo_encode   the same on an engine handle: its stream, scratch kept between calls; frames = NULL encodes the frames of the
 *            handle's last blocking infer call where that call left them (mi355_yolo_render's rules on which copies are alive).
 *   mi355_op_jpeg_coefficients   the transform stage alone: coefs[i] (host) receives int16 [blocks][64], quantised, zigzag order, blocks
 *            in scan order (MCU rows, MCUs, blocks of an MCU); blocks = MCUs x (6 | 3). */
#define MI355_JPEG_420 420
#define MI355_JPEG_444 444
typedef struct mi355_jpeg_out {
    uint8_t* data;                      /* host memory of `capacity` bytes */
    int64_t capacity;
    int64_t length;                     /* set by the call */
} mi355_jpeg_out;
int64_t mi355_jpeg_bound(int height, int width, int subsampling);
int  mi355_jpeg_encode(int device, const mi355_render_frame* frames, int n, int quality, int subsampling, mi355_jpeg_out* outs, void* stream,
                       float* launch_ms);
int  mi355_yolo_encode(mi355_yolo* h, const mi355_render_frame* frames, int n, int quality, int subsampling, mi355_jpeg_out* outs,
                       float* launch_ms);
int  mi355_op_jpeg_coefficients(int device, const mi355_render_frame* frames, int n, int quality, int subsampling, int16_t* const* coefs);
/* ---- JPEG ingest: a baseline JPEG stream in host memory in, a BGR frame out ----------------------------------------------
 * Integer arithmetic throughout, libjpeg's default decoder step for step (csrc/jpeg_decode.h; the kernels of
 * csrc/jpeg_decode_kernels.hip and their host twin give the same bytes, and so does Pillow with libjpeg-turbo).
 *   streams  baseline sequential DCT (SOF0), 8 bits, Huffman, one interleaved scan; 3 components with Y sampled 1x1 (4:4:4), 2x1 (4:2:2)
 *            or 2x2 (4:2:0) and chroma 1x1, or 1 component (gray: B = G = R = Y).  Any DQT (8-bit steps, ids 0 .. 3), any DHT (ids 0 .. 1
 *            per class, several tables per marker), DRI optional, APPn and COM skipped.  Height and width 1 .. 65535, a decoded frame
 *            below 2 GiB.  Refused with MI355_EINVAL and a message naming the stream and the reason, before any work and with every
 *            destination untouched: SOF1, SOF2 and the other SOFs, 12-bit precision, 4 components, other sampling factors, several
 *            scans, arithmetic coding, DNL, a missing table, no EOI, a marker other than RSTn inside the scan, RSTn out of sequence.
 *   entropy  Annex F.2.2 per restart segment, DC predictors 0 at each segment's start; coefficients int16 [blocks][64] in zigzag order,
 *            blocks in scan order (MCU rows, MCUs, blocks of an MCU: the Y blocks row by row, Cb, Cr), DC absolute (the low 16 bits of
 *            the running sum).  Decoding terminates inside its buffers for ANY bytes: reads past a segment's end supply zero bits, and
 *            a 16-bit code that matches nothing (MI355_JPEG_CODE_NOT_FOUND), a run that leaves the block (_RUN_PAST_BLOCK), a segment
 *            that ends early (_SEGMENT_SHORT) or has bytes left over (_SEGMENT_LONG) end that stream's decoding with status[i] set.
 *   pixels   coef * step; libjpeg's jpeg_idct_islow (13-bit constants, columns with descale 11, then rows with descale 18, every
 *            descale (x + (1 << (n - 1))) >> n), sample = clamp(x + 128, 0, 255); "fancy" chroma upsampling -- 4:2:2:
 *            out[2x] = (3 p[x] + p[x-1] + 1) >> 2, out[2x+1] = (3 p[x] + p[x+1] + 2) >> 2; 4:2:0: s[x] = 3 p[near][x] + p[far][x] with
 *            far = r - 1 (r + 1) for output row 2r (2r + 1), out[2x] = (3 s[x] + s[x-1] + 8) >> 4, out[2x+1] = (3 s[x] + s[x+1] + 7) >> 4;
 *            neighbour indices clamped to the chroma plane of ceil(W/2) x ceil(H/2) (4:2:2: x H) samples; a chroma plane of at most 2
 *            columns is replicated instead; R = Y + ((91881 cr + 32768) >> 16), G = Y + ((-22554 cb - 46802 cr + 32768) >> 16),
 *            B = Y + ((116130 cb + 32768) >> 16) with cb, cr less 128, clamped to 0 .. 255, stored B, G, R.
 *   mi355_jpeg_info     parses a stream's header and finds its scan: geometry, subsampling (444, 422, 420; 400 = gray), restart
 *            interval in MCUs (0: none), segments (restart intervals of the scan; 1 without DRI) and 8 x 8 blocks of the coefficient
 *            array.  A refused stream gives MI355_EINVAL and its reason in mi355_last_error().
 *   mi355_jpeg_decode   device >= 0: that GPU; -1: the host twin, which touches no GPU (host destinations only).  streams[i]: HOST
 *            bytes.  outs[i]: the BGR destination of stream i in host memory or memory of that GPU (on_device = 1), row_stride >= 3 x
 *            width.  entropy: MI355_JPEG_ENTROPY_GPU -- one GPU lane per restart segment (a stream without DRI is one segment on one
 *            lane: slow, correct); _HOST -- the twin's segment routine on the calling thread, the coefficients uploaded (128 bytes per
 *            block), only the idct and colour launches run; _AUTO -- _GPU for a stream with a restart interval, _HOST for one without;
 *            _SYNC -- many GPU lanes per restart segment: the self-synchronising parallel Huffman decoder of csrc/jpeg_sync.h, for
 *            streams without restart markers (opt-in: _AUTO never chooses it; device -1 runs its host twin, round for round).
 *            streams[i].entropy, when non-zero, is that stream's own request and replaces the call's argument for it.
 *            The call sets streams[i].entropy_used.  All streams of a call, whatever their sizes and layouts, take three launches on
 *            `stream` (two when no stream's entropy stage runs on the GPU, four more when any stream is decoded with _SYNC: local
 *            rounds, global rounds + block index, write pass, DC pass); the stream bytes are staged through pinned memory in one
 *            copy; the call returns when the launches and copies have finished.  status (n ints, or NULL) receives 0 or an
 *            MI355_JPEG_* status per stream.  When any is non-zero the call returns MI355_EINVAL naming the first such stream; the
 *            other streams' frames are complete, a failed stream's host destination is untouched.  launch_ms (or NULL): the launches'
 *            device time.  At most MI355_RENDER_MAX_FRAMES streams per call.
 *   mi355_yolo_decode   the same on an engine handle: its device and stream, scratch kept between calls.
 *   mi355_op_jpeg_decode_coefficients   the entropy stage alone: coefs[i] (host) receives int16 [blocks][64].
 *   mi355_op_jpeg_sync   test hook of _SYNC on one stream with subsequences of sub_bytes bytes (a power of two >= 8) and sequences of
 *            seq_subs subsequences (2 .. 256); device -1: the host twin.  coef (host, int16 [blocks][64]) and status as above (a corrupt
 *            stream is no error of this call); states[i], i < stats->nsub: the true entry state of subsequence i -- its segment, the
 *            position (byte, bit) relative to the segment's begin, the block j within the MCU, the zigzag index k of the next coefficient
 *            (0: a DC symbol) and the block in progress; stats: subsequences, sequences, rounds_local (the most local rounds in which
 *            something changed, over the sequences) and rounds_global (the global rounds in which something changed).  With coef NULL
 *            only stats->nsub and stats->nseq are filled: what the caller needs to size `states` (max_states entries). */
#define MI355_JPEG_ENTROPY_AUTO 0
#define MI355_JPEG_ENTROPY_GPU  1
#define MI355_JPEG_ENTROPY_HOST 2
#define MI355_JPEG_ENTROPY_SYNC 3
#define MI355_JPEG_CODE_NOT_FOUND 1
#define MI355_JPEG_RUN_PAST_BLOCK 2
#define MI355_JPEG_SEGMENT_SHORT  3
#define MI355_JPEG_SEGMENT_LONG   4
typedef struct mi355_jpeg_stream {
    const uint8_t* data;                /* host memory */
    int64_t length;
    int entropy_used;                   /* set by the call: MI355_JPEG_ENTROPY_GPU, _HOST or _SYNC */
    int entropy;                        /* this stream's own request, MI355_JPEG_ENTROPY_*; 0: the call's argument */
} mi355_jpeg_stream;
typedef struct mi355_jpeg_sync_state {
    int segment;
    uint32_t byte;
    int bit, j, k;
    uint32_t block;
} mi355_jpeg_sync_state;
typedef struct mi355_jpeg_sync_stats {
    int nsub, nseq, rounds_local, rounds_global;
} mi355_jpeg_sync_stats;
typedef struct mi355_jpeg_stream_info {
    int height, width, components;
    int subsampling;                    /* 444, 422, 420; 400: gray */
    int restart_interval;               /* MCUs; 0: none */
    int segments;
    int64_t blocks;                     /* 8 x 8 blocks of the coefficient array */
} mi355_jpeg_stream_info;
int  mi355_jpeg_info(const uint8_t* data, int64_t length, mi355_jpeg_stream_info* info);
int  mi355_jpeg_decode(int device, mi355_jpeg_stream* streams, int n, int entropy, const mi355_render_out* outs, int* status, void* stream,
                       float* launch_ms);
int  mi355_yolo_decode(mi355_yolo* h, mi355_jpeg_stream* streams, int n, int entropy, const mi355_render_out* outs, int* status,
                       float* launch_ms);
int  mi355_op_jpeg_decode_coefficients(int device, mi355_jpeg_stream* streams, int n, int entropy, int16_t* const* coefs, int* status);
int  mi355_op_jpeg_sync(int device, mi355_jpeg_stream* stream, int sub_bytes, int seq_subs, int16_t* coef, int* status,
                        mi355_jpeg_sync_state* states, int max_states, mi355_jpeg_sync_stats* stats);
/* Depthwise 3x3 conv (stride 1, pad 1) + bias (+SiLU) (+residual) on channel views, fp32, as the engine runs YOLO11's
 * DWConv and Attention.pe (ultralytics nn/modules/conv.py:DWConv, Conv with groups = c).  x[n][h][w][x_cs] holds the input view at
 * channels x_off .. x_off+c-1; residual (or NULL) [n][h][w][res_cs] at res_off; y[n][h][w][y_cs] is read in, its view y_off ..
 * y_off+c-1 written and every other channel handed back unchanged.  w[c][1][k][k], bias[c].  All strides and offsets are
 * multiples of 4 and every view lies inside its tensor. */
int  mi355_op_dwconv2d(int device_id, const float* x, int n, int h, int w, int x_cs, int x_off, int c, const float* w_c1kk,
                       const float* bias, int k, int silu, const float* residual, int res_cs, int res_off, float* y, int y_cs,
                       int y_off);
/* PSA attention (ultralytics nn/modules/block.py:Attention between qkv and pe), fp32: qkv[n][hw][heads*(2*key_dim+head_dim)] laid
 * out [q of every head | k of every head | v of every head]; y[n][hw][heads*head_dim] = per frame and head
 * softmax_j(q_i . k_j * key_dim^-0.5) v_j.  key_dim 32, head_dim 64 (every YOLO11 scale). */
int  mi355_op_psa_attention(int device_id, const float* qkv, int n, int hw, int heads, int key_dim, int head_dim, float* y);
/* The head decode kernel alone (DFL + dist2bbox, class sigmoid -> best score / first argmax, keypoint decode), fp32, on raw head
 * maps of the caller: bufs[l] = [n][h][w][cs] and geom[l] = {cs, box_off, cls_off, kpt_off, h, w, stride} for each of n_levels
 * (1 .. 4) levels; 64 box logits at box_off, nc class logits at cls_off, nkpt*kdim keypoint values at kpt_off (kdim 2 or 3, or
 * nkpt = kdim = 0).  mode 0: the raw-head form (every class score stored); 1: the form NMS runs behind (box, keypoints and best
 * only); 2: the split form of the sparse box branch -- the score stage, then the box stage behind a device gate word set to
 * `gate`; *fallback_count (or NULL) receives the box stage's counter.  pred[n][A][4+nc+nkpt*kdim] (anchor-major) and best[n][A][2]
 * are read in and handed back, so whatever the launch does not write keeps the caller's bits.  The launcher's alignment rules
 * (cs and box_off multiples of 4) come back as MI355_EHIP with its message. */
int  mi355_op_decode(int device_id, const float* const* bufs, const int* geom, int n_levels, int n, int nc, int nkpt, int kdim,
                     int mode, int gate, float* pred, float* best, int* fallback_count);
/* The object-feature gather alone (csrc/post_kernels.hip: one wave per row slot), on maps of the caller: bufs[l] = [n][h][w][cs] and
 * geom[l] = {cs, c_off, C, h, w} for each of n_levels (1 .. 4) levels, the level's channels at c_off .. c_off + C - 1; half = 0: fp32
 * elements, 1: fp16 bit patterns (all levels alike).  dim must be min(C_l) and divide every C_l; cs and c_off are multiples of 4
 * (fp32) or 8 (fp16) elements.  anchor_idx[n][cap] in [0, A), A = sum h*w, P3 row-major first; counts[n] in [0, cap].
 * feats[n][cap][dim] is read in and handed back, so rows at or beyond counts[i] keep the caller's bits. */
int  mi355_op_obj_feats(int device_id, const void* const* bufs, const int* geom, int n_levels, int n, int half, const int* anchor_idx,
                        const int* counts, int cap, int dim, float* feats);
/* The sparse box branch alone (csrc/conv_f32_sparse.hip), enqueued as a pass enqueues its sparse tail minus the dense launches:
 * the 12 state ints zeroed, the lists kernel, then cv2.i.0 at the dilated and cv2.i.1 -> cv2.i.2 -> DFL -> box at the candidate
 * positions.  n_levels 1 .. 3; per level l
 *   geom[11 l ..] = {h, w, src_cs, src_off, cin, cout_a, stride, mid_cs, mid_off, cap_dil, cap_cand}
 *   ptrs[10 l ..] = {src, wA, bA, wB, bB, wC, bC, mid, dil, cand}
 * src[n][h][w][src_cs] holds the neck map at channels src_off .. src_off+cin-1 (cin a multiple of 16); wA[cout_a][cin][3][3]
 * (cout_a >= 64: the first 64 couts are cv2.i.0, a merged cv3.i.0 may follow), wB[64][64][3][3], wC[64][64][1][1] are OIHW with
 * their biases; mid[n][h][w][mid_cs] is read in, channels mid_off .. mid_off+63 of the dilated pixels written, and handed back;
 * dil / cand receive the first min(count, cap) list entries (b*h*w + y*w + x, in no fixed order).  Strides and offsets are
 * multiples of 4, capacities lie in 1 .. n*h*w.  best[n][A][2] (score, class) is the caller's; conf and classes[n_classes] (or
 * NULL = every class) filter as NMS does.  pred[n][A][no] is read in and handed back with columns 0 .. 3 of the candidate anchors
 * written; act as in the conv epilogues (1 = SiLU).  state[12] receives the device words: [0, 3) dilated counts, [4, 7)
 * candidate counts, [8] = 1 when a list overflowed (nothing else is then written). */
int  mi355_op_sparse_box(int device_id, void* const* ptrs, const int* geom, int n_levels, int n, const float* best, float conf,
                         const int* classes, int n_classes, int nc, int no, int act, float* pred, int* state);
/* SPPF's three chained MaxPool2d(5, 1, 2) on channel views: x[n][h][w][x_cs] holds the input view at channels x_off .. x_off+c-1;
 * y[n][h][w][y_cs] is read in, x1|x2|x3 written to channels y_off .. y_off+3c-1 and every other channel handed back unchanged.
 * half = 0: fp32 elements, c, strides and offsets multiples of 4; half = 1: fp16 bit patterns, multiples of 8. */
int  mi355_op_sppf_pools(int device_id, const void* x, int n, int h, int w, int x_cs, int x_off, int c, void* y, int y_cs, int y_off,
                         int half);
/* Nearest 2x upsample of 32-bit words on channel views (also the engine's copy of fp16 pairs: the words are never interpreted):
 * x[n][h][w][x_cs] view x_off .. x_off+c-1 -> y[n][2h][2w][y_cs] view y_off .. y_off+c-1; y is read in and its other channels
 * handed back unchanged.  Strides and offsets are multiples of 4, c is any positive count. */
int  mi355_op_upsample2x(int device_id, const uint32_t* x, int n, int h, int w, int x_cs, int x_off, int c, uint32_t* y, int y_cs,
                         int y_off);
/* The u8 stem: letterboxed BGR frames -> (x/255, RGB) -> conv k x k stride s (pad k/2, or 2 for k=6) + bias + SiLU. */
int  mi355_op_stem(int device_id, const uint8_t* bgr, int n, int h, int w, const float* w_oihw, const float* bias,
                   int cout, int k, int stride, float* y);
/* The half=True form of the same op (input, weights and output rounded to fp16 as the half predictor does, fp32 accumulation); y holds
 * fp16 bit patterns.  variant: 0 = the kernel the engine launches, 1 = the general kernel, 2 = the k 3 / stride 2 kernel. */
int  mi355_op_stem_f16(int device_id, const uint8_t* bgr, int n, int h, int w, const float* w_oihw, const float* bias,
                       int cout, int k, int stride, int variant, uint16_t* y);
/* data/augment.py:LetterBox on uint8 BGR frames (cv2.resize INTER_LINEAR fixed-point + 114 border).
 * out must hold n * out_h * out_w * 3 bytes where (out_h,out_w) = mi355_letterbox_shape(). */
int  mi355_letterbox_shape(int height, int width, int imgsz, int* out_h, int* out_w);
int  mi355_op_letterbox(int device_id, const uint8_t* bgr, int n, int height, int width, int imgsz, uint8_t* out);
/* Host-only: the letterbox geometry the engine uses for one frame.  auto_pad = 1: LetterBox auto=True (rect, padding modulo 32);
 * 0: auto=False (square imgsz x imgsz).  i6 = Hl, Wl, Hr, Wr, top, left; d5 = the scale_boxes / scale_coords constants
 * gain, pad_x, pad_y (rounded, boxes), kpad_x, kpad_y (unrounded, keypoints), in double. */
int  mi355_letterbox_geometry(int height, int width, int imgsz, int auto_pad, int* i6, double* d5);
/* The per-frame letterbox of a batch of frames of different sizes (the kernel mi355_yolo_infer_multi runs): HOST frames as in
 * mi355_yolo_infer_multi, every one letterboxed to the square imgsz x imgsz canvas; out[n][imgsz][imgsz][3]. */
int  mi355_op_letterbox_multi(int device_id, const uint8_t* const* frames, const int* heights, const int* widths,
                              const int* row_strides, int n, int imgsz, uint8_t* out);
/* utils/nms.py:non_max_suppression on a decoded head tensor pred[n][4+nc+extra][A] (Ultralytics layout).
 * Rows come back in letterboxed pixels (no scale-back): x1,y1,x2,y2,conf,cls,anchor_idx, kpt = the `extra` columns. */
int  mi355_op_nms(int device_id, const float* pred, int n, int nc, int extra, int anchors, float conf, float iou,
                  const int* classes, int n_classes, int max_det, mi355_det* out_rows, int out_capacity_per_image,
                  int* out_counts);
/* The same launches with every argument a pass sets open to the caller, plus the row compaction behind them.  pred as above; best
 * [n][A][2] (score, class) or NULL (then computed from pred's class columns as mi355_op_nms does).  kdim 0, 2 or 3: how the `extra`
 * columns are read by scale-back (x, y[, conf] per keypoint; 0 = no keypoints).  geom_mode 0: no scale-back (geom NULL); 1: geom =
 * {gain, pad_x, pad_y, kpad_x, kpad_y, orig_w, orig_h} for every frame; 2: geom[n][7], one row per frame.  rows[n][max_det][58 words]
 * and, with pack != 0, packed[n * max_det][58 words] and offsets[n + 1] are read in and handed back, so whatever the launches do not
 * write keeps the caller's bits; counts[n] receives the kept rows per frame.  Which launch path runs follows from n and anchors
 * alone: anchors > 16384 the multi-launch sort, else n <= 16 the fused kernel, else sort + greedy.  Refused with
 * MI355_EINVAL before any device call: max_det outside 1 .. 1024, max_nms < 1, extra > MI355_MAX_KPT_FLOATS, kdim not 0 / 2 / 3 or
 * not dividing extra, conf < 0, and -- with a class list -- a class of a supplied best[] outside 0 .. nc-1. */
int  mi355_op_nms_ex(int device_id, const float* pred, const float* best, int n, int nc, int extra, int anchors, float conf, float iou,
                     const int* classes, int n_classes, int max_det, int max_nms, int kdim, const float* geom, int geom_mode, int pack,
                     uint32_t* rows, int* counts, uint32_t* packed, int* offsets);

/* ---- Shopformer: pose windows -> anomaly score ----------------------------------------------------------------
 * The score path of the reference's shopformer/ network in eval() mode as one fused kernel launch per call, whatever n is.
 * `image` is the weight image cvsd_amd/shopformer.py builds from a checkpoint (folded BatchNorms, matrices in MFMA fragment order).
 * windows [n][2][seq_len][num_keypoints] fp32, normalised as the reference's loader does; scores [n]; tokens and recon
 * [n][n_tokens][d_model] or NULL.  A window's outputs do not depend on n or on its position in the batch, bit for bit.
 * The device_async form takes device pointers, enqueues the one launch on the caller's stream (NULL = the null stream) and returns.
 * The blocking form stages through buffers and a stream owned by the handle: one call at a time per handle (not re-entrant); use one
 * handle per thread, or the device_async form with buffers of the caller. */
typedef struct mi355_shopformer mi355_shopformer;
typedef struct {
    int num_keypoints, seq_len, hidden_channels, latent_channels, heads, layers, n_tokens, d_model;
    int group;              /* windows per workgroup */
    int lds_bytes;          /* LDS the plan of that group uses */
    int variant;            /* 1 = shopformer/ (version-1 image), 2 = shopformer_2/ (version-2 image); was reserved */
    int group_transformer;  /* windows per workgroup of the transformer phase (variant 1: = group); was reserved */
    long long n_params, macs_per_window;
    long long launches;     /* kernel launches this handle has enqueued so far: a counter incremented beside the launch itself */
} mi355_shopformer_info_t;
int  mi355_shopformer_create(const void* image, size_t nbytes, int device_id, mi355_shopformer** out);
void mi355_shopformer_destroy(mi355_shopformer* h);
int  mi355_shopformer_info(const mi355_shopformer* h, mi355_shopformer_info_t* info);
int  mi355_shopformer_score(mi355_shopformer* h, const float* windows, int n, float* scores, float* tokens, float* recon);
int  mi355_shopformer_score_device_async(mi355_shopformer* h, const float* windows_dev, int n, float* scores_dev, float* tokens_dev,
                                         float* recon_dev, void* stream);
/* Version-2 images hold the reference's shopformer_2/ network: pre-norm layers, erf GELU, two tokens per window,
 * tokens and recon [n][n_tokens][latent_channels * num_keypoints].  The functions above take them too (two launches per call:
 * tokenizer, then the transformer over groups of up to 16 windows).  The _ex forms add the per-token scores: every pointer of the
 * struct is optional (at least one must be set; struct_size = sizeof), token_scores [n][n_tokens] exists for version-2 images only.
 * Host pointers for mi355_shopformer_score_ex, device pointers for the device_async form; a device_async call without a tokens
 * output keeps the tokens in a scratch buffer of the handle, grown (hipMalloc) by the first call with a larger n. */
typedef struct {
    int struct_size, reserved;
    float* scores;          /* [n] */
    float* token_scores;    /* [n][n_tokens] */
    float* tokens;          /* [n][n_tokens][token width] */
    float* recon;           /* [n][n_tokens][token width] */
    /* the struct grew here (see below); struct_size may be the size up to this point, the two pointers below are then absent */
    float* poses;           /* [n][2][seq_len][num_keypoints]: the GCAE decoder's reconstruction of the window */
    float* pose_error;      /* [n][seq_len][num_keypoints]: mean over the 2 channels of (poses - windows)^2; needs poses */
} mi355_shopformer_outputs_t;
int  mi355_shopformer_score_ex(mi355_shopformer* h, const float* windows, int n, const mi355_shopformer_outputs_t* out);
int  mi355_shopformer_score_ex_device_async(mi355_shopformer* h, const float* windows_dev, int n, const mi355_shopformer_outputs_t* out,
                                            void* stream);
/* Version-3 images (cvsd_amd/shopformer.py, decoder=True) hold either network plus its GCAE decoder: tokens ->
 * initial_proj -> four (transposed) convolutions -> linear interpolation along time when the layers emit fewer frames than seq_len.
 * `poses` / `pose_error` of the outputs struct ask the _ex calls for it: ONE more launch after the score path's, reading the tokens
 * that path wrote; version-1-variant images are accepted by the _ex calls with scores set.  A caller that passes the struct's
 * earlier size (up to and including `recon`) gets the earlier behaviour.  mi355_shopformer_decode runs the decoder alone on
 * caller-supplied tokens [n][n_tokens][token width] -> poses [n][2][seq_len][num_keypoints] (one launch; no pose_error: there is no
 * window).  A pose's bits do not depend on n or on its position in the batch.  On a handle whose image was built without the
 * decoder each of these fails with MI355_EINVAL before any launch. */
int  mi355_shopformer_decode(mi355_shopformer* h, const float* tokens, int n, float* poses);
int  mi355_shopformer_decode_device_async(mi355_shopformer* h, const float* tokens_dev, int n, float* poses_dev, void* stream);
typedef struct {
    int factors[4];         /* upsample factor of each decoder layer: 2 = (2,1)/(2,1) transposed convolution, 1 = 1x1 convolution */
    int frames;             /* frames the layers emit (n_tokens * product of the factors) */
    int interpolate;        /* 1: frames != seq_len, linear interpolation along time (align_corners=False) follows */
    int group;              /* windows per workgroup: group * n_tokens rows of initial_proj */
    int lds_bytes;
    long long macs_per_window;
} mi355_shopformer_decoder_info_t;
int  mi355_shopformer_decoder_info(const mi355_shopformer* h, mi355_shopformer_decoder_info_t* info);

/* ---- Pose windows on the device -------------------------------------------------------------------------------
 * poses [P][V_src][2]: the x, y of every retained pose, MI355_POSE_F32 or MI355_POSE_F64; window i is the seq_len consecutive poses
 * starts[i] .. starts[i] + seq_len - 1 (windows may overlap).  windows [n][2][seq_len][V] fp32 = what the host loader
 * (cvsd_amd/shopformer.py:_window_tensor) makes of them, bit for bit: joints beyond min(V, V_src) zero, with `neck` joint 17 from the
 * shoulders (joints 5, 6), centred on the mean of the non-zero joints, divided by the largest |offset| + 1e-6, every operation in the
 * poses' own type in numpy's order, non-finite quotients zeroed, one rounding to fp32.
 * Refused with MI355_EINVAL on the host, before any device call: starts[i] < 0 or starts[i] + seq_len > P, V_src < 1, neck with
 * V != 18 or V_src < 7, seq_len * V > 768, an unknown dtype.  n == 0 launches nothing.
 * mi355_pose_windows is the parity hook: host memory in, host memory out (words of windows_out the kernel does not write keep the
 * caller's content); device = -1 runs the same per-window routine compiled for the host and never touches a GPU.
 * mi355_shopformer_score_poses is the whole path in one call: ONE upload of poses and starts, the window launch into the handle's
 * window buffer (seq_len and V are the model's), the score launch(es) of mi355_shopformer_score_ex unchanged, the download of what
 * `out` asks for (host pointers).  The handle's launch counter counts the window launch too. */
#define MI355_POSE_F32 0
#define MI355_POSE_F64 1
int  mi355_pose_windows(int device_or_minus1, const void* poses, int dtype, int P, int V_src, const int* starts, int n, int seq_len, int V,
                        int neck, float* windows_out);
int  mi355_shopformer_score_poses(mi355_shopformer* h, const void* poses, int dtype, int P, int V_src, const int* starts, int n, int neck,
                                  const mi355_shopformer_outputs_t* out);

#ifdef __cplusplus
}
#endif
#endif /* MI355_YOLO_H */
