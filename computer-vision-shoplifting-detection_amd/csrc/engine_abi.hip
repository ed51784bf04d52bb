// The C ABI of include/mi355_yolo.h: engine handle entry points (create / infer / raw_head / plan_info / memory_plan ...).
#include "engine_internal.h"
#include "jpeg_codec.h"
#include "jpeg_decode.h"

namespace mi355 { thread_local std::string g_err; }
using namespace mi355;

extern "C" {

const char* mi355_last_error(void) { return g_err.c_str(); }

int mi355_yolo_create_from_memory(const void* blob, size_t nbytes, int device_id, const mi355_opts* opts, mi355_yolo** out) {
    return create_impl((const uint8_t*)blob, nbytes, device_id, opts, out);
}

int mi355_yolo_create(const char* path, int device_id, const mi355_opts* opts, mi355_yolo** out) {
    if (!path || !out) return fail(MI355_EINVAL, "null argument");
    FILE* f = std::fopen(path, "rb");
    if (!f) return fail(MI355_EIO, std::string("cannot open weights file: ") + path);
    std::fseek(f, 0, SEEK_END);
    const long sz = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    std::vector<uint8_t> buf(sz > 0 ? (size_t)sz : 0);
    const size_t got = buf.empty() ? 0 : std::fread(buf.data(), 1, buf.size(), f);
    std::fclose(f);
    if (got != buf.size() || buf.empty()) return fail(MI355_EIO, std::string("cannot read weights file: ") + path);
    return create_impl(buf.data(), buf.size(), device_id, opts, out);
}

void mi355_yolo_destroy(mi355_yolo* h) { delete h; }

int mi355_yolo_info(const mi355_yolo* h, mi355_model_info* info) {
    if (!h || !info) return fail(MI355_EINVAL, "null argument");
    std::memset(info, 0, sizeof(*info));
    info->task = h->hdr.task; info->nc = h->hdr.nc; info->nkpt = h->hdr.nkpt; info->kdim = h->hdr.kdim;
    info->reg_max = h->hdr.reg_max; info->n_levels = (int)h->levels.size();
    for (size_t i = 0; i < h->levels.size(); ++i) info->strides[i] = h->levels[i].stride;
    info->n_convs = (int)h->convs.size(); info->n_ops = (int)h->ops.size(); info->n_buffers = (int)h->bufs.size();
    info->n_params = h->n_params; info->macs_640 = h->macs640;
    std::strncpy(info->family, h->hdr.family == 0 ? "v8" : h->hdr.family == 1 ? "v5u" : h->hdr.family == 2 ? "v11" : "?", sizeof(info->family) - 1);
    info->scale = (char)h->hdr.scale;
    return MI355_OK;
}

// the filter arguments every infer entry point takes
static InferCall filtered(float conf, float iou, const int* classes, int n_classes, int max_det, int imgsz) {
    InferCall c;
    c.conf = conf; c.iou = iou; c.classes = classes; c.n_classes = n_classes; c.max_det = max_det; c.imgsz = imgsz;
    return c;
}

int mi355_yolo_infer(mi355_yolo* h, const uint8_t* bgr, int n, int height, int width, int row_stride, float conf, float iou,
                     const int* classes, int n_classes, int max_det, int imgsz, mi355_det* out_rows, int cap, int* out_counts) {
    InferCall c = filtered(conf, iou, classes, n_classes, max_det, imgsz);
    c.src = bgr; c.n = n; c.height = height; c.width = width; c.row_stride = row_stride;
    c.out_rows = out_rows; c.cap = cap; c.out_counts = out_counts;
    return infer_impl(h, c);
}

int mi355_yolo_infer_device(mi355_yolo* h, const uint8_t* bgr_dev, int n, int height, int width, float conf, float iou,
                            const int* classes, int n_classes, int max_det, int imgsz, mi355_det* out_rows, int cap, int* out_counts) {
    InferCall c = filtered(conf, iou, classes, n_classes, max_det, imgsz);
    c.src = bgr_dev; c.on_device = true; c.n = n; c.height = height; c.width = width;
    c.out_rows = out_rows; c.cap = cap; c.out_counts = out_counts;
    return infer_impl(h, c);
}

int mi355_yolo_infer_device_async(mi355_yolo* h, const uint8_t* bgr_dev, int n, int height, int width, float conf, float iou,
                                  const int* classes, int n_classes, int max_det, int imgsz, mi355_det* rows_dev, int* counts_dev,
                                  int* total_dev) {
    if (!rows_dev) return fail(MI355_EINVAL, "null argument");
    InferCall c = filtered(conf, iou, classes, n_classes, max_det, imgsz);
    c.src = bgr_dev; c.on_device = true; c.n = n; c.height = height; c.width = width;
    c.dev_rows = rows_dev; c.dev_counts = counts_dev; c.dev_total = total_dev;
    return infer_impl(h, c);
}

void* mi355_yolo_stream(mi355_yolo* h) { return h ? (void*)h->stream : nullptr; }

int mi355_yolo_sync(mi355_yolo* h) {
    if (!h) return fail(MI355_EINVAL, "null argument");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->async_pending = false;
    return MI355_OK;
}

int mi355_yolo_plan_info(const mi355_yolo* h, unsigned long long* plan_hash, int* source, int* launches, long long* activation_bytes,
                         long long* activation_bytes_unshared) {
    if (!h) return fail(MI355_EINVAL, "null argument");
    if (plan_hash) *plan_hash = h->plan_hash;
    if (source) *source = h->plan_source;
    if (launches) *launches = h->plan_launches;
    if (activation_bytes) *activation_bytes = h->act_bytes;
    if (activation_bytes_unshared) *activation_bytes_unshared = h->act_bytes_noreuse;
    return MI355_OK;
}

int mi355_memory_plan(const void* blob, size_t nbytes, int n, int height, int width, int imgsz, int half, int reuse, long long* offsets,
                      long long* sizes, int cap, int* n_buffers, long long* arena_bytes, long long* unshared_bytes) {
    return mi355_memory_plan_ex(blob, nbytes, n, height, width, imgsz, half, reuse, 0, offsets, sizes, cap, n_buffers, arena_bytes,
                                unshared_bytes, nullptr);
}

int mi355_memory_plan_ex(const void* blob, size_t nbytes, int n, int height, int width, int imgsz, int half, int reuse, int obj_feats,
                         long long* offsets, long long* sizes, int cap, int* n_buffers, long long* arena_bytes,
                         long long* unshared_bytes, int* detect_bufs) {
    if (!blob || n <= 0 || height <= 0 || width <= 0 || cap < 0 || (cap > 0 && (!offsets || !sizes))) return fail(MI355_EINVAL, "bad argument");
    if (imgsz <= 0) imgsz = 640;
    if (imgsz % 32) return fail(MI355_EINVAL, "imgsz must be a multiple of 32");
    mi355_yolo h;
    h.host_only = true; h.half = half != 0; h.obj_feats = obj_feats != 0;
    const int rc = parse_blob(&h, (const uint8_t*)blob, nbytes); if (rc) return rc;
    h.mem_reuse = reuse;
    const Geometry g = make_geometry(height, width, imgsz);
    std::vector<size_t> off, bytes; size_t arena = 0, plain = 0;
    plan_memory(&h, n, g.Hl, g.Wl, &off, &bytes, &arena, &plain);
    if (n_buffers) *n_buffers = (int)off.size();
    for (size_t i = 0; i < off.size() && (int)i < cap; ++i) { offsets[i] = (long long)off[i]; sizes[i] = (long long)bytes[i]; }
    if (arena_bytes) *arena_bytes = (long long)arena;
    if (unshared_bytes) *unshared_bytes = (long long)plain;
    for (int l = 0; detect_bufs && l < h.feat_levels; ++l) detect_bufs[l] = h.ops[h.feat_src[l]].src_buf;
    return MI355_OK;
}

int mi355_yolo_feat_dim(const mi355_yolo* h, int* dim) {
    if (!h || !dim) return fail(MI355_EINVAL, "null argument");
    *dim = h->obj_feats ? h->feat_dim : 0;
    return MI355_OK;
}

int mi355_yolo_last_feats(const mi355_yolo* h, float* out, int cap, int n) {
    if (!h || !out || cap < 1) return fail(MI355_EINVAL, "bad argument");
    if (!h->obj_feats || h->last_feat_n == 0) return fail(MI355_EINVAL, "the last infer call on this handle produced no object features");
    if (n != h->last_feat_n) return fail(MI355_EINVAL, "n differs from the last infer call's");
    const size_t dim = (size_t)h->feat_dim;
    const float* src = (const float*)h->h_feats.p;
    size_t at = 0;
    for (int i = 0; i < n; ++i) {
        const int cnt = std::min(h->counts_host()[i], cap);
        std::memcpy(out + (size_t)i * cap * dim, src + (h->last_feat_packed ? at : (size_t)i * h->last_feat_max_det) * dim, (size_t)cnt * dim * sizeof(float));
        at += (size_t)h->counts_host()[i];
    }
    return MI355_OK;
}

int mi355_yolo_set_profiling(mi355_yolo* h, int on) {
    if (!h) return fail(MI355_EINVAL, "null argument");
    h->profiling = on != 0;
    return MI355_OK;
}

int mi355_yolo_last_timing(const mi355_yolo* h, mi355_timing* t) {
    if (!h || !t) return fail(MI355_EINVAL, "null argument");
    *t = h->last;
    return MI355_OK;
}

int mi355_yolo_sparse_stats(mi355_yolo* h, long long* out10) {
    if (!h || !out10) return fail(MI355_EINVAL, "null argument");
    for (int i = 0; i < 10; ++i) out10[i] = 0;
    out10[0] = h->sparse_shape ? 1 : -(long long)h->sparse_why; out10[1] = h->sp_passes;
    if (!h->sp_state) return MI355_OK;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    int st[16];
    HIPCHK(hipMemcpy(st, h->sp_state, sizeof(st), hipMemcpyDeviceToHost));
    out10[2] = st[12];
    for (int l = 0; l < 3; ++l) { out10[3 + l] = st[l]; out10[6 + l] = st[4 + l]; }
    out10[9] = st[8];
    return MI355_OK;
}

int mi355_yolo_raw_head(mi355_yolo* h, const uint8_t* bgr, int n, int height, int width, int row_stride, int imgsz,
                        float* out, int* out_channels, int* out_anchors) {
    if (!h || !out_channels || !out_anchors) return fail(MI355_EINVAL, "null argument");
    if (n <= 0 || height <= 0 || width <= 0) return fail(MI355_EINVAL, "n, height and width must be positive");
    RawHeadCall c;
    c.bgr = bgr; c.n = n; c.height = height; c.width = width; c.row_stride = row_stride;
    c.imgsz = imgsz; c.out = out; c.out_channels = out_channels; c.out_anchors = out_anchors;
    return raw_head_impl(h, c);
}

// ------------------------------------------------------------------------------------- single operators
int mi355_letterbox_shape(int height, int width, int imgsz, int* out_h, int* out_w) {
    if (!out_h || !out_w || height <= 0 || width <= 0 || imgsz <= 0) return fail(MI355_EINVAL, "bad argument");
    const Geometry g = make_geometry(height, width, imgsz);
    *out_h = g.Hl; *out_w = g.Wl;
    return MI355_OK;
}

// ------------------------------------------------------------------------------------- JPEG evidence frames (jpeg_kernels.hip)
int64_t mi355_jpeg_bound(int height, int width, int subsampling) {
    if (height < 1 || width < 1 || height > kJpegMaxSide || width > kJpegMaxSide || (subsampling != kJpeg420 && subsampling != kJpeg444)) return 0;
    return jpeg_bound(height, width, subsampling);
}

int mi355_jpeg_encode(int device, const mi355_render_frame* frames, int n, int quality, int subsampling, mi355_jpeg_out* outs, void* stream,
                      float* launch_ms) {
    if (!outs) return fail(MI355_EINVAL, "jpeg: null output");
    JpegCtx ctx;
    const int rc = jpeg_run(ctx, device, frames, n, quality, subsampling, outs, nullptr, (hipStream_t)stream, launch_ms);
    if (device >= 0) jpeg_ctx_free(ctx);
    return rc;
}

int mi355_yolo_encode(mi355_yolo* h, const mi355_render_frame* frames, int n, int quality, int subsampling, mi355_jpeg_out* outs, float* launch_ms) {
    if (!h) return fail(MI355_EINVAL, "jpeg: null handle");
    if (!outs) return fail(MI355_EINVAL, "jpeg: null output");
    std::vector<mi355_render_frame> last;
    if (!frames) {                                             // the frames of the handle's last call, where that call left them on the device
        if (h->last_frames.empty()) return fail(MI355_EINVAL, "jpeg: the handle has no frames of a last blocking infer call");
        if (n != (int)h->last_frames.size())
            return fail(MI355_EINVAL, "jpeg: n = " + std::to_string(n) + ", but the last call had " + std::to_string(h->last_frames.size()) + " frames");
        last.resize((size_t)n);
        for (int i = 0; i < n; ++i) {
            const mi355_yolo::LastFrame& f = h->last_frames[i];
            if (!f.p) return fail(MI355_EINVAL, "jpeg: frame " + std::to_string(i) + " of the last call is no longer on the device (a host call of more than two "
                                                "chunks keeps its last two): pass the frames again");
            last[i] = mi355_render_frame{f.p, f.h, f.w, f.pitch, 1};
        }
        frames = last.data();
    }
    HIPCHK(hipSetDevice(h->device));
    if (h->async_pending) { HIPCHK(hipStreamSynchronize(h->stream)); h->async_pending = false; }
    return jpeg_run(h->jpeg, h->device, frames, n, quality, subsampling, outs, nullptr, h->stream, launch_ms);
}

// ------------------------------------------------------------------------------------- JPEG ingest (jpeg_decode_kernels.hip)
int mi355_yolo_decode(mi355_yolo* h, mi355_jpeg_stream* streams, int n, int entropy, const mi355_render_out* outs, int* status, float* launch_ms) {
    if (!h) return fail(MI355_EINVAL, "jpeg decode: null handle");
    if (!outs) return fail(MI355_EINVAL, "jpeg decode: null output");
    HIPCHK(hipSetDevice(h->device));
    if (h->async_pending) { HIPCHK(hipStreamSynchronize(h->stream)); h->async_pending = false; }
    return jpeg_dec_call(&h->jpeg_dec, h->device, streams, n, entropy, outs, nullptr, status, h->stream, launch_ms);
}

}  // extern "C"
