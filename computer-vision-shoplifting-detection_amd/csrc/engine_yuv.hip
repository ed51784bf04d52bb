// NV12 / I420 frames at ingest: the argument checks, the packed staging of host planes, the per-frame conversion
// descriptors of a call and the one conversion launch per chunk that infer_impl (engine_run.hip) puts in front of run_chunk /
// run_chunk_multi; the three entry points of include/mi355_yolo.h.  The kernel and its host twin are yuv_kernels.hip.
#include "engine_internal.h"

namespace mi355 {

static size_t chroma_row(const mi355_yuv_frame& f) { return f.format == MI355_PIX_NV12 ? (size_t)f.width : (size_t)f.width / 2; }
static int chroma_planes(const mi355_yuv_frame& f) { return f.format == MI355_PIX_NV12 ? 1 : 2; }

int yuv_check(const mi355_yuv_frame* frames, int n) {
    if (n <= 0) return fail(MI355_EINVAL, "n must be positive");
    if (!frames) return fail(MI355_EINVAL, "frames is null");
    for (int i = 0; i < n; ++i) {
        const mi355_yuv_frame& f = frames[i];
        const std::string at = "frames[" + std::to_string(i) + "].";
        if (f.format != MI355_PIX_NV12 && f.format != MI355_PIX_I420)
            return fail(MI355_EINVAL, at + "format = " + std::to_string(f.format) + " is neither MI355_PIX_NV12 nor MI355_PIX_I420");
        if (!f.y) return fail(MI355_EINVAL, at + "y is null");
        if (!f.u) return fail(MI355_EINVAL, at + "u is null");
        if (f.format == MI355_PIX_I420 && !f.v) return fail(MI355_EINVAL, at + "v is null (I420 has a V plane of its own)");
        if (f.height <= 0 || (f.height & 1)) return fail(MI355_EINVAL, at + "height = " + std::to_string(f.height) + " must be positive and even");
        if (f.width <= 0 || (f.width & 1)) return fail(MI355_EINVAL, at + "width = " + std::to_string(f.width) + " must be positive and even");
        if (f.y_stride < f.width) return fail(MI355_EINVAL, at + "y_stride = " + std::to_string(f.y_stride) + " is smaller than a row of Y");
        if ((size_t)f.uv_stride < chroma_row(f) || f.uv_stride < 0)
            return fail(MI355_EINVAL, at + "uv_stride = " + std::to_string(f.uv_stride) + " is smaller than a row of chroma");
    }
    return MI355_OK;
}

YuvFrameDesc yuv_desc(const mi355_yuv_frame& f, uint8_t* dst) {
    YuvFrameDesc d{};
    d.y = f.y; d.u = f.u; d.v = f.format == MI355_PIX_I420 ? f.v : nullptr; d.dst = dst;
    d.H = f.height; d.W = f.width; d.y_stride = f.y_stride; d.uv_stride = f.uv_stride; d.format = f.format;
    d.vec = yuv_vector_ok(d) ? 1 : 0;
    return d;
}

// frame f's planes packed at `base`: Y rows width bytes apart, then the chroma plane(s), rows chroma_row apart
static mi355_yuv_frame packed_at(const mi355_yuv_frame& f, const uint8_t* base) {
    mi355_yuv_frame p = f;
    p.y = base; p.u = base + (size_t)f.height * f.width;
    p.v = f.format == MI355_PIX_I420 ? p.u + (size_t)(f.height / 2) * (f.width / 2) : nullptr;
    p.y_stride = f.width; p.uv_stride = (int)chroma_row(f);
    return p;
}

static void copy_rows(uint8_t* dst, const uint8_t* src, size_t row, size_t stride, int rows) {
    if (stride == row) { std::memcpy(dst, src, row * rows); return; }
    for (int y = 0; y < rows; ++y) std::memcpy(dst + y * row, src + y * stride, row);
}

void yuv_layout(const mi355_yuv_frame* frames, int n, int nb, YuvCall& yc) {
    yc.plane_off.assign(n, 0);
    yc.yuv_slot_bytes = 0;
    for (int s = 0; s < n; s += nb) {                     // chunk by chunk, 1.5 bytes per pixel, frame starts 256-byte aligned
        size_t at = 0;
        for (int i = s; i < std::min(n, s + nb); ++i) { yc.plane_off[i] = at; at += round_up_sz((size_t)frames[i].height * frames[i].width * 3 / 2, 256); }
        yc.yuv_slot_bytes = std::max(yc.yuv_slot_bytes, at);
    }
}

// The call's n descriptors -> d_yuvdesc, one asynchronous copy on the engine's stream out of their pinned image (which the launches size
// their grids from).  Frame i converts into slot (i / nb) & 1 of d_in; host planes are read from the same slot of d_yuv.
int yuv_upload(mi355_yolo* h, const mi355_yuv_frame* frames, bool on_device, int n, int nb, size_t bgr_slot_bytes, YuvCall& yc) {
    const size_t bytes = (size_t)n * sizeof(YuvFrameDesc);
    GROW(h->d_yuvdesc, bytes); GROW(h->h_yuvdesc, bytes);
    if (!on_device) GROW(h->d_yuv, 2 * yc.yuv_slot_bytes);
    YuvFrameDesc* hd = (YuvFrameDesc*)h->h_yuvdesc.p;
    for (int i = 0; i < n; ++i) {
        const size_t slot = (size_t)((i / nb) & 1);
        uint8_t* dst = h->d_in.p + slot * bgr_slot_bytes + yc.bgr_off[i];
        hd[i] = on_device ? yuv_desc(frames[i], dst) : yuv_desc(packed_at(frames[i], h->d_yuv.p + slot * yc.yuv_slot_bytes + yc.plane_off[i]), dst);
    }
    // the previous upload out of the pinned image has completed: a synchronous call synchronises the stream before it returns, and
    // infer_impl waits for an asynchronous one before it gets here
    HIPCHK(hipMemcpyAsync(h->d_yuvdesc.p, hd, bytes, hipMemcpyHostToDevice, h->stream));
    yc.d_desc = (const YuvFrameDesc*)h->d_yuvdesc.p;
    return MI355_OK;
}

// Host planes of chunk [s0, s0 + m): packed into pinned staging slot `slot`, then ONE host-to-device copy into d_yuv's slot on the copy
// stream (after the conversion launch that read that slot last time has been passed) -- multi_stage_chunk's hand-over.
int yuv_stage_chunk(mi355_yolo* h, const mi355_yuv_frame* frames, const YuvCall& yc, int s0, int m, int slot) {
    if (h->h_stage.p && h->h_stage.cap < yc.yuv_slot_bytes * 2) HIPCHK(hipStreamSynchronize(h->copy_stream));
    GROW(h->h_stage, yc.yuv_slot_bytes * 2);
    HIPCHK(hipEventSynchronize(h->ev_copied[slot]));      // the previous copy out of this pinned slot has finished
    uint8_t* dst = h->h_stage.p + (size_t)slot * yc.yuv_slot_bytes;
    size_t end = 0;
    for (int i = s0; i < s0 + m; ++i) {
        const mi355_yuv_frame& f = frames[i];
        const mi355_yuv_frame p = packed_at(f, dst + yc.plane_off[i]);
        copy_rows((uint8_t*)p.y, f.y, (size_t)f.width, (size_t)f.y_stride, f.height);
        copy_rows((uint8_t*)p.u, f.u, chroma_row(f), (size_t)f.uv_stride, f.height / 2);
        if (p.v) copy_rows((uint8_t*)p.v, f.v, chroma_row(f), (size_t)f.uv_stride, f.height / 2);
        end = yc.plane_off[i] + (size_t)f.height * f.width * 3 / 2;
    }
    HIPCHK(hipStreamWaitEvent(h->copy_stream, h->ev_consumed[slot], 0));
    HIPCHK(hipMemcpyAsync(h->d_yuv.p + (size_t)slot * yc.yuv_slot_bytes, dst, end, hipMemcpyHostToDevice, h->copy_stream));
    HIPCHK(hipEventRecord(h->ev_copied[slot], h->copy_stream));
    return MI355_OK;
}

// frames [s0, s0 + m) -> BGR in their d_in slot: one launch, timed as preprocess
int yuv_convert_chunk(mi355_yolo* h, Prof& pf, const YuvCall& yc, int s0, int m) {
    TIMED(pf, K_LETTERBOX, launch_yuv_to_bgr(yc.d_desc + s0, (const YuvFrameDesc*)h->h_yuvdesc.p + s0, m, h->stream));
    return MI355_OK;
}

}  // namespace mi355

using namespace mi355;

extern "C" {

int mi355_yolo_infer_yuv(mi355_yolo* h, const mi355_yuv_frame* frames, int frames_on_device, int n, float conf, float iou,
                         const int* classes, int n_classes, int max_det, int imgsz, mi355_det* out_rows, int cap, int* out_counts) {
    InferCall c;
    c.yuv = frames; c.on_device = frames_on_device != 0; c.n = n;
    c.conf = conf; c.iou = iou; c.classes = classes; c.n_classes = n_classes; c.max_det = max_det; c.imgsz = imgsz;
    c.out_rows = out_rows; c.cap = cap; c.out_counts = out_counts;
    return infer_impl(h, c);
}

int mi355_yolo_infer_yuv_device_async(mi355_yolo* h, const mi355_yuv_frame* frames, int n, float conf, float iou, const int* classes,
                                      int n_classes, int max_det, int imgsz, mi355_det* rows_dev, int* counts_dev, int* total_dev) {
    if (!rows_dev) return fail(MI355_EINVAL, "null argument");
    const int rc = yuv_check(frames, n); if (rc) return rc;
    for (int i = 1; i < n; ++i)
        if (frames[i].height != frames[0].height || frames[i].width != frames[0].width)
            return fail(MI355_EINVAL, "frames[" + std::to_string(i) + "]: the asynchronous call takes frames of one size");
    InferCall c;
    c.yuv = frames; c.on_device = true; c.n = n;
    c.conf = conf; c.iou = iou; c.classes = classes; c.n_classes = n_classes; c.max_det = max_det; c.imgsz = imgsz;
    c.dev_rows = rows_dev; c.dev_counts = counts_dev; c.dev_total = total_dev;
    return infer_impl(h, c);
}

int mi355_op_yuv_to_bgr(int device_id, const mi355_yuv_frame* frames, int n, uint8_t* const* bgr_out) {
    const int rc = yuv_check(frames, n); if (rc) return rc;
    if (!bgr_out) return fail(MI355_EINVAL, "bgr_out is null");
    for (int i = 0; i < n; ++i) if (!bgr_out[i]) return fail(MI355_EINVAL, "bgr_out[" + std::to_string(i) + "] is null");
    std::vector<YuvFrameDesc> desc(n);
    if (device_id < 0) {
        for (int i = 0; i < n; ++i) desc[i] = yuv_desc(frames[i], bgr_out[i]);
        yuv_to_bgr_host(desc.data(), n);
        return MI355_OK;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(MI355_EHIP, "no HIP device: the conversion kernel needs an MI355X (device_id = -1 runs its host twin)");
    if (device_id >= ndev) return fail(MI355_EINVAL, "device_id out of range");
    HIPCHK(hipSetDevice(device_id));
    // every plane at a 256-byte aligned start + its host address modulo 16, rows its own stride apart; every output 256-byte aligned with at least 64 guard bytes behind it
    constexpr size_t GUARD = 64; constexpr uint8_t SENTINEL = 0xA5;
    auto span = [](size_t stride, int rows) { return stride * (size_t)rows; };
    struct Place { size_t y, u, v, dst; };
    std::vector<Place> at(n);
    size_t in_bytes = 0, out_bytes = 0;
    auto place = [&](const uint8_t* host, size_t bytes) { const size_t o = in_bytes + ((size_t)host & 15); in_bytes = round_up_sz(o + bytes, 256); return o; };
    for (int i = 0; i < n; ++i) {
        const mi355_yuv_frame& f = frames[i];
        at[i].y = place(f.y, span((size_t)f.y_stride, f.height));
        at[i].u = place(f.u, span((size_t)f.uv_stride, f.height / 2));
        at[i].v = chroma_planes(f) == 2 ? place(f.v, span((size_t)f.uv_stride, f.height / 2)) : 0;
        at[i].dst = out_bytes; out_bytes = round_up_sz(out_bytes + (size_t)f.height * f.width * 3 + GUARD, 256);
    }
    DevMem dm; uint8_t *d_in, *d_out; YuvFrameDesc* d_desc;
    HIPCHK(dm.alloc(&d_in, in_bytes)); HIPCHK(dm.alloc(&d_out, out_bytes)); HIPCHK(dm.alloc(&d_desc, (size_t)n * sizeof(YuvFrameDesc)));
    HIPCHK(hipMemset(d_out, SENTINEL, out_bytes));
    for (int i = 0; i < n; ++i) {
        mi355_yuv_frame f = frames[i];
        HIPCHK(hipMemcpy2D(d_in + at[i].y, (size_t)f.y_stride, f.y, (size_t)f.y_stride, (size_t)f.width, (size_t)f.height, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy2D(d_in + at[i].u, (size_t)f.uv_stride, f.u, (size_t)f.uv_stride, chroma_row(f), (size_t)f.height / 2, hipMemcpyHostToDevice));
        if (chroma_planes(f) == 2)
            HIPCHK(hipMemcpy2D(d_in + at[i].v, (size_t)f.uv_stride, f.v, (size_t)f.uv_stride, chroma_row(f), (size_t)f.height / 2, hipMemcpyHostToDevice));
        f.y = d_in + at[i].y; f.u = d_in + at[i].u; f.v = chroma_planes(f) == 2 ? d_in + at[i].v : nullptr;
        desc[i] = yuv_desc(f, d_out + at[i].dst);
    }
    HIPCHK(hipMemcpy(d_desc, desc.data(), (size_t)n * sizeof(YuvFrameDesc), hipMemcpyHostToDevice));
    KCHK(launch_yuv_to_bgr(d_desc, desc.data(), n, nullptr));
    HIPCHK(hipDeviceSynchronize());
    std::vector<uint8_t> back(out_bytes);
    HIPCHK(hipMemcpy(back.data(), d_out, out_bytes, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) {
        const size_t bytes = (size_t)frames[i].height * frames[i].width * 3;
        const size_t end = i + 1 < n ? at[i + 1].dst : out_bytes;
        for (size_t k = at[i].dst + bytes; k < end; ++k)
            if (back[k] != SENTINEL) return fail(MI355_EHIP, "yuv_to_bgr wrote beyond frame " + std::to_string(i) + "'s " + std::to_string(bytes) + " bytes");
        std::memcpy(bgr_out[i], back.data() + at[i].dst, bytes);
    }
    return MI355_OK;
}

}  // extern "C"
