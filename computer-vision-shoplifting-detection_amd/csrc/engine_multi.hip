// One call over frames of different sizes (several cameras at different resolutions): Ultralytics' BasePredictor.pre_transform
// letterboxes such a batch to the square imgsz x imgsz canvas (LetterBox auto=False) and scales every frame's rows back against
// its own shape.  The per-frame geometry lives in one device buffer (descriptors for letterbox_multi_kernel, scale-back constants
// for the NMS epilogue, resize tables); the net runs once on [n][imgsz][imgsz][3].  All frames the same shape: the rect geometry
// of mi355_yolo_infer, so the rows equal that call's on the stacked frames.
#include "engine_internal.h"

namespace mi355 {

int multi_check(const MultiFrames& mf, int n) {
    if (n <= 0) return fail(MI355_EINVAL, "n must be positive");
    if (!mf.frames || !mf.heights || !mf.widths) return fail(MI355_EINVAL, "null argument");
    for (int i = 0; i < n; ++i) {
        if (!mf.frames[i]) return fail(MI355_EINVAL, "null frame pointer");
        if (mf.heights[i] <= 0 || mf.widths[i] <= 0) return fail(MI355_EINVAL, "frame height and width must be positive");
        const int rs = mf.row_strides ? mf.row_strides[i] : 0;
        if (rs != 0 && rs < mf.widths[i] * 3) return fail(MI355_EINVAL, "row_stride_bytes smaller than a row");
    }
    return MI355_OK;
}

static int row_stride_of(const MultiFrames& mf, int i) {
    const int rs = mf.row_strides ? mf.row_strides[i] : 0;
    return rs ? rs : mf.widths[i] * 3;
}

void multi_prepare(const MultiFrames& mf, int n, int nb, int imgsz, MultiCall& mc) {
    bool same = true;
    for (int i = 1; i < n; ++i) same = same && mf.heights[i] == mf.heights[0] && mf.widths[i] == mf.widths[0];
    mc.g.resize(n);
    for (int i = 0; i < n; ++i) mc.g[i] = make_geometry(mf.heights[i], mf.widths[i], imgsz, same);
    mc.Hd = same ? mc.g[0].Hl : imgsz;
    mc.Wd = same ? mc.g[0].Wl : imgsz;
    mc.stage_off.assign(n, 0);
    mc.slot_bytes = 0;
    for (int s = 0; s < n; s += nb) {                     // host frames: chunk by chunk, packed (rows w*3 apart) in frame order
        size_t at = 0;
        for (int i = s; i < std::min(n, s + nb); ++i) { mc.stage_off[i] = at; at += round_up_sz((size_t)mf.heights[i] * mf.widths[i] * 3, 256); }
        mc.slot_bytes = std::max(mc.slot_bytes, at);
    }
}

// Descriptors + scale-back rows + tables -> one host image; uploaded with one asynchronous copy on the engine's stream unless the
// device buffer already holds exactly these bytes.  Host frames: the descriptors point into the staging slots of d_in.
int multi_upload(mi355_yolo* h, const MultiFrames& mf, int n, int nb, MultiCall& mc) {
    const size_t desc_bytes = round_up_sz((size_t)n * sizeof(LetterboxFrame), 256);
    const size_t geom_bytes = round_up_sz((size_t)n * 7 * sizeof(float), 256);
    std::vector<LetterboxFrame> desc(n);
    std::vector<float> geom((size_t)n * 7);
    std::vector<int> tabs;
    std::vector<std::array<int, 4>> seen;                 // (h0, w0) -> (xoff, yoff) of a table built for an earlier frame
    for (int i = 0; i < n; ++i) {
        const Geometry& g = mc.g[i];
        LetterboxFrame& f = desc[i];
        if (mf.on_device) { f.src = mf.frames[i]; f.row_stride = row_stride_of(mf, i); }
        else {
            const int slot = (i / nb) & 1;
            f.src = h->d_in + (size_t)slot * mc.slot_bytes + mc.stage_off[i]; f.row_stride = g.w0 * 3;
        }
        f.H = g.h0; f.W = g.w0; f.Hr = g.Hr; f.Wr = g.Wr; f.top = g.top; f.left = g.left;
        f.resize = g.resize ? 1 : 0; f.xoff = f.yoff = 0; f.pad_ = 0;
        if (g.resize) {
            int k = -1;
            for (size_t j = 0; j < seen.size(); ++j) if (seen[j][0] == g.h0 && seen[j][1] == g.w0) k = (int)j;
            if (k < 0) {
                std::vector<int> xt, yt;
                resize_table(g.Wr, g.w0, xt); resize_table(g.Hr, g.h0, yt);
                const int xo = (int)tabs.size(); tabs.insert(tabs.end(), xt.begin(), xt.end());
                const int yo = (int)tabs.size(); tabs.insert(tabs.end(), yt.begin(), yt.end());
                seen.push_back({g.h0, g.w0, xo, yo}); k = (int)seen.size() - 1;
            }
            f.xoff = seen[k][2]; f.yoff = seen[k][3];
        }
        float* r = &geom[(size_t)i * 7];
        r[0] = (float)g.gain; r[1] = (float)g.pad_x; r[2] = (float)g.pad_y; r[3] = (float)g.kpad_x; r[4] = (float)g.kpad_y;
        r[5] = (float)g.w0; r[6] = (float)g.h0;
    }
    const size_t bytes = desc_bytes + geom_bytes + std::max<size_t>(tabs.size() * 4, 16);
    if (h->multi_cap < bytes) {
        if (h->d_multi) (void)hipFree(h->d_multi); if (h->h_multi) (void)hipHostFree(h->h_multi);
        h->d_multi = nullptr; h->h_multi = nullptr; h->multi_cap = h->multi_bytes = 0;
        HIPCHK(hipMalloc(&h->d_multi, bytes)); HIPCHK(hipHostMalloc(&h->h_multi, bytes));
        h->multi_cap = bytes;
    }
    std::vector<char> img(bytes, 0);
    std::memcpy(img.data(), desc.data(), (size_t)n * sizeof(LetterboxFrame));
    std::memcpy(img.data() + desc_bytes, geom.data(), geom.size() * 4);
    if (!tabs.empty()) std::memcpy(img.data() + desc_bytes + geom_bytes, tabs.data(), tabs.size() * 4);
    if (h->multi_bytes != bytes || std::memcmp(h->h_multi, img.data(), bytes) != 0) {
        // the previous upload out of h_multi has completed: every infer / raw_head call synchronises the stream before it returns
        std::memcpy(h->h_multi, img.data(), bytes);
        HIPCHK(hipMemcpyAsync(h->d_multi, h->h_multi, bytes, hipMemcpyHostToDevice, h->stream));
        h->multi_bytes = bytes;
    }
    mc.d_desc = (const LetterboxFrame*)h->d_multi;
    mc.d_geom = (const float*)(h->d_multi + desc_bytes);
    mc.d_tabs = (const int*)(h->d_multi + desc_bytes + geom_bytes);
    return MI355_OK;
}

// Host frames of chunk [s0, s0 + m): packed into pinned staging slot `slot`, then ONE host-to-device copy into d_in's slot on the
// copy stream (after the kernels that read that slot last time have been passed, as for mi355_yolo_infer's chunks).
int multi_stage_chunk(mi355_yolo* h, const MultiFrames& mf, const MultiCall& mc, int s0, int m, int nb, int slot) {
    (void)nb;
    if (h->h_stage_bytes < mc.slot_bytes * 2) {
        if (h->h_stage) { HIPCHK(hipStreamSynchronize(h->copy_stream)); (void)hipHostFree(h->h_stage); }
        h->h_stage = nullptr; h->h_stage_bytes = 0;
        HIPCHK(hipHostMalloc(&h->h_stage, mc.slot_bytes * 2)); h->h_stage_bytes = mc.slot_bytes * 2;
    }
    HIPCHK(hipEventSynchronize(h->ev_copied[slot]));      // the previous copy out of this pinned slot has finished
    uint8_t* dst = h->h_stage + (size_t)slot * mc.slot_bytes;
    size_t end = 0;
    for (int i = s0; i < s0 + m; ++i) {
        const size_t row = (size_t)mf.widths[i] * 3, rs = (size_t)row_stride_of(mf, i);
        uint8_t* d = dst + mc.stage_off[i];
        if (rs == row) std::memcpy(d, mf.frames[i], row * mf.heights[i]);
        else for (int y = 0; y < mf.heights[i]; ++y) std::memcpy(d + y * row, mf.frames[i] + y * rs, row);
        end = mc.stage_off[i] + row * mf.heights[i];
    }
    HIPCHK(hipStreamWaitEvent(h->copy_stream, h->ev_consumed[slot], 0));
    HIPCHK(hipMemcpyAsync(h->d_in + (size_t)slot * mc.slot_bytes, dst, end, hipMemcpyHostToDevice, h->copy_stream));
    HIPCHK(hipEventRecord(h->ev_copied[slot], h->copy_stream));
    return MI355_OK;
}

// frames [s0, s0 + m) of the call -> canvas (h->lbox) -> net + decode.  No hipGraph replay here (opts MI355_OPT_HIP_GRAPH covers
// the single-shape entry points).
int run_chunk_multi(mi355_yolo* h, Prof& pf, const MultiCall& mc, int s0, int m, bool full_pred) {
    LetterboxMultiArgs la{};
    la.frames = mc.d_desc + s0; la.tabs = mc.d_tabs; la.dst = h->lbox; la.Hd = mc.Hd; la.Wd = mc.Wd; la.B = m;
    if (pf.begin(K_LETTERBOX)) return fail(MI355_EHIP, "event");
    KCHK(launch_letterbox_multi(la, h->stream));
    pf.end();
    Geometry gc{};                                        // launch_net reads the canvas size only
    gc.Hl = mc.Hd; gc.Wl = mc.Wd;
    return launch_net(h, pf, h->lbox, m, gc, full_pred);
}

}  // namespace mi355

using namespace mi355;

extern "C" {

int mi355_letterbox_geometry(int h0, int w0, int imgsz, int auto_pad, int* i6, double* d5) {
    if (!i6 || !d5 || h0 <= 0 || w0 <= 0 || imgsz <= 0) return fail(MI355_EINVAL, "bad argument");
    const Geometry g = make_geometry(h0, w0, imgsz, auto_pad != 0);
    i6[0] = g.Hl; i6[1] = g.Wl; i6[2] = g.Hr; i6[3] = g.Wr; i6[4] = g.top; i6[5] = g.left;
    d5[0] = g.gain; d5[1] = g.pad_x; d5[2] = g.pad_y; d5[3] = g.kpad_x; d5[4] = g.kpad_y;
    return MI355_OK;
}

int mi355_yolo_infer_multi(mi355_yolo* h, const uint8_t* const* frames, const int* heights, const int* widths, const int* row_strides,
                           int frames_on_device, int n, float conf, float iou, const int* classes, int n_classes, int max_det, int imgsz,
                           mi355_det* out_rows, int cap, int* out_counts) {
    const MultiFrames mf{frames, heights, widths, row_strides, frames_on_device != 0};
    return infer_impl(h, nullptr, frames_on_device != 0, n, 1, 1, 0, conf, iou, classes, n_classes, max_det, imgsz, out_rows, cap,
                      out_counts, nullptr, nullptr, nullptr, &mf);
}

int mi355_yolo_raw_head_multi(mi355_yolo* h, const uint8_t* const* frames, const int* heights, const int* widths, const int* row_strides,
                              int frames_on_device, int n, int imgsz, float* out, int* out_channels, int* out_anchors) {
    if (!h || !out_channels || !out_anchors) return fail(MI355_EINVAL, "null argument");
    const MultiFrames mf{frames, heights, widths, row_strides, frames_on_device != 0};
    int rc = multi_check(mf, n); if (rc) return rc;
    if (imgsz <= 0) imgsz = 640;
    if (imgsz % 32) return fail(MI355_EINVAL, "imgsz must be a multiple of 32");
    const int nb = std::min(n, h->chunk);
    MultiCall mc;
    multi_prepare(mf, n, nb, imgsz, mc);
    int A = 0;
    for (const FileLevel& lv : h->levels) A += (mc.Hd / lv.stride) * (mc.Wd / lv.stride);
    *out_channels = h->no(); *out_anchors = A;
    if (!out) return MI355_OK;
    HIPCHK(hipSetDevice(h->device));
    if (h->async_pending) { HIPCHK(hipStreamSynchronize(h->stream)); h->async_pending = false; }
    rc = ensure_shape(h, nb, mc.Hd, mc.Wd); if (rc) return rc;
    if (!mf.on_device && h->d_in_bytes < mc.slot_bytes * 2) {
        if (h->d_in) (void)hipFree(h->d_in);
        h->d_in = nullptr; h->d_in_bytes = 0;
        HIPCHK(hipMalloc(&h->d_in, mc.slot_bytes * 2)); h->d_in_bytes = mc.slot_bytes * 2;
    }
    rc = multi_upload(h, mf, n, nb, mc); if (rc) return rc;
    const size_t per = (size_t)A * h->no();
    if (h->rawhead_floats < per * nb) {
        if (h->d_rawhead) (void)hipFree(h->d_rawhead); h->d_rawhead = nullptr; h->rawhead_floats = 0;
        HIPCHK(hipMalloc(&h->d_rawhead, per * nb * 4)); h->rawhead_floats = per * nb;
    }
    Prof pf{h};
    const bool was = h->profiling; h->profiling = false;
    for (int s = 0, ci = 0; s < n; s += nb, ++ci) {
        const int m = std::min(nb, n - s);
        if (!mf.on_device) {
            HIPCHK(hipEventRecord(h->ev_consumed[ci & 1], h->stream));
            rc = multi_stage_chunk(h, mf, mc, s, m, nb, ci & 1);
            if (!rc) { const hipError_t e = hipStreamWaitEvent(h->stream, h->ev_copied[ci & 1], 0); if (e != hipSuccess) rc = fail(MI355_EHIP, hipGetErrorString(e)); }
        }
        if (!rc) rc = run_chunk_multi(h, pf, mc, s, m, true);
        if (rc) { h->profiling = was; return rc; }
        KCHK(launch_transpose_pred(h->pred, h->d_rawhead, m, A, h->no(), h->stream));
        HIPCHK(hipMemcpyAsync(out + (size_t)s * per, h->d_rawhead, per * m * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    h->profiling = was;
    return MI355_OK;
}

int mi355_op_letterbox_multi(int device_id, const uint8_t* const* frames, const int* heights, const int* widths, const int* row_strides,
                             int n, int imgsz, uint8_t* out) {
    const MultiFrames mf{frames, heights, widths, row_strides, false};
    int rc = multi_check(mf, n); if (rc) return rc;
    if (!out || imgsz <= 0 || (imgsz & 3)) return fail(MI355_EINVAL, "bad argument");
    HIPCHK(hipSetDevice(device_id));
    // the square canvas for every frame (auto = False), whatever the shapes: the kernel a mixed batch runs
    std::vector<Geometry> g(n);
    std::vector<size_t> off(n);
    size_t src_bytes = 0;
    for (int i = 0; i < n; ++i) {
        g[i] = make_geometry(heights[i], widths[i], imgsz, false);
        off[i] = src_bytes; src_bytes += round_up_sz((size_t)heights[i] * widths[i] * 3, 256);
    }
    std::vector<LetterboxFrame> desc(n);
    std::vector<int> tabs;
    for (int i = 0; i < n; ++i) {
        LetterboxFrame& f = desc[i];
        f = LetterboxFrame{};
        f.H = g[i].h0; f.W = g[i].w0; f.row_stride = g[i].w0 * 3; f.Hr = g[i].Hr; f.Wr = g[i].Wr; f.top = g[i].top; f.left = g[i].left;
        f.resize = g[i].resize ? 1 : 0;
        if (g[i].resize) {
            std::vector<int> xt, yt;
            resize_table(g[i].Wr, g[i].w0, xt); resize_table(g[i].Hr, g[i].h0, yt);
            f.xoff = (int)tabs.size(); tabs.insert(tabs.end(), xt.begin(), xt.end());
            f.yoff = (int)tabs.size(); tabs.insert(tabs.end(), yt.begin(), yt.end());
        }
    }
    DevMem dm; uint8_t *d_src, *d_dst; int* d_tabs; LetterboxFrame* d_desc;
    const size_t db = (size_t)n * imgsz * imgsz * 3;
    HIPCHK(dm.alloc(&d_src, src_bytes)); HIPCHK(dm.alloc(&d_dst, db));
    HIPCHK(dm.alloc(&d_tabs, tabs.size() * 4)); HIPCHK(dm.alloc(&d_desc, desc.size() * sizeof(LetterboxFrame)));
    for (int i = 0; i < n; ++i) {
        desc[i].src = d_src + off[i];
        HIPCHK(hipMemcpy2D(d_src + off[i], (size_t)widths[i] * 3, frames[i], (size_t)row_stride_of(mf, i), (size_t)widths[i] * 3,
                           (size_t)heights[i], hipMemcpyHostToDevice));
    }
    if (!tabs.empty()) HIPCHK(hipMemcpy(d_tabs, tabs.data(), tabs.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_desc, desc.data(), desc.size() * sizeof(LetterboxFrame), hipMemcpyHostToDevice));
    LetterboxMultiArgs la{};
    la.frames = d_desc; la.tabs = d_tabs; la.dst = d_dst; la.Hd = imgsz; la.Wd = imgsz; la.B = n;
    KCHK(launch_letterbox_multi(la, nullptr));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, d_dst, db, hipMemcpyDeviceToHost));
    return MI355_OK;
}

}  // extern "C"
