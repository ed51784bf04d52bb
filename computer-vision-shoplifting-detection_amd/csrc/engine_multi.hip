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

// Descriptors + scale-back rows + resize tables (one pair per distinct shape) of the call's frames -> one host image.  Pure host
// arithmetic.  Host frames: the descriptors point into the two staging slots at `staged` (frame i in slot (i / nb) & 1, at
// mc.stage_off[i], rows w*3 apart); device frames: at the caller's pointers with the caller's row strides.
void multi_image(const MultiFrames& mf, const MultiCall& mc, int n, int nb, const uint8_t* staged, MultiImage& img) {
    std::vector<LetterboxFrame> desc(n);
    std::vector<float> geom((size_t)n * 7);
    std::vector<int> tabs;
    std::vector<std::array<int, 4>> seen;                 // (h0, w0) -> (xoff, yoff) of a table built for an earlier frame
    for (int i = 0; i < n; ++i) {
        const Geometry& g = mc.g[i];
        LetterboxFrame& f = desc[i];
        if (mf.on_device) { f.src = mf.frames[i]; f.row_stride = row_stride_of(mf, i); }
        else { f.src = staged + (size_t)((i / nb) & 1) * mc.slot_bytes + mc.stage_off[i]; f.row_stride = g.w0 * 3; }
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
    img.geom_off = round_up_sz((size_t)n * sizeof(LetterboxFrame), 256);
    img.tabs_off = img.geom_off + round_up_sz((size_t)n * 7 * sizeof(float), 256);
    img.tab_ints = tabs.size();
    img.bytes.assign(img.tabs_off + std::max<size_t>(tabs.size() * 4, 16), 0);
    std::memcpy(img.bytes.data(), desc.data(), (size_t)n * sizeof(LetterboxFrame));
    std::memcpy(img.bytes.data() + img.geom_off, geom.data(), geom.size() * 4);
    if (!tabs.empty()) std::memcpy(img.bytes.data() + img.tabs_off, tabs.data(), tabs.size() * 4);
}

// The call's image -> d_multi, with one asynchronous copy on the engine's stream unless the device buffer already holds exactly
// these bytes (the same cameras call after call).
int multi_upload(mi355_yolo* h, const MultiFrames& mf, int n, int nb, MultiCall& mc) {
    MultiImage img;
    multi_image(mf, mc, n, nb, h->d_in.p, img);
    const size_t bytes = img.bytes.size();
    const int grown = grow_or_fail(h->d_multi, bytes, "d_multi"); if (grown < 0) return MI355_EHIP;
    GROW(h->h_multi, bytes);
    if (grown) h->multi_bytes = 0;                        // a new block holds nothing of the last image
    if (h->multi_bytes != bytes || std::memcmp(h->h_multi.p, img.bytes.data(), bytes) != 0) {
        // the previous upload out of h_multi has completed: every infer / raw_head call synchronises the stream before it returns
        std::memcpy(h->h_multi.p, img.bytes.data(), bytes);
        HIPCHK(hipMemcpyAsync(h->d_multi.p, h->h_multi.p, bytes, hipMemcpyHostToDevice, h->stream));
        h->multi_bytes = bytes;
    }
    mc.d_desc = (const LetterboxFrame*)h->d_multi.p;
    mc.d_geom = (const float*)(h->d_multi.p + img.geom_off);
    mc.d_tabs = (const int*)(h->d_multi.p + img.tabs_off);
    return MI355_OK;
}

// Host frames of chunk [s0, s0 + m): packed into pinned staging slot `slot`, then ONE host-to-device copy into d_in's slot on the
// copy stream (after the kernels that read that slot last time have been passed, as for mi355_yolo_infer's chunks).
int multi_stage_chunk(mi355_yolo* h, const MultiFrames& mf, const MultiCall& mc, int s0, int m, int slot) {
    // a copy out of the old block may still be running on the copy stream: it must finish before the block is freed
    if (h->h_stage.p && h->h_stage.cap < mc.slot_bytes * 2) HIPCHK(hipStreamSynchronize(h->copy_stream));
    GROW(h->h_stage, mc.slot_bytes * 2);
    HIPCHK(hipEventSynchronize(h->ev_copied[slot]));      // the previous copy out of this pinned slot has finished
    uint8_t* dst = h->h_stage.p + (size_t)slot * mc.slot_bytes;
    size_t end = 0;
    for (int i = s0; i < s0 + m; ++i) {
        const size_t row = (size_t)mf.widths[i] * 3, rs = (size_t)row_stride_of(mf, i);
        uint8_t* d = dst + mc.stage_off[i];
        if (rs == row) std::memcpy(d, mf.frames[i], row * mf.heights[i]);
        else for (int y = 0; y < mf.heights[i]; ++y) std::memcpy(d + y * row, mf.frames[i] + y * rs, row);
        end = mc.stage_off[i] + row * mf.heights[i];
    }
    HIPCHK(hipStreamWaitEvent(h->copy_stream, h->ev_consumed[slot], 0));
    HIPCHK(hipMemcpyAsync(h->d_in.p + (size_t)slot * mc.slot_bytes, dst, end, hipMemcpyHostToDevice, h->copy_stream));
    HIPCHK(hipEventRecord(h->ev_copied[slot], h->copy_stream));
    return MI355_OK;
}

// frames [s0, s0 + m) of the call -> canvas (h->lbox) -> net + decode.  No hipGraph replay here (opts MI355_OPT_HIP_GRAPH covers
// the single-shape entry points).
int run_chunk_multi(mi355_yolo* h, Prof& pf, const MultiCall& mc, int s0, int m, bool full_pred) {
    LetterboxMultiArgs la{};
    la.frames = mc.d_desc + s0; la.tabs = mc.d_tabs; la.dst = h->lbox; la.Hd = mc.Hd; la.Wd = mc.Wd; la.B = m;
    TIMED(pf, K_LETTERBOX, launch_letterbox_multi(la, h->stream));
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
    InferCall c;
    c.multi = &mf; c.n = n;
    c.conf = conf; c.iou = iou; c.classes = classes; c.n_classes = n_classes; c.max_det = max_det; c.imgsz = imgsz;
    c.out_rows = out_rows; c.cap = cap; c.out_counts = out_counts;
    return infer_impl(h, c);
}

int mi355_yolo_raw_head_multi(mi355_yolo* h, const uint8_t* const* frames, const int* heights, const int* widths, const int* row_strides,
                              int frames_on_device, int n, int imgsz, float* out, int* out_channels, int* out_anchors) {
    if (!h || !out_channels || !out_anchors) return fail(MI355_EINVAL, "null argument");
    const MultiFrames mf{frames, heights, widths, row_strides, frames_on_device != 0};
    const int rc0 = multi_check(mf, n); if (rc0) return rc0;
    RawHeadCall c;
    c.multi = &mf; c.n = n; c.imgsz = imgsz; c.out = out; c.out_channels = out_channels; c.out_anchors = out_anchors;
    return raw_head_impl(h, c);
}

int mi355_op_letterbox_multi(int device_id, const uint8_t* const* frames, const int* heights, const int* widths, const int* row_strides,
                             int n, int imgsz, uint8_t* out) {
    const MultiFrames mf{frames, heights, widths, row_strides, false};
    int rc = multi_check(mf, n); if (rc) return rc;
    if (!out || imgsz <= 0 || (imgsz & 3)) return fail(MI355_EINVAL, "bad argument");
    HIPCHK(hipSetDevice(device_id));
    // the square canvas for every frame (auto = False), whatever the shapes: the kernel a mixed batch runs.  All n frames are one
    // chunk, staged in one slot.
    MultiCall mc;
    mc.Hd = mc.Wd = imgsz; mc.g.resize(n); mc.stage_off.resize(n);
    for (int i = 0; i < n; ++i) {
        mc.g[i] = make_geometry(heights[i], widths[i], imgsz, false);
        mc.stage_off[i] = mc.slot_bytes; mc.slot_bytes += round_up_sz((size_t)heights[i] * widths[i] * 3, 256);
    }
    DevMem dm; uint8_t *d_src, *d_dst, *d_img;
    const size_t db = (size_t)n * imgsz * imgsz * 3;
    HIPCHK(dm.alloc(&d_src, mc.slot_bytes)); HIPCHK(dm.alloc(&d_dst, db));
    MultiImage img;
    multi_image(mf, mc, n, n, d_src, img);
    HIPCHK(dm.alloc(&d_img, img.bytes.size()));
    for (int i = 0; i < n; ++i)
        HIPCHK(hipMemcpy2D(d_src + mc.stage_off[i], (size_t)widths[i] * 3, frames[i], (size_t)row_stride_of(mf, i), (size_t)widths[i] * 3,
                           (size_t)heights[i], hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_img, img.bytes.data(), img.bytes.size(), hipMemcpyHostToDevice));
    LetterboxMultiArgs la{};
    la.frames = (const LetterboxFrame*)d_img; la.tabs = (const int*)(d_img + img.tabs_off); la.dst = d_dst; la.Hd = imgsz; la.Wd = imgsz; la.B = n;
    KCHK(launch_letterbox_multi(la, nullptr));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, d_dst, db, hipMemcpyDeviceToHost));
    return MI355_OK;
}

}  // extern "C"
