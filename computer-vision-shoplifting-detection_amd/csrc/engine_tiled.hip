// Tiled predict for high-resolution frames: the tile grid, the entry list of a call (every frame's tiles, then the
// frame itself), the single upload of host frames, and the merge of the per-entry rows behind the last chunk's NMS -- launched here,
// the kernel is post_kernels.hip's tile_merge_kernel; its host twin (mi355_op_tile_merge with device = -1) is below.  The detector
// pass itself is infer_impl's (engine_run.hip) over the entry list as an on-device mixed-shape call: no case is special.
#include "engine_internal.h"
#include "tile_merge.h"

#pragma clang fp contract(off)

namespace mi355 {

// positions of the tiles along one axis (the rule of include/mi355_yolo.h); every tile's extent is min(t, L)
static void tile_axis(int L, int t, int o, std::vector<int>& pos) {
    pos.clear();
    int p = 0;
    while (p + t < L) { pos.push_back(p); p += t - o; }
    pos.push_back(std::max(0, L - t));
}

static int grid_check(int height, int width, int th, int tw, int oy, int ox) {
    if (height <= 0 || width <= 0) return fail(MI355_EINVAL, "tile grid: height and width must be positive");
    if (th <= 0 || tw <= 0) return fail(MI355_EINVAL, "tile grid: tile must be positive");
    if (oy < 0 || oy >= th || ox < 0 || ox >= tw) return fail(MI355_EINVAL, "tile grid: overlap must be in [0, tile) pixels");
    return MI355_OK;
}

static void tile_grid(int height, int width, int th, int tw, int oy, int ox, std::vector<int>& xywh) {
    std::vector<int> ys, xs;
    tile_axis(height, th, oy, ys); tile_axis(width, tw, ox, xs);
    const int eh = std::min(th, height), ew = std::min(tw, width);
    xywh.clear();
    for (int y : ys) for (int x : xs) { xywh.push_back(x); xywh.push_back(y); xywh.push_back(ew); xywh.push_back(eh); }
}

// The kernel's per-frame routine in plain host C++: the same keys, the same order, the same expressions (tile_merge.h).
static void tile_merge_host(const TileMergeArgs& a) {
    std::vector<unsigned long long> keys;
    std::vector<TileBox> kept; std::vector<int> kcl, ksl;
    for (int f = 0; f < a.n_frames; ++f) {
        const int e0 = a.entry_off ? a.entry_off[f] : f * a.entries;
        const int E = a.entry_off ? a.entry_off[f + 1] - e0 : a.entries;
        const unsigned* rows = a.rows + (size_t)e0 * a.max_det * TILE_ROW_WORDS;
        keys.clear(); kept.clear(); kcl.clear(); ksl.clear();
        for (int e = 0; e < E; ++e) {
            const int cnt = std::min(std::max(a.counts[e0 + e], 0), a.max_det);
            for (int r = 0; r < cnt; ++r) {
                const unsigned slot = (unsigned)(e * a.max_det + r);
                keys.push_back(((unsigned long long)(~rows[(size_t)slot * TILE_ROW_WORDS + 4]) << 32) | slot);
            }
        }
        std::sort(keys.begin(), keys.end());
        for (size_t j = 0; j < keys.size() && (int)kept.size() < a.max_det; ++j) {
            const int slot = (int)(keys[j] & 0xffffffffull), e = slot / a.max_det;
            const unsigned* p = rows + (size_t)slot * TILE_ROW_WORDS;
            const float ox = (float)a.origins[2 * (e0 + e)], oy = (float)a.origins[2 * (e0 + e) + 1];
            TileBox me;
            me.x1 = __builtin_bit_cast(float, p[0]) + ox; me.y1 = __builtin_bit_cast(float, p[1]) + oy;
            me.x2 = __builtin_bit_cast(float, p[2]) + ox; me.y2 = __builtin_bit_cast(float, p[3]) + oy;
            me.area = (me.x2 - me.x1) * (me.y2 - me.y1);
            const int cls = (int)p[5];
            bool alive = true;
            for (size_t k = 0; k < kept.size() && alive; ++k)
                if (kcl[k] == cls && tile_overlap_gt(kept[k], me, a.metric, a.thr)) alive = false;
            if (alive) { kept.push_back(me); kcl.push_back(cls); ksl.push_back(slot); }
        }
        a.out_counts[f] = (int)kept.size();
        unsigned* out = a.out_rows + (size_t)f * a.max_det * TILE_ROW_WORDS;
        for (size_t k = 0; k < kept.size(); ++k) {
            const int slot = ksl[k], e = slot / a.max_det;
            const float ox = (float)a.origins[2 * (e0 + e)], oy = (float)a.origins[2 * (e0 + e) + 1];
            for (int q = 0; q < TILE_ROW_WORDS; ++q)
                out[k * TILE_ROW_WORDS + q] = tile_shift_word(rows[(size_t)slot * TILE_ROW_WORDS + q], q, ox, oy, a.nk, a.kdim);
            if (a.out_tile_idx) a.out_tile_idx[(size_t)f * a.max_det + k] = e;
        }
    }
}

static int pow2_at_least(long v) { long p = 1; while (p < v) p <<= 1; return (int)p; }

// ---- the merge of a call, enqueued behind the last chunk's NMS (infer_impl).  The per-frame entry ranges and the origins ride in one
// small device image, uploaded only when its bytes change (the same cameras call after call); the merged rows of a small call are
// written straight into the pinned host blocks, as the NMS kernel's are for an untiled one.
int tile_merge_enqueue(mi355_yolo* h, const InferCall& c, Prof& pf, bool direct_rows_on) {
    const TileCall& t = *c.tile;
    const int n = t.n_frames, NE = c.n, md = c.max_det;
    const size_t ints = (size_t)(n + 1) + 2 * (size_t)NE, bytes = ints * sizeof(int);
    const int grown = grow_or_fail(h->d_tile, bytes, "d_tile"); if (grown < 0) return MI355_EHIP;
    GROW(h->h_tile, bytes);
    if (grown) h->tile_bytes = 0;
    std::vector<int> img(ints);
    std::memcpy(img.data(), t.entry_off.data(), (size_t)(n + 1) * sizeof(int));
    std::memcpy(img.data() + n + 1, t.origins.data(), 2 * (size_t)NE * sizeof(int));
    if (h->tile_bytes != bytes || std::memcmp(h->h_tile.p, img.data(), bytes) != 0) {
        std::memcpy(h->h_tile.p, img.data(), bytes);      // the previous upload out of h_tile has completed: blocking calls synchronise
        HIPCHK(hipMemcpyAsync(h->d_tile.p, h->h_tile.p, bytes, hipMemcpyHostToDevice, h->stream));
        h->tile_bytes = bytes;
    }
    const size_t out_ints = (size_t)n + 2 * (size_t)n * md;           // counts | tile_idx slots | tile_idx packed
    GROW(h->d_tile_out, out_ints * sizeof(int)); GROW(h->h_tile_out, out_ints * sizeof(int));
    TileMergeArgs a{};
    a.rows = (const unsigned*)h->rows_dev(); a.counts = h->counts_dev();
    a.entry_off = (const int*)h->d_tile.p; a.origins = (const int*)h->d_tile.p + n + 1;
    a.n_frames = n; a.entries = t.max_entries; a.max_det = md;
    a.nk = (int)(h->hdr.nkpt * h->hdr.kdim); a.kdim = (int)h->hdr.kdim;
    a.metric = t.metric; a.thr = t.thr;
    if ((long)t.max_entries * md > 4096) {
        a.key_stride = pow2_at_least((long)t.max_entries * md);
        GROW(h->d_tile_keys, (size_t)n * a.key_stride * sizeof(unsigned long long));
        a.keys = (unsigned long long*)h->d_tile_keys.p;
    }
    h->tile_direct = n <= 16 && direct_rows_on;
    if (h->tile_direct) {
        void *rows_dev = nullptr, *out_dev = nullptr;
        HIPCHK(hipHostGetDevicePointer(&rows_dev, h->h_rows.p, 0));
        HIPCHK(hipHostGetDevicePointer(&out_dev, h->h_tile_out.p, 0));
        a.out_rows = (unsigned*)rows_dev; a.out_counts = (int*)out_dev; a.out_tile_idx = (int*)out_dev + n;
    } else {
        a.out_rows = (unsigned*)h->d_packed.p; a.out_counts = (int*)h->d_tile_out.p; a.out_tile_idx = (int*)h->d_tile_out.p + n;
    }
    TIMED(pf, K_NMS, launch_tile_merge(a, h->stream));
    return MI355_OK;
}

// ... and its rows on their way to the caller: counts clipped to the caller's capacity
int tile_merge_fetch(mi355_yolo* h, const InferCall& c) {
    const TileCall& t = *c.tile;
    const int n = t.n_frames, md = c.max_det;
    int* ho = (int*)h->h_tile_out.p;
    const int* idx = ho + n;                              // direct: slot layout [n][max_det]; otherwise packed in frame order
    if (h->tile_direct) {
        HIPCHK(hipStreamSynchronize(h->stream));
    } else {
        // compact on the GPU (the entry rows in d_rows are spent: the packed merged rows go there), then counts, then sum(counts) rows
        int* dc = (int*)h->d_tile_out.p;
        KCHK(launch_compact_rows(h->d_packed.p, dc, n, md, TILE_ROW_WORDS, (int*)h->d_offsets.p, h->d_rows.p, h->stream));
        KCHK(launch_compact_rows(dc + n, dc, n, md, 1, (int*)h->d_offsets.p, dc + n + (size_t)n * md, h->stream));
        HIPCHK(hipMemcpyAsync(ho, dc, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        size_t total = 0;
        for (int i = 0; i < n; ++i) total += (size_t)ho[i];
        if (total) {
            HIPCHK(hipMemcpyAsync(h->h_rows.p, h->d_rows.p, total * sizeof(mi355_det), hipMemcpyDeviceToHost, h->stream));
            HIPCHK(hipMemcpyAsync(ho + n, dc + n + (size_t)n * md, total * sizeof(int), hipMemcpyDeviceToHost, h->stream));
            HIPCHK(hipStreamSynchronize(h->stream));
        }
    }
    size_t at = 0;
    for (int i = 0; i < n; ++i) {
        const int cnt = std::min(ho[i], t.cap);
        const size_t from = h->tile_direct ? (size_t)i * md : at;
        t.out_counts[i] = cnt;
        std::memcpy(t.out_rows + (size_t)i * t.cap, h->rows_host() + from, (size_t)cnt * sizeof(mi355_det));
        if (t.out_tile_idx) std::memcpy(t.out_tile_idx + (size_t)i * t.cap, idx + from, (size_t)cnt * sizeof(int));
        at += (size_t)ho[i];
    }
    return MI355_OK;
}

static int tile_opts_check(const mi355_tile_opts* o) {
    if (!o) return fail(MI355_EINVAL, "tile: null options");
    if (o->struct_size < (int)sizeof(mi355_tile_opts)) return fail(MI355_EINVAL, "tile: struct_size is smaller than mi355_tile_opts");
    if (o->tile_h < 32 || o->tile_w < 32) return fail(MI355_EINVAL, "tile: tile_h and tile_w must be >= 32");
    if (o->overlap_y_px < 0 || o->overlap_y_px >= o->tile_h || o->overlap_x_px < 0 || o->overlap_x_px >= o->tile_w)
        return fail(MI355_EINVAL, "tile: overlap must be in [0, tile) pixels");
    if (o->metric != MI355_TILE_IOS && o->metric != MI355_TILE_IOU) return fail(MI355_EINVAL, "tile: metric is neither MI355_TILE_IOS nor MI355_TILE_IOU");
    if (!(o->thr >= 0.f && o->thr <= 1.f)) return fail(MI355_EINVAL, "tile: thr must be in [0, 1]");
    return MI355_OK;
}

struct TileOut { mi355_det* rows; int cap; int* counts; int* tile_idx; };

// n dense-or-pitched BGR frames on the engine's device -> entry list -> infer_impl with the merge behind it
static int tiled_run(mi355_yolo* h, const uint8_t* const* dev, const int* heights, const int* widths, const int* strides, int n,
                     const mi355_tile_opts& o, float conf, float iou, const int* classes, int n_classes, int max_det, int imgsz, const TileOut& out) {
    const int md = max_det <= 0 ? 300 : max_det;
    if (md > 1024) return fail(MI355_EINVAL, "max_det must be <= 1024");
    TileCall t;
    t.n_frames = n; t.metric = o.metric; t.thr = o.thr;
    t.out_rows = out.rows; t.cap = out.cap; t.out_counts = out.counts; t.out_tile_idx = out.tile_idx;
    std::vector<const uint8_t*> eptr; std::vector<int> eh, ew, es, xywh;
    t.entry_off.push_back(0);
    for (int i = 0; i < n; ++i) {
        const int rs = strides[i];
        tile_grid(heights[i], widths[i], o.tile_h, o.tile_w, o.overlap_y_px, o.overlap_x_px, xywh);
        if (o.full_frame) { xywh.push_back(0); xywh.push_back(0); xywh.push_back(widths[i]); xywh.push_back(heights[i]); }
        const int E = (int)xywh.size() / 4;
        if (E > MI355_TILE_MAX_ENTRIES)
            return fail(MI355_EINVAL, "tile: frame " + std::to_string(i) + " has " + std::to_string(E) + " entries, more than MI355_TILE_MAX_ENTRIES");
        if ((long)E * md > MI355_TILE_MAX_CANDIDATES)
            return fail(MI355_EINVAL, "tile: entries x max_det of frame " + std::to_string(i) + " exceeds MI355_TILE_MAX_CANDIDATES");
        for (int e = 0; e < E; ++e) {
            const int x = xywh[4 * e], y = xywh[4 * e + 1];
            eptr.push_back(dev[i] + (size_t)y * rs + (size_t)x * 3);
            ew.push_back(xywh[4 * e + 2]); eh.push_back(xywh[4 * e + 3]); es.push_back(rs);
            t.origins.push_back(x); t.origins.push_back(y);
        }
        t.max_entries = std::max(t.max_entries, E);
        t.entry_off.push_back((int)eptr.size());
    }
    const MultiFrames mf{eptr.data(), eh.data(), ew.data(), es.data(), true};
    InferCall c;
    c.multi = &mf; c.n = (int)eptr.size(); c.tile = &t;
    c.conf = conf; c.iou = iou; c.classes = classes; c.n_classes = n_classes; c.max_det = md; c.imgsz = imgsz;
    c.out_rows = out.rows; c.cap = out.cap; c.out_counts = out.counts;
    const int rc = infer_impl(h, c); if (rc) return rc;
    h->last_frames.resize((size_t)n);                         // the one device copy of every source frame (d_tile_frames, or the caller's)
    for (int i = 0; i < n; ++i) h->last_frames[i] = mi355_yolo::LastFrame{dev[i], heights[i], widths[i], strides[i]};
    return MI355_OK;
}

// what both entry points check and do first
static int tiled_begin(mi355_yolo* h, const mi355_tile_opts* tile, const TileOut& out) {
    if (!h || !out.rows || !out.counts) return fail(MI355_EINVAL, "null argument");
    if (out.cap < 1) return fail(MI355_EINVAL, "out_capacity_per_image must be >= 1");
    const int rc = tile_opts_check(tile); if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    if (h->async_pending) { HIPCHK(hipStreamSynchronize(h->stream)); h->async_pending = false; }   // it may still read the buffers grown below
    return MI355_OK;
}

}  // namespace mi355

using namespace mi355;

extern "C" {

int mi355_tile_grid(int height, int width, int tile_h, int tile_w, int overlap_y_px, int overlap_x_px, int* out_xywh, int cap, int* count) {
    if (!count) return fail(MI355_EINVAL, "tile grid: count is null");
    const int rc = grid_check(height, width, tile_h, tile_w, overlap_y_px, overlap_x_px); if (rc) return rc;
    std::vector<int> xywh;
    tile_grid(height, width, tile_h, tile_w, overlap_y_px, overlap_x_px, xywh);
    *count = (int)xywh.size() / 4;
    if (!out_xywh) return MI355_OK;
    if (*count > cap) return fail(MI355_EINVAL, "tile grid: " + std::to_string(*count) + " tiles, more than cap");
    std::memcpy(out_xywh, xywh.data(), xywh.size() * sizeof(int));
    return MI355_OK;
}

int mi355_yolo_infer_tiled(mi355_yolo* h, const uint8_t* const* frames, const int* heights, const int* widths, const int* row_strides,
                           int frames_on_device, int n, const mi355_tile_opts* tile, float conf, float iou, const int* classes, int n_classes,
                           int max_det, int imgsz, mi355_det* out_rows, int cap, int* out_counts, int* out_tile_idx) {
    const TileOut out{out_rows, cap, out_counts, out_tile_idx};
    int rc = tiled_begin(h, tile, out); if (rc) return rc;
    const MultiFrames mf{frames, heights, widths, row_strides, frames_on_device != 0};
    rc = multi_check(mf, n); if (rc) return rc;
    std::vector<const uint8_t*> dev(n); std::vector<int> strides(n);
    for (int i = 0; i < n; ++i) { const int rs = row_strides ? row_strides[i] : 0; strides[i] = rs ? rs : widths[i] * 3; dev[i] = frames[i]; }
    if (!frames_on_device) {
        // every host frame ONCE, ahead of the first chunk, rows packed: the entries of a frame are views of this copy
        std::vector<size_t> off(n);
        size_t at = 0;
        for (int i = 0; i < n; ++i) { off[i] = at; at += round_up_sz((size_t)heights[i] * widths[i] * 3, 256); }
        GROW(h->d_tile_frames, at);
        for (int i = 0; i < n; ++i) {
            const size_t row = (size_t)widths[i] * 3;
            if ((size_t)strides[i] == row) HIPCHK(hipMemcpyAsync(h->d_tile_frames.p + off[i], frames[i], row * heights[i], hipMemcpyHostToDevice, h->stream));
            else HIPCHK(hipMemcpy2DAsync(h->d_tile_frames.p + off[i], row, frames[i], (size_t)strides[i], row, (size_t)heights[i], hipMemcpyHostToDevice, h->stream));
            dev[i] = h->d_tile_frames.p + off[i]; strides[i] = (int)row;
        }
    }
    return tiled_run(h, dev.data(), heights, widths, strides.data(), n, *tile, conf, iou, classes, n_classes, max_det, imgsz, out);
}

int mi355_yolo_infer_tiled_yuv(mi355_yolo* h, const mi355_yuv_frame* frames, int frames_on_device, int n, const mi355_tile_opts* tile,
                               float conf, float iou, const int* classes, int n_classes, int max_det, int imgsz, mi355_det* out_rows, int cap,
                               int* out_counts, int* out_tile_idx) {
    const TileOut out{out_rows, cap, out_counts, out_tile_idx};
    int rc = tiled_begin(h, tile, out); if (rc) return rc;
    rc = yuv_check(frames, n); if (rc) return rc;
    // all n frames -> dense BGR in d_tile_frames by ONE conversion launch; host planes are uploaded first, rows packed
    std::vector<size_t> off(n), poff(n);
    size_t at = 0, pat = 0;
    for (int i = 0; i < n; ++i) {
        off[i] = at; at += round_up_sz((size_t)frames[i].height * frames[i].width * 3, 256);
        poff[i] = pat; pat += round_up_sz((size_t)frames[i].height * frames[i].width * 3 / 2, 256);
    }
    GROW(h->d_tile_frames, at);
    if (!frames_on_device) GROW(h->d_yuv, pat);
    const size_t dbytes = (size_t)n * sizeof(YuvFrameDesc);
    GROW(h->d_yuvdesc, dbytes); GROW(h->h_yuvdesc, dbytes);
    YuvFrameDesc* hd = (YuvFrameDesc*)h->h_yuvdesc.p;
    std::vector<const uint8_t*> dev(n); std::vector<int> heights(n), widths(n), strides(n);
    for (int i = 0; i < n; ++i) {
        mi355_yuv_frame f = frames[i];
        if (!frames_on_device) {
            const bool nv12 = f.format == MI355_PIX_NV12;
            const size_t crow = nv12 ? (size_t)f.width : (size_t)f.width / 2;
            uint8_t* y = h->d_yuv.p + poff[i]; uint8_t* u = y + (size_t)f.height * f.width; uint8_t* v = u + (size_t)(f.height / 2) * (f.width / 2);
            HIPCHK(hipMemcpy2DAsync(y, (size_t)f.width, f.y, (size_t)f.y_stride, (size_t)f.width, (size_t)f.height, hipMemcpyHostToDevice, h->stream));
            HIPCHK(hipMemcpy2DAsync(u, crow, f.u, (size_t)f.uv_stride, crow, (size_t)f.height / 2, hipMemcpyHostToDevice, h->stream));
            if (!nv12) HIPCHK(hipMemcpy2DAsync(v, crow, f.v, (size_t)f.uv_stride, crow, (size_t)f.height / 2, hipMemcpyHostToDevice, h->stream));
            f.y = y; f.u = u; f.v = nv12 ? nullptr : v; f.y_stride = f.width; f.uv_stride = (int)crow;
        }
        hd[i] = yuv_desc(f, h->d_tile_frames.p + off[i]);
        dev[i] = h->d_tile_frames.p + off[i]; heights[i] = f.height; widths[i] = f.width; strides[i] = f.width * 3;
    }
    HIPCHK(hipMemcpyAsync(h->d_yuvdesc.p, hd, dbytes, hipMemcpyHostToDevice, h->stream));
    KCHK(launch_yuv_to_bgr((const YuvFrameDesc*)h->d_yuvdesc.p, hd, n, h->stream));
    return tiled_run(h, dev.data(), heights.data(), widths.data(), strides.data(), n, *tile, conf, iou, classes, n_classes, max_det, imgsz, out);
}

int mi355_op_tile_merge(int device, const mi355_det* rows, const int* counts, const int* origins, int n_frames, int entries, int max_det,
                        int kdim, int metric, float thr, mi355_det* out_rows, int* out_counts, int* out_tile_idx) {
    if (!rows || !counts || !origins || !out_rows || !out_counts) return fail(MI355_EINVAL, "tile_merge: null argument");
    if (n_frames < 1) return fail(MI355_EINVAL, "tile_merge: n_frames must be positive");
    if (entries < 1 || entries > MI355_TILE_MAX_ENTRIES) return fail(MI355_EINVAL, "tile_merge: entries must be in [1, MI355_TILE_MAX_ENTRIES]");
    if (max_det < 1 || max_det > 1024) return fail(MI355_EINVAL, "tile_merge: max_det must be in [1, 1024]");
    if ((long)entries * max_det > MI355_TILE_MAX_CANDIDATES) return fail(MI355_EINVAL, "tile_merge: entries x max_det exceeds MI355_TILE_MAX_CANDIDATES");
    if (!(kdim == 0 || kdim == 2 || kdim == 3)) return fail(MI355_EINVAL, "tile_merge: kdim must be 0, 2 or 3");
    if (metric != MI355_TILE_IOS && metric != MI355_TILE_IOU) return fail(MI355_EINVAL, "tile_merge: metric is neither MI355_TILE_IOS nor MI355_TILE_IOU");
    if (!(thr >= 0.f && thr <= 1.f)) return fail(MI355_EINVAL, "tile_merge: thr must be in [0, 1]");
    const size_t NE = (size_t)n_frames * entries;
    for (size_t i = 0; i < NE; ++i)
        if (counts[i] < 0 || counts[i] > max_det) return fail(MI355_EINVAL, "tile_merge: counts[" + std::to_string(i) + "] outside [0, max_det]");
    TileMergeArgs a{};
    a.n_frames = n_frames; a.entries = entries; a.max_det = max_det; a.kdim = kdim;
    a.nk = kdim ? (MI355_MAX_KPT_FLOATS / kdim) * kdim : 0;
    a.metric = metric; a.thr = thr;
    if (device < 0) {
        a.rows = (const unsigned*)rows; a.counts = counts; a.origins = origins;
        a.out_rows = (unsigned*)out_rows; a.out_counts = out_counts; a.out_tile_idx = out_tile_idx;
        tile_merge_host(a);
        return MI355_OK;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(MI355_EHIP, "no HIP device: the merge kernel needs an MI355X (device = -1 runs its host twin)");
    if (device >= ndev) return fail(MI355_EINVAL, "tile_merge: device out of range");
    HIPCHK(hipSetDevice(device));
    const size_t in_rows = NE * max_det * sizeof(mi355_det), out_rows_b = (size_t)n_frames * max_det * sizeof(mi355_det);
    const size_t idx_b = (size_t)n_frames * max_det * sizeof(int);
    DevMem dm; unsigned *d_rows, *d_out; int *d_counts, *d_origins, *d_oc, *d_idx; unsigned long long* d_keys = nullptr;
    HIPCHK(dm.alloc(&d_rows, in_rows)); HIPCHK(dm.alloc(&d_counts, NE * sizeof(int))); HIPCHK(dm.alloc(&d_origins, NE * 2 * sizeof(int)));
    HIPCHK(dm.alloc(&d_out, out_rows_b)); HIPCHK(dm.alloc(&d_oc, (size_t)n_frames * sizeof(int))); HIPCHK(dm.alloc(&d_idx, idx_b));
    if ((long)entries * max_det > 4096) {
        a.key_stride = pow2_at_least((long)entries * max_det);
        HIPCHK(dm.alloc(&d_keys, (size_t)n_frames * a.key_stride * sizeof(unsigned long long)));
    }
    HIPCHK(hipMemcpy(d_rows, rows, in_rows, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_counts, counts, NE * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_origins, origins, NE * 2 * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_out, out_rows, out_rows_b, hipMemcpyHostToDevice));                 // what the launch does not write keeps the caller's bits
    if (out_tile_idx) HIPCHK(hipMemcpy(d_idx, out_tile_idx, idx_b, hipMemcpyHostToDevice));
    a.rows = d_rows; a.counts = d_counts; a.origins = d_origins; a.keys = d_keys;
    a.out_rows = d_out; a.out_counts = d_oc; a.out_tile_idx = d_idx;
    KCHK(launch_tile_merge(a, nullptr));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out_rows, d_out, out_rows_b, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_counts, d_oc, (size_t)n_frames * sizeof(int), hipMemcpyDeviceToHost));
    if (out_tile_idx) HIPCHK(hipMemcpy(out_tile_idx, d_idx, idx_b, hipMemcpyDeviceToHost));
    return MI355_OK;
}

}  // extern "C"
