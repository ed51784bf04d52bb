// Evidence frames: a tile-binned rasteriser.  Source frame in, rendered frame out, never in place.  Two launches per
// call, whatever the number of frames (descriptor-driven, blockIdx.y = frame):
//   bin    one lane per primitive: for every 32 x 32 tile its bounding box meets (render_touches), atomicOr of its bit into the tile's
//          mask and of the tile's flags.  A mask is a set, so the order in which lanes arrive cannot show.
//   draw   one block of 256 lanes per tile.  A tile without primitives is copied.  Otherwise the tile is staged in LDS, the block means
//          of the SOURCE are formed when a mosaic touches it, and every lane carries four pixels of a row through the tile's primitives
//          in ascending index (mosaics first, then the rest), 256 mask words at a time, their records fetched into LDS 256 at once.  The tile goes back through LDS and out
//          with 16-byte stores where the frame's alignment allows them, by bytes otherwise.
// The rules themselves are render_raster.h's, shared with the host twin (device = -1).
#include "engine_internal.h"
#include "render_raster.h"

namespace mi355 {
namespace {

__global__ __launch_bounds__(256) void render_bin_kernel(const RenderFrame* __restrict__ frames) {
    const RenderFrame f = frames[blockIdx.y];
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= f.P) return;
    int p[kRenderWords];
    const int4* q = reinterpret_cast<const int4*>(f.prims + (size_t)i * kRenderWords);
    const int4 a = q[0], b = q[1];
    p[0] = a.x; p[1] = a.y; p[2] = a.z; p[3] = a.w; p[4] = b.x; p[5] = b.y; p[6] = b.z; p[7] = b.w;
    int x0, y0, x1, y1;
    render_bbox(p, x0, y0, x1, y1);
    x0 = render_max(x0, 0); y0 = render_max(y0, 0); x1 = render_min(x1, f.W - 1); y1 = render_min(y1, f.H - 1);
    if (x1 < x0 || y1 < y0) return;
    const unsigned bit = 1u << (i & 31), fl = p[0] == RENDER_MOSAIC ? 3u : 1u;
    for (int ty = y0 / kRenderTile; ty <= y1 / kRenderTile; ++ty)
        for (int tx = x0 / kRenderTile; tx <= x1 / kRenderTile; ++tx) {
            const int px0 = tx * kRenderTile, py0 = ty * kRenderTile;
            if (!render_touches(p, px0, py0, render_min(px0 + kRenderTile, f.W) - 1, render_min(py0 + kRenderTile, f.H) - 1)) continue;
            const int tile = ty * f.tiles_x + tx;
            atomicOr(f.bins + (size_t)tile * f.words + (i >> 5), bit);
            atomicOr(f.flags + tile, fl);
        }
}

__global__ __launch_bounds__(256) void render_draw_kernel(const RenderFrame* __restrict__ frames) {
    const RenderFrame f = frames[blockIdx.y];
    const int tile = (int)blockIdx.x;
    if (tile >= f.tiles_x * f.tiles_y) return;                         // block-uniform
    const int t = (int)threadIdx.x;
    const int ty = tile / f.tiles_x, tx = tile - ty * f.tiles_x;
    const int x0 = tx * kRenderTile, y0 = ty * kRenderTile;
    const int tw = render_min(kRenderTile, f.W - x0), th = render_min(kRenderTile, f.H - y0);
    const bool vec = f.vec && tw == kRenderTile;                       // a full-width tile's rows start at a multiple of 96 bytes
    const unsigned fl = f.flags[tile];
    const uint8_t* src = f.src + (size_t)y0 * f.src_pitch + (size_t)x0 * 3;
    uint8_t* dst = f.dst + (size_t)y0 * f.dst_pitch + (size_t)x0 * 3;

    __shared__ __attribute__((aligned(16))) uint8_t s_tile[kRenderTile * kRenderTileRow];
    __shared__ unsigned s_words[256];
    __shared__ unsigned long long s_nz[4];
    __shared__ unsigned short s_list[256];
    __shared__ __attribute__((aligned(16))) int s_prims[256 * kRenderWords];
    __shared__ unsigned s_sum[kRenderMeans * 3];
    __shared__ unsigned s_mean[kRenderMeans];

    // ---- stage the tile (or copy it straight through when nothing touches it)
    if (vec) {
        if (t < 6 * kRenderTile) {
            const int row = t / 6, c = t - row * 6;
            if (row < th) {
                const uint4 v = *reinterpret_cast<const uint4*>(src + (size_t)row * f.src_pitch + c * 16);
                if (!fl) *reinterpret_cast<uint4*>(dst + (size_t)row * f.dst_pitch + c * 16) = v;
                else *reinterpret_cast<uint4*>(s_tile + row * kRenderTileRow + c * 16) = v;
            }
        }
    } else {
        const int rb = tw * 3;
        for (int i = t; i < th * rb; i += 256) {
            const int row = i / rb, b = i - row * rb;
            const uint8_t v = src[(size_t)row * f.src_pitch + b];
            if (!fl) dst[(size_t)row * f.dst_pitch + b] = v;
            else s_tile[row * kRenderTileRow + b] = v;
        }
    }
    if (!fl) return;                                                   // block-uniform
    __syncthreads();

    // ---- block means of the source, when a mosaic touches the tile: 4 x 4 sums from the pixels, each larger block from its four children
    if (fl & 2u) {
        if (t < 64 * 3) {
            const int blk = t / 3, ch = t - blk * 3, bx = (blk & 7) * 4, by = (blk >> 3) * 4;
            unsigned s = 0;
            for (int y = by; y < render_min(by + 4, th); ++y)
                for (int x = bx; x < render_min(bx + 4, tw); ++x) s += s_tile[y * kRenderTileRow + x * 3 + ch];
            s_sum[t] = s;
        }
        __syncthreads();
        if (t < 16 * 3) {
            const int blk = t / 3, ch = t - blk * 3, cx = (blk & 3) * 2, cy = (blk >> 2) * 2;
            s_sum[(64 + blk) * 3 + ch] = s_sum[(cy * 8 + cx) * 3 + ch] + s_sum[(cy * 8 + cx + 1) * 3 + ch] + s_sum[((cy + 1) * 8 + cx) * 3 + ch] +
                                         s_sum[((cy + 1) * 8 + cx + 1) * 3 + ch];
        }
        __syncthreads();
        if (t < 4 * 3) {
            const int blk = t / 3, ch = t - blk * 3, cx = (blk & 1) * 2, cy = (blk >> 1) * 2;
            s_sum[(80 + blk) * 3 + ch] = s_sum[(64 + cy * 4 + cx) * 3 + ch] + s_sum[(64 + cy * 4 + cx + 1) * 3 + ch] +
                                         s_sum[(64 + (cy + 1) * 4 + cx) * 3 + ch] + s_sum[(64 + (cy + 1) * 4 + cx + 1) * 3 + ch];
        }
        __syncthreads();
        if (t < 3) s_sum[84 * 3 + t] = s_sum[80 * 3 + t] + s_sum[81 * 3 + t] + s_sum[82 * 3 + t] + s_sum[83 * 3 + t];
        __syncthreads();
        if (t < kRenderMeans) {
            int B, bx, by;
            const int n = render_mean_block(t, tw, th, B, bx, by);
            unsigned m = 0;
            if (n) m = render_mean(s_sum[t * 3], (unsigned)n) | render_mean(s_sum[t * 3 + 1], (unsigned)n) << 8 | render_mean(s_sum[t * 3 + 2], (unsigned)n) << 16;
            s_mean[t] = m;
        }
        __syncthreads();
    }

    // ---- this lane's four pixels
    const int ly = t >> 3, lx = (t & 7) * 4;
    const bool live = ly < th && lx < tw;
    unsigned px[4] = {0, 0, 0, 0};
    if (live) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (lx + k < tw) {
                const uint8_t* s = s_tile + ly * kRenderTileRow + (lx + k) * 3;
                px[k] = (unsigned)s[0] | (unsigned)s[1] << 8 | (unsigned)s[2] << 16;
            }
        }
    }
    const unsigned* bins = f.bins + (size_t)tile * f.words;
    for (int pass = (fl & 2u) ? 0 : 1; pass < 2; ++pass) {
        for (int w0 = 0; w0 < f.words; w0 += 256) {
            __syncthreads();                                           // the previous round's words have been walked
            const unsigned wv = w0 + t < f.words ? bins[w0 + t] : 0u;
            s_words[t] = wv;
            const unsigned long long nz = __ballot(wv != 0u);
            if ((t & 63) == 0) s_nz[t >> 6] = nz;
            __syncthreads();
            // the round's non-zero words in ascending order, then their primitives eight words at a time: lane (k, bit) fetches the
            // record of bit `bit` of the k-th word into LDS -- one global round trip per 256 candidate records instead of one per record
            const int wave = t >> 6;
            int before = 0, nnz = 0;
            for (int g = 0; g < 4; ++g) { const int c = __popcll(s_nz[g]); before += g < wave ? c : 0; nnz += c; }
            if (wv != 0u) s_list[before + __popcll(nz & ((1ull << (t & 63)) - 1ull))] = (unsigned short)t;
            __syncthreads();
            for (int b0 = 0; b0 < nnz; b0 += 8) {
                const int k = t >> 5, bit = t & 31;
                if (b0 + k < nnz) {
                    const int j = s_list[b0 + k];
                    if ((s_words[j] >> bit) & 1u) {
                        const int4* q = reinterpret_cast<const int4*>(f.prims + (size_t)((w0 + j) * 32 + bit) * kRenderWords);
                        int4* d = reinterpret_cast<int4*>(s_prims + t * kRenderWords);
                        d[0] = q[0]; d[1] = q[1];
                    }
                }
                __syncthreads();
                const int nk = render_min(8, nnz - b0);
                for (int k2 = 0; k2 < nk; ++k2) {
                    for (unsigned bits = __builtin_amdgcn_readfirstlane(s_words[s_list[b0 + k2]]); bits; bits &= bits - 1) {   // the same for every lane
                        const int4* q = reinterpret_cast<const int4*>(s_prims + (k2 * 32 + __ffs((int)bits) - 1) * kRenderWords);
                        const int4 a = q[0], b = q[1];
                        const int p[kRenderWords] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
                        if (live) render_apply(p, pass, x0 + lx, y0 + ly, x0, y0, s_mean, px);
                    }
                }
                __syncthreads();                                       // before the next eight words' records replace these
            }
        }
    }
    __syncthreads();                                                   // every lane has read its source pixels: the tile becomes the output
    if (live) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (lx + k < tw) {
                uint8_t* s = s_tile + ly * kRenderTileRow + (lx + k) * 3;
                s[0] = (uint8_t)px[k]; s[1] = (uint8_t)(px[k] >> 8); s[2] = (uint8_t)(px[k] >> 16);
            }
        }
    }
    __syncthreads();
    if (vec) {
        if (t < 6 * kRenderTile) {
            const int row = t / 6, c = t - row * 6;
            if (row < th) *reinterpret_cast<uint4*>(dst + (size_t)row * f.dst_pitch + c * 16) = *reinterpret_cast<const uint4*>(s_tile + row * kRenderTileRow + c * 16);
        }
    } else {
        const int rb = tw * 3;
        for (int i = t; i < th * rb; i += 256) {
            const int row = i / rb, b = i - row * rb;
            dst[(size_t)row * f.dst_pitch + b] = s_tile[row * kRenderTileRow + b];
        }
    }
}

constexpr size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

const char* launch_render(const RenderFrame* frames_dev, const RenderFrame* frames_host, int n, hipStream_t st) {
    int most_p = 0, most_t = 1;
    for (int i = 0; i < n; ++i) {
        most_p = std::max(most_p, frames_host[i].P);
        most_t = std::max(most_t, frames_host[i].tiles_x * frames_host[i].tiles_y);
    }
    if (most_p) {
        hipLaunchKernelGGL(render_bin_kernel, dim3((unsigned)((most_p + 255) / 256), (unsigned)n), dim3(256), 0, st, frames_dev);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hipGetErrorString(e);
    }
    hipLaunchKernelGGL(render_draw_kernel, dim3((unsigned)most_t, (unsigned)n), dim3(256), 0, st, frames_dev);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? hipGetErrorString(e) : nullptr;
}

// ---- one call: checks, the work buffer's layout, staging of host frames, the launches, the copy back -----------------------------------
int render_check(const mi355_render_frame* frames, int n, const int32_t* const* prims, const int* n_prims, const mi355_render_out* outs, bool host_only) {
    if (!frames || !n_prims || !prims || !outs) return fail(MI355_EINVAL, "render: null argument");
    if (n < 1 || n > MI355_RENDER_MAX_FRAMES) return fail(MI355_EINVAL, "render: n must be in [1, " + std::to_string(MI355_RENDER_MAX_FRAMES) + "]");
    for (int i = 0; i < n; ++i) {
        const mi355_render_frame& f = frames[i];
        const std::string at = "render: frames[" + std::to_string(i) + "]: ";
        if (!f.data || !outs[i].data) return fail(MI355_EINVAL, at + "a frame or output pointer is null");
        if (f.height < 1 || f.width < 1 || f.height > kRenderMaxSide || f.width > kRenderMaxSide)
            return fail(MI355_EINVAL, at + "height and width must be in [1, " + std::to_string(kRenderMaxSide) + "]");
        if ((long long)f.row_stride < 3ll * f.width || (long long)outs[i].row_stride < 3ll * f.width) return fail(MI355_EINVAL, at + "a row_stride is smaller than a row");
        if ((long long)f.height * f.row_stride >= (1ll << 31) || (long long)f.height * outs[i].row_stride >= (1ll << 31))
            return fail(MI355_EINVAL, at + "a frame must be smaller than 2 GiB");
        if (host_only && (f.on_device || outs[i].on_device)) return fail(MI355_EINVAL, at + "the host twin (device -1) takes host memory");
        if (f.data == outs[i].data) return fail(MI355_EINVAL, at + "rendering is out of place: the output must not be the source");
        if (n_prims[i] < 0) return fail(MI355_EINVAL, at + "negative primitive count");
        if (n_prims[i] > MI355_RENDER_MAX_PRIMS)
            return fail(MI355_EINVAL, at + std::to_string(n_prims[i]) + " primitives: at most MI355_RENDER_MAX_PRIMS = " + std::to_string(MI355_RENDER_MAX_PRIMS) +
                                          " per frame are binned; nothing was drawn");
        if (n_prims[i] && !prims[i]) return fail(MI355_EINVAL, at + "the primitive array is null");
        for (int k = 0; k < n_prims[i]; ++k) {
            const char* why = render_check_prim(prims[i] + (size_t)k * kRenderWords);
            if (why) return fail(MI355_EINVAL, at + "primitive " + std::to_string(k) + ": " + why);
        }
    }
    return MI355_OK;
}

RenderFrame render_desc(const mi355_render_frame& f, const mi355_render_out& o, int P) {
    RenderFrame d{};
    d.src = f.data; d.dst = o.data; d.H = f.height; d.W = f.width; d.src_pitch = f.row_stride; d.dst_pitch = o.row_stride;
    d.P = P; d.words = (P + 31) / 32; d.tiles_x = (f.width + kRenderTile - 1) / kRenderTile; d.tiles_y = (f.height + kRenderTile - 1) / kRenderTile;
    return d;
}

int render_run(RenderCtx& ctx, int device, const mi355_render_frame* frames, int n, const int32_t* const* prims, const int* n_prims,
               const mi355_render_out* outs, hipStream_t st, float* launch_ms) {
    int rc = render_check(frames, n, prims, n_prims, outs, device < 0); if (rc) return rc;
    if (launch_ms) *launch_ms = 0.f;
    std::vector<RenderFrame> desc((size_t)n);
    for (int i = 0; i < n; ++i) desc[i] = render_desc(frames[i], outs[i], n_prims[i]);
    if (device < 0) {
        for (int i = 0; i < n; ++i) { desc[i].prims = prims[i]; render_frame_host(desc[i]); }
        return MI355_OK;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return fail(MI355_EHIP, "no HIP device: the render kernel needs an MI355X (device = -1 runs its host twin)"); }
    if (device >= ndev) return fail(MI355_EINVAL, "render: device out of range");
    HIPCHK(hipSetDevice(device));
    // the work buffer: [descriptors | primitives | bins and flags (zeroed per call) | staged host sources | staged host outputs]; a host
    // frame is staged with the caller's pitch and its address modulo 16, so it takes the path it would take in place
    const size_t desc_bytes = al256((size_t)n * sizeof(RenderFrame));
    size_t at = desc_bytes;
    std::vector<size_t> prim_off((size_t)n), bin_off((size_t)n), flag_off((size_t)n), src_off((size_t)n, 0), dst_off((size_t)n, 0);
    for (int i = 0; i < n; ++i) { prim_off[i] = at; at = al256(at + (size_t)n_prims[i] * kRenderWords * 4); }
    const size_t img_bytes = at, zero_at = at;
    for (int i = 0; i < n; ++i) {
        const size_t tiles = (size_t)desc[i].tiles_x * desc[i].tiles_y;
        bin_off[i] = at; at += tiles * desc[i].words * 4; flag_off[i] = at; at = al256(at + tiles * 4);
    }
    const size_t zero_bytes = at - zero_at;
    auto span = [](int h, int pitch, int w) { return (size_t)(h - 1) * pitch + (size_t)w * 3; };
    for (int i = 0; i < n; ++i) {
        if (!frames[i].on_device) { src_off[i] = at + ((uintptr_t)frames[i].data & 15u); at = al256(src_off[i] + span(desc[i].H, desc[i].src_pitch, desc[i].W)); }
        if (!outs[i].on_device) { dst_off[i] = at + ((uintptr_t)outs[i].data & 15u); at = al256(dst_off[i] + span(desc[i].H, desc[i].dst_pitch, desc[i].W)); }
    }
    if (buf_grow(ctx.d_work, at, at + at / 4) < 0 || buf_grow(ctx.h_img, img_bytes, img_bytes + img_bytes / 4) < 0)
        return fail(MI355_EHIP, "render: out of device or pinned memory");
    uint8_t* base = ctx.d_work.p;
    for (int i = 0; i < n; ++i) {
        RenderFrame& d = desc[i];
        d.prims = (const int*)(base + prim_off[i]); d.bins = (unsigned*)(base + bin_off[i]); d.flags = (unsigned*)(base + flag_off[i]);
        if (!frames[i].on_device) {
            d.src = base + src_off[i];
            HIPCHK(hipMemcpyAsync(base + src_off[i], frames[i].data, span(d.H, d.src_pitch, d.W), hipMemcpyHostToDevice, st));
        }
        if (!outs[i].on_device) d.dst = base + dst_off[i];
        auto a16 = [](const void* p) { return ((uintptr_t)p & 15u) == 0; };
        d.vec = a16(d.src) && a16(d.dst) && d.src_pitch % 16 == 0 && d.dst_pitch % 16 == 0 ? 1 : 0;
        if (n_prims[i]) std::memcpy(ctx.h_img.p + prim_off[i], prims[i], (size_t)n_prims[i] * kRenderWords * 4);
    }
    std::memcpy(ctx.h_img.p, desc.data(), (size_t)n * sizeof(RenderFrame));
    HIPCHK(hipMemcpyAsync(base, ctx.h_img.p, img_bytes, hipMemcpyHostToDevice, st));
    if (launch_ms && !ctx.ev0) { HIPCHK(hipEventCreate(&ctx.ev0)); HIPCHK(hipEventCreate(&ctx.ev1)); }
    if (launch_ms) HIPCHK(hipEventRecord(ctx.ev0, st));
    if (zero_bytes) HIPCHK(hipMemsetAsync(base + zero_at, 0, zero_bytes, st));
    KCHK(launch_render((const RenderFrame*)base, desc.data(), n, st));
    if (launch_ms) HIPCHK(hipEventRecord(ctx.ev1, st));
    // host outputs come back through pinned memory (a copy into pageable memory runs at a fraction of the link's rate), rows packed;
    // only the pixels travel on: the caller's row padding keeps its bytes
    std::vector<size_t> back((size_t)n, 0);
    size_t back_bytes = 0;
    for (int i = 0; i < n; ++i)
        if (!outs[i].on_device) { back[i] = back_bytes; back_bytes = al256(back_bytes + (size_t)desc[i].H * desc[i].W * 3); }
    if (back_bytes && buf_grow(ctx.h_out, back_bytes, back_bytes + back_bytes / 4) < 0) return fail(MI355_EHIP, "render: out of pinned memory");
    for (int i = 0; i < n; ++i) {
        if (outs[i].on_device) continue;
        HIPCHK(hipMemcpy2DAsync(ctx.h_out.p + back[i], (size_t)desc[i].W * 3, desc[i].dst, (size_t)desc[i].dst_pitch, (size_t)desc[i].W * 3, (size_t)desc[i].H,
                                hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    for (int i = 0; i < n; ++i) {
        if (outs[i].on_device) continue;
        const size_t row = (size_t)desc[i].W * 3;
        if ((size_t)outs[i].row_stride == row) std::memcpy(outs[i].data, ctx.h_out.p + back[i], row * desc[i].H);
        else for (int y = 0; y < desc[i].H; ++y) std::memcpy(outs[i].data + (size_t)y * outs[i].row_stride, ctx.h_out.p + back[i] + (size_t)y * row, row);
    }
    if (launch_ms) HIPCHK(hipEventElapsedTime(launch_ms, ctx.ev0, ctx.ev1));
    return MI355_OK;
}

void render_ctx_free(RenderCtx& ctx) {
    buf_free(ctx.d_work); buf_free(ctx.h_img); buf_free(ctx.h_out);
    if (ctx.ev0) { (void)hipEventDestroy(ctx.ev0); (void)hipEventDestroy(ctx.ev1); ctx.ev0 = ctx.ev1 = nullptr; }
}

}  // namespace mi355

using namespace mi355;

extern "C" int mi355_render(int device, const mi355_render_frame* frames, int n, const int32_t* const* prims, const int* n_prims,
                            const mi355_render_out* outs, void* stream, float* launch_ms) {
    RenderCtx ctx;
    const int rc = render_run(ctx, device, frames, n, prims, n_prims, outs, (hipStream_t)stream, launch_ms);
    if (device >= 0) render_ctx_free(ctx);
    return rc;
}

extern "C" int mi355_yolo_last_frames(mi355_yolo* h, mi355_render_frame* frames_out, int cap, int* n) {
    if (!h || !n) return fail(MI355_EINVAL, "last frames: null argument");
    *n = (int)h->last_frames.size();
    if (!frames_out) return MI355_OK;
    if (cap < *n) return fail(MI355_EINVAL, "last frames: cap is smaller than the last call's number of frames");
    for (int i = 0; i < *n; ++i) {
        const mi355_yolo::LastFrame& f = h->last_frames[i];
        frames_out[i] = mi355_render_frame{f.p, f.h, f.w, f.pitch, 1};
    }
    return MI355_OK;
}

extern "C" int mi355_yolo_render(mi355_yolo* h, const mi355_render_frame* frames, int n, const int32_t* const* prims, const int* n_prims,
                                 const mi355_render_out* outs, float* launch_ms) {
    if (!h) return fail(MI355_EINVAL, "render: null handle");
    std::vector<mi355_render_frame> last;
    if (!frames) {                                             // the frames of the handle's last call, where that call left them on the device
        if (h->last_frames.empty()) return fail(MI355_EINVAL, "render: the handle has no frames of a last blocking infer call");
        if (n != (int)h->last_frames.size())
            return fail(MI355_EINVAL, "render: n = " + std::to_string(n) + ", but the last call had " + std::to_string(h->last_frames.size()) + " frames");
        last.resize((size_t)n);
        for (int i = 0; i < n; ++i) {
            const mi355_yolo::LastFrame& f = h->last_frames[i];
            if (!f.p) return fail(MI355_EINVAL, "render: frame " + std::to_string(i) + " of the last call is no longer on the device (a host call of more than two "
                                                "chunks keeps its last two): pass the frames again");
            last[i] = mi355_render_frame{f.p, f.h, f.w, f.pitch, 1};
        }
        frames = last.data();
    }
    HIPCHK(hipSetDevice(h->device));
    if (h->async_pending) { HIPCHK(hipStreamSynchronize(h->stream)); h->async_pending = false; }
    return render_run(h->render, h->device, frames, n, prims, n_prims, outs, h->stream, launch_ms);
}
