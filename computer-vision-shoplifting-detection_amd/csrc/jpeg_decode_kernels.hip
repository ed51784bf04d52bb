// JPEG ingest: baseline JPEG streams in host memory in, dense BGR frames out.  Three launches per call, whatever the
// number, sizes and layouts of the frames (descriptor-driven, blockIdx.y = frame):
//   entropy  one lane per restart segment, in blocks of one wave so that a frame's segments spread over the CUs.  The frame's four Huffman
//            tables (8-bit look-ahead, maxcode / valptr behind it) and the block's segment offsets are staged in LDS; a lane fetches its
//            bytes as aligned 32-bit words, unstuffs them into a 64-bit window and stores only non-zero coefficients: the coefficient
//            buffer was zeroed by a memset on the call's stream.  A stream without restart markers is one segment on one lane.
//   idct     one block of 256 lanes per run of 24 blocks: coefficients staged and dequantised into LDS, 192 lanes run the column pass and
//            then the row pass, one 8-vector each, and every lane stores one row of 8 samples to its component's plane.
//   colour   one lane per four pixels of a row: chroma upsampling (the triangle filter reads its neighbours across MCU borders from the
//            planes), colour conversion, three 32-bit stores where the row is aligned.
// entropy = host replaces the first launch by the twin's segment routine on the calling thread; the coefficients travel with the
// descriptors.  The rules themselves are jpeg_decode.h's, shared with the host twin (device = -1).
#include "engine_internal.h"
#include "jpeg_decode.h"

namespace mi355 {
namespace {

constexpr int kDecLanes = 256;
constexpr int kDecGroupBlocks = 24;
constexpr int kDecBlkStride = 72, kDecRowStride = 9;      // LDS layout of a staged block: with rows of 9 ints a half-wave hits 32 different banks in both passes

__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const JpegDecFrame* __restrict__ frames) {
    const JpegDecFrame& f = frames[blockIdx.y];
    const int s0 = (int)blockIdx.x * 64;
    if (!f.lanes || s0 >= f.nseg) return;                              // block-uniform
    const int t = (int)threadIdx.x;
    __shared__ JpegHuff s_h[4];
    __shared__ uint32_t s_seg[128];
    static_assert(sizeof(JpegHuff) % 4 == 0, "tables are copied as words");
    const uint32_t* src = reinterpret_cast<const uint32_t*>(f.huff);
    uint32_t* dst = reinterpret_cast<uint32_t*>(s_h);
    for (int i = t; i < (int)(4 * sizeof(JpegHuff) / 4); i += 64) dst[i] = src[i];
    const int seg = s0 + t;
    if (seg < f.nseg) { s_seg[2 * t] = f.seg[2 * seg]; s_seg[2 * t + 1] = f.seg[2 * seg + 1]; }
    __syncthreads();
    if (seg >= f.nseg) return;
    const long long mcus = (long long)f.mcus_x * f.mcus_y, mcu0 = (long long)seg * f.seg_mcus;
    const int nm = (int)(mcus - mcu0 < f.seg_mcus ? mcus - mcu0 : f.seg_mcus);
    JpegFetchWords fetch{reinterpret_cast<const uint32_t*>(f.scan)};
    const int st = jpeg_dec_segment(f, s_h, fetch, s_seg[2 * t], s_seg[2 * t + 1], mcu0, nm, f.coef);
    if (st) *f.status = st;
}

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const JpegDecFrame* __restrict__ frames) {
    const JpegDecFrame& f = frames[blockIdx.y];
    const long long nblk = jpeg_dec_blocks(f), b0 = (long long)blockIdx.x * kDecGroupBlocks;
    if (b0 >= nblk) return;                                            // block-uniform
    const int t = (int)threadIdx.x;
    __shared__ int s_blk[kDecGroupBlocks * kDecBlkStride];
    __shared__ uint8_t s_q[3][64], s_zz[64];
    __shared__ int s_narrow[kDecGroupBlocks];
    if (t < 192) s_q[t >> 6][t & 63] = f.q[t >> 6][t & 63];
    else s_zz[t - 192] = f.zigzag[t - 192];
    __syncthreads();
    const int ny = f.ncomp == 1 ? 1 : f.hs * f.vs;
    for (int i = t; i < kDecGroupBlocks * 64; i += kDecLanes) {
        const int b = i >> 6, k = i & 63, nat = s_zz[k];
        const long long gb = b0 + b;
        int v = 0;
        if (gb < nblk) {
            const int j = (int)(gb % f.bpm), c = j < ny ? 0 : j - ny + 1;
            v = (int)f.coef[gb * 64 + k] * s_q[c][k];
        }
        s_blk[b * kDecBlkStride + (nat >> 3) * kDecRowStride + (nat & 7)] = v;
    }
    __syncthreads();
    const int b = t >> 3, i8 = t & 7;
    if (t < kDecGroupBlocks * 8) {                                     // waves 0 .. 2 whole
        int* col = s_blk + b * kDecBlkStride + i8;
        int v[8], sum = 0;                                             // |coef * step| < 2^23: eight of them, then eight columns, fit
#pragma unroll
        for (int k = 0; k < 8; ++k) { v[k] = col[k * kDecRowStride]; sum += v[k] < 0 ? -v[k] : v[k]; }
        sum += __shfl_xor(sum, 1, 64); sum += __shfl_xor(sum, 2, 64); sum += __shfl_xor(sum, 4, 64);
        const bool narrow = sum <= (int)kJpegIdctNarrowSum;
        if (i8 == 0) s_narrow[b] = narrow;
        jpeg_idct_pass(v, 11, narrow);
#pragma unroll
        for (int k = 0; k < 8; ++k) col[k * kDecRowStride] = v[k];
    }
    __syncthreads();
    if (t < kDecGroupBlocks * 8 && b0 + b < nblk) {
        const int* row = s_blk + b * kDecBlkStride + i8 * kDecRowStride;
        int v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = row[k];
        jpeg_idct_pass(v, 18, s_narrow[b] != 0);
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { lo |= (uint32_t)jpeg_clamp255(v[k] + 128) << (8 * k); hi |= (uint32_t)jpeg_clamp255(v[k + 4] + 128) << (8 * k); }
        const long long gb = b0 + b, mcu = gb / f.bpm;
        const int j = (int)(gb - mcu * f.bpm), my = (int)(mcu / f.mcus_x), mx = (int)(mcu - (long long)my * f.mcus_x);
        int c, x0, y0;
        jpeg_dec_block_place(f, mx, my, j, c, x0, y0);
        // planes are 256-byte aligned, their rows and x0 multiples of 8: one 8-byte store
        *reinterpret_cast<uint2*>(f.plane[c] + (size_t)(y0 + i8) * f.pw[c] + x0) = make_uint2(lo, hi);
    }
}

__global__ __launch_bounds__(256) void jpeg_colour_kernel(const JpegDecFrame* __restrict__ frames) {
    const JpegDecFrame& f = frames[blockIdx.y];
    const int qw = (f.W + 3) >> 2;
    const long long q = (long long)blockIdx.x * kDecLanes + threadIdx.x;
    if (q >= (long long)qw * f.H) return;
    const int y = (int)(q / qw), x = (int)(q - (long long)y * qw) * 4;
    const int np = jpeg_min(4, f.W - x);
    uint8_t* o = f.out + (size_t)y * f.pitch + (size_t)x * 3;
    uint32_t w[3] = {0u, 0u, 0u};
    for (int i = 0; i < np; ++i) {
        int b, g, r;
        jpeg_dec_pixel(f, x + i, y, b, g, r);
        const int at = i * 3;
        w[at >> 2] |= (uint32_t)b << (8 * (at & 3));
        w[(at + 1) >> 2] |= (uint32_t)g << (8 * ((at + 1) & 3));
        w[(at + 2) >> 2] |= (uint32_t)r << (8 * ((at + 2) & 3));
    }
    if (np == 4 && (reinterpret_cast<uintptr_t>(o) & 3u) == 0) {
        uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
        o4[0] = w[0]; o4[1] = w[1]; o4[2] = w[2];
    } else {
        for (int i = 0; i < np * 3; ++i) o[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
    }
}

constexpr size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

// The GPU half of one call; the streams are parsed and every argument checked (jpeg_dec_call).  lanes[i]: frame i's entropy stage runs
// on the GPU.  outs (BGR) or coefs (the entropy stage alone, host int16) is given.
int jpeg_dec_run_gpu(JpegDecCtx* ctxp, int device, std::vector<JpegParsed>& P, const mi355_jpeg_stream* streams, int n, const int* lanes,
                     const mi355_render_out* outs, int16_t* const* coefs, int* status, void* stream, float* launch_ms) {
    hipStream_t st = (hipStream_t)stream;
    JpegDecCtx local;
    JpegDecCtx& ctx = ctxp ? *ctxp : local;
    struct Free { JpegDecCtx* c; ~Free() { if (c) jpeg_dec_ctx_free(*c); } } free_local{ctxp ? nullptr : &local};
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return fail(MI355_EHIP, "no HIP device: the JPEG decode kernels need an MI355X (device = -1 runs their host twin)"); }
    if (device >= ndev) return fail(MI355_EINVAL, "jpeg decode: device out of range");
    HIPCHK(hipSetDevice(device));
    if (launch_ms) *launch_ms = 0.f;
    // the image, built in pinned memory and uploaded in one copy: [descriptors | Huffman tables | status | per frame: segment offsets,
    // scan bytes (lanes) or coefficients (host entropy)]; behind it on the device: [coefficients of the lane frames | planes | host outputs]
    const size_t huff_off = al256((size_t)n * sizeof(JpegDecFrame)), stat_off = al256(huff_off + (size_t)n * 4 * sizeof(JpegHuff));
    size_t at = al256(stat_off + (size_t)n * 4);
    std::vector<size_t> seg_off((size_t)n), data_off((size_t)n), coef_off((size_t)n), plane_off((size_t)n * 3, 0), out_off((size_t)n, 0);
    for (int i = 0; i < n; ++i) {
        const JpegDecFrame& f = P[i].f;
        if (lanes[i]) {
            seg_off[i] = at; at = al256(at + (size_t)f.nseg * 8);
            data_off[i] = at; at = al256(at + (size_t)(P[i].scan_end - P[i].scan_begin) + 8);
        } else { coef_off[i] = at; at = al256(at + (size_t)jpeg_dec_blocks(f) * 128); }
    }
    const size_t img_bytes = at, zero_off = at;
    for (int i = 0; i < n; ++i)
        if (lanes[i]) { coef_off[i] = at; at = al256(at + (size_t)jpeg_dec_blocks(P[i].f) * 128); }
    const size_t zero_bytes = at - zero_off;
    size_t back_bytes = 0;
    std::vector<size_t> back((size_t)n, 0);
    long long most_seg = 0, most_grp = 1, most_quad = 1;
    for (int i = 0; i < n; ++i) {
        JpegDecFrame& f = P[i].f;
        if (outs) {
            for (int c = 0; c < f.ncomp; ++c) {
                f.pw[c] = f.mcus_x * 8 * (c ? 1 : f.hs); f.ph[c] = f.mcus_y * 8 * (c ? 1 : f.vs);
                plane_off[3 * i + c] = at; at = al256(at + (size_t)f.pw[c] * f.ph[c]);
            }
            if (!outs[i].on_device) { out_off[i] = at; at = al256(at + (size_t)f.H * f.W * 3); back[i] = back_bytes; back_bytes = al256(back_bytes + (size_t)f.H * f.W * 3); }
        }
        if (lanes[i]) most_seg = std::max(most_seg, (long long)f.nseg);
        most_grp = std::max(most_grp, (jpeg_dec_blocks(f) + kDecGroupBlocks - 1) / kDecGroupBlocks);
        most_quad = std::max(most_quad, ((long long)((f.W + 3) / 4) * f.H + kDecLanes - 1) / kDecLanes);
    }
    if (most_grp > 0x7FFFFFFFll || most_quad > 0x7FFFFFFFll) return fail(MI355_EINVAL, "jpeg decode: a frame is too large for one launch");
    if (buf_grow(ctx.d_work, at, at + at / 4) < 0 || buf_grow(ctx.h_img, img_bytes, img_bytes + img_bytes / 4) < 0 ||
        buf_grow(ctx.h_out, back_bytes, back_bytes + back_bytes / 4) < 0)
        return fail(MI355_EHIP, "jpeg decode: out of device or pinned memory (" + std::to_string(at) + " bytes of scratch)");
    uint8_t* base = ctx.d_work.p;
    uint8_t* img = ctx.h_img.p;
    std::vector<int> host_status((size_t)n, 0);
    std::memset(img + stat_off, 0, (size_t)n * 4);
    for (int i = 0; i < n; ++i) {
        JpegDecFrame& f = P[i].f;
        f.lanes = lanes[i];
        for (int k = 0; k < 64; ++k) f.zigzag[k] = kJpegZigzag[k];
        f.huff = (const JpegHuff*)(base + huff_off) + (size_t)i * 4;
        std::memcpy(img + huff_off + (size_t)i * 4 * sizeof(JpegHuff), P[i].huff, 4 * sizeof(JpegHuff));
        f.status = (int*)(base + stat_off) + i;
        f.coef = (int16_t*)(base + coef_off[i]);
        if (lanes[i]) {
            const size_t nb = (size_t)(P[i].scan_end - P[i].scan_begin);
            f.seg = (const uint32_t*)(base + seg_off[i]); f.scan = base + data_off[i];
            std::memcpy(img + seg_off[i], P[i].seg.data(), (size_t)f.nseg * 8);
            std::memcpy(img + data_off[i], streams[i].data + P[i].scan_begin, nb);
            std::memset(img + data_off[i] + nb, 0, 8);
        } else {
            f.seg = nullptr; f.scan = nullptr;
            host_status[i] = jpeg_dec_coefficients_host(P[i], streams[i].data, (int16_t*)(img + coef_off[i]));
        }
        for (int c = 0; c < 3; ++c) f.plane[c] = outs && c < f.ncomp ? base + plane_off[3 * i + c] : nullptr;
        if (outs) {
            f.out = outs[i].on_device ? (uint8_t*)outs[i].data : base + out_off[i];
            f.pitch = outs[i].on_device ? outs[i].row_stride : 3 * f.W;
        }
        std::memcpy(img + (size_t)i * sizeof(JpegDecFrame), &f, sizeof(JpegDecFrame));
    }
    HIPCHK(hipMemcpyAsync(base, img, img_bytes, hipMemcpyHostToDevice, st));
    if (launch_ms && !ctx.ev0) { HIPCHK(hipEventCreate(&ctx.ev0)); HIPCHK(hipEventCreate(&ctx.ev1)); }
    if (launch_ms) HIPCHK(hipEventRecord(ctx.ev0, st));
    const JpegDecFrame* dd = (const JpegDecFrame*)base;
    auto launched = [&]() -> const char* { const hipError_t e = hipGetLastError(); return e != hipSuccess ? hipGetErrorString(e) : nullptr; };
    if (most_seg > 0) {
        HIPCHK(hipMemsetAsync(base + zero_off, 0, zero_bytes, st));
        hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)((most_seg + 63) / 64), (unsigned)n), dim3(64), 0, st, dd);
        KCHK(launched());
    }
    if (outs) {
        hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)most_grp, (unsigned)n), dim3(kDecLanes), 0, st, dd);
        KCHK(launched());
        hipLaunchKernelGGL(jpeg_colour_kernel, dim3((unsigned)most_quad, (unsigned)n), dim3(kDecLanes), 0, st, dd);
        KCHK(launched());
    }
    if (launch_ms) HIPCHK(hipEventRecord(ctx.ev1, st));
    if (buf_grow(ctx.h_stat, (size_t)n * 4) < 0) return fail(MI355_EHIP, "jpeg decode: out of pinned memory");
    int* h_stat = (int*)ctx.h_stat.p;
    HIPCHK(hipMemcpyAsync(h_stat, base + stat_off, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    if (coefs)
        for (int i = 0; i < n; ++i) HIPCHK(hipMemcpyAsync(coefs[i], P[i].f.coef, (size_t)jpeg_dec_blocks(P[i].f) * 128, hipMemcpyDeviceToHost, st));
    if (outs)
        for (int i = 0; i < n; ++i)
            if (!outs[i].on_device) HIPCHK(hipMemcpyAsync(ctx.h_out.p + back[i], base + out_off[i], (size_t)P[i].f.H * P[i].f.W * 3, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (launch_ms) HIPCHK(hipEventElapsedTime(launch_ms, ctx.ev0, ctx.ev1));
    for (int i = 0; i < n; ++i) {
        const int s = lanes[i] ? h_stat[i] : host_status[i];
        if (status) status[i] = s;
        if (outs && !outs[i].on_device && !s) {
            const JpegDecFrame& f = P[i].f;
            for (int y = 0; y < f.H; ++y) std::memcpy((uint8_t*)outs[i].data + (size_t)y * outs[i].row_stride, ctx.h_out.p + back[i] + (size_t)y * f.W * 3, (size_t)f.W * 3);
        }
    }
    return MI355_OK;
}

void jpeg_dec_ctx_free(JpegDecCtx& ctx) {
    buf_free(ctx.d_work); buf_free(ctx.h_img); buf_free(ctx.h_out); buf_free(ctx.h_stat);
    if (ctx.ev0) { (void)hipEventDestroy(ctx.ev0); (void)hipEventDestroy(ctx.ev1); ctx.ev0 = ctx.ev1 = nullptr; }
}

}  // namespace mi355
