// 4:2:0 YUV (NV12 / I420) -> dense BGR at ingest: what cv2.cvtColor(COLOR_YUV2BGR_NV12 / _I420) computes, BT.601 limited
// range in 20-bit fixed point, one (U, V) sample per 2x2 block of Y, no chroma interpolation.  ONE statement of the arithmetic,
// yuv_block, compiled for both targets: the kernel's two paths and the host twin (device = -1) all convert their blocks with it.
// The kernel is descriptor-driven (one launch converts all frames of a chunk, whatever their sizes: blockIdx.y = frame) and writes
// exactly H * W * 3 bytes per frame.  No LDS, no atomics.
#include "common.h"

namespace mi355 {
namespace {

constexpr int YUV_CY = 1220542, YUV_CUB = 2116026, YUV_CUG = -409993, YUV_CVG = -852492, YUV_CVR = 1673527, YUV_SHIFT = 20;

// sat_u8(sum >> 20) with the arithmetic (floor) shift of the statement, written as clamp-then-shift: a sum below 0 gives 0, one from
// 256 << 20 on gives 255, and in between the sign bit is clear, so the logical shift is the arithmetic one.  (Shift-then-clamp of two
// channels is what hipcc for gfx950 folds into its packed shift-and-saturate instruction, whose upper result half it then takes for
// zero when it ORs the pixel together; on the MI355X that half came back non-zero.  This order keeps the fold from forming.)
__host__ __device__ inline unsigned yuv_sat(int sum) {
    constexpr int top = (256 << YUV_SHIFT) - 1;
    return (unsigned)(sum < 0 ? 0 : sum > top ? top : sum) >> YUV_SHIFT;
}

// one pixel: B | G << 8 | R << 16 from its Y and the block's chroma terms (rounding constant included)
__host__ __device__ inline unsigned yuv_px(int Y, int ruv, int guv, int buv) {
    const int yy = (Y > 16 ? Y - 16 : 0) * YUV_CY;
    return yuv_sat(yy + buv) | (yuv_sat(yy + guv) << 8) | (yuv_sat(yy + ruv) << 16);
}

// One 2x2 block: its four Y samples and its (U, V) -> the two pixels of the upper and of the lower row, 6 bytes each in the low 48 bits
// (B G R B G R, first byte lowest).  All intermediates fit int32.
__host__ __device__ inline void yuv_block(int y00, int y01, int y10, int y11, int U, int V, unsigned long long& top, unsigned long long& bot) {
    const int uu = U - 128, vv = V - 128, half = 1 << (YUV_SHIFT - 1);
    const int ruv = half + YUV_CVR * vv, guv = half + YUV_CVG * vv + YUV_CUG * uu, buv = half + YUV_CUB * uu;
    top = (unsigned long long)yuv_px(y00, ruv, guv, buv) | ((unsigned long long)yuv_px(y01, ruv, guv, buv) << 24);
    bot = (unsigned long long)yuv_px(y10, ruv, guv, buv) | ((unsigned long long)yuv_px(y11, ruv, guv, buv) << 24);
}

// block (bx, by) of frame f with byte accesses: the generic path's lane and the host twin's loop body
__host__ __device__ inline void yuv_block_bytes(const YuvFrameDesc& f, int bx, int by) {
    const uint8_t* y0 = f.y + (size_t)(2 * by) * f.y_stride + 2 * bx;
    const uint8_t* y1 = y0 + f.y_stride;
    int U, V;
    if (f.format == 1) { const uint8_t* c = f.u + (size_t)by * f.uv_stride + 2 * bx; U = c[0]; V = c[1]; }
    else { U = f.u[(size_t)by * f.uv_stride + bx]; V = f.v[(size_t)by * f.uv_stride + bx]; }
    unsigned long long top, bot;
    yuv_block(y0[0], y0[1], y1[0], y1[1], U, V, top, bot);
    uint8_t* d0 = f.dst + ((size_t)(2 * by) * f.W + 2 * bx) * 3;
    uint8_t* d1 = d0 + (size_t)f.W * 3;
    for (int i = 0; i < 6; ++i) { d0[i] = (uint8_t)(top >> (8 * i)); d1[i] = (uint8_t)(bot >> (8 * i)); }
}

// Vector path: a lane owns 16 pixels x 2 rows = 8 blocks.  Two 16-byte Y loads (one per row), 16 bytes of chroma (NV12: one 16-byte
// load; I420: two 8-byte loads), three 16-byte stores per output row.  Adjacent lanes take adjacent 16-pixel groups of a row pair, so
// every load instruction of a wave reads one contiguous run and the three stores of a row together cover one contiguous run of 48 bytes
// per lane.  Needs W % 16 == 0 and 16-byte aligned plane bases, strides and dst (8 for I420 chroma): yuv_vector_ok.
__device__ __forceinline__ void yuv_lane16(const YuvFrameDesc& f, int gx, int by) {
    const uint8_t* yp = f.y + (size_t)(2 * by) * f.y_stride + 16 * gx;
    const uint4 ya = *reinterpret_cast<const uint4*>(yp), yb = *reinterpret_cast<const uint4*>(yp + f.y_stride);
    const unsigned y0w[4] = {ya.x, ya.y, ya.z, ya.w}, y1w[4] = {yb.x, yb.y, yb.z, yb.w};
    unsigned uw[2], vw[2];                 // the 8 U and the 8 V samples, one byte each
    if (f.format == 1) {
        const uint4 c = *reinterpret_cast<const uint4*>(f.u + (size_t)by * f.uv_stride + 16 * gx);
        const unsigned cw[4] = {c.x, c.y, c.z, c.w};
        uw[0] = uw[1] = vw[0] = vw[1] = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {      // U V U V ...: sample k sits in the bytes 2k, 2k + 1
            const unsigned pair = cw[k >> 1] >> (16 * (k & 1));
            uw[k >> 2] |= (pair & 255u) << (8 * (k & 3));
            vw[k >> 2] |= ((pair >> 8) & 255u) << (8 * (k & 3));
        }
    } else {
        const uint2 cu = *reinterpret_cast<const uint2*>(f.u + (size_t)by * f.uv_stride + 8 * gx);
        const uint2 cv = *reinterpret_cast<const uint2*>(f.v + (size_t)by * f.uv_stride + 8 * gx);
        uw[0] = cu.x; uw[1] = cu.y; vw[0] = cv.x; vw[1] = cv.y;
    }
    unsigned r0[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, r1[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 8; ++k) {          // block k = pixels 2k, 2k + 1: 48 bits at bit 48k of a row's 384
        const unsigned a = y0w[k >> 1] >> (16 * (k & 1)), b = y1w[k >> 1] >> (16 * (k & 1));
        const int U = (int)((uw[k >> 2] >> (8 * (k & 3))) & 255u), V = (int)((vw[k >> 2] >> (8 * (k & 3))) & 255u);
        unsigned long long top, bot;
        yuv_block((int)(a & 255u), (int)((a >> 8) & 255u), (int)(b & 255u), (int)((b >> 8) & 255u), U, V, top, bot);
        const int w = (48 * k) >> 5, s = (48 * k) & 31;                    // s is 0 or 16: 48 bits span exactly two words
        r0[w] |= (unsigned)(top << s); r0[w + 1] |= (unsigned)(top >> (32 - s));
        r1[w] |= (unsigned)(bot << s); r1[w + 1] |= (unsigned)(bot >> (32 - s));
    }
    uint4* d0 = reinterpret_cast<uint4*>(f.dst + ((size_t)(2 * by) * f.W + 16 * gx) * 3);
    uint4* d1 = reinterpret_cast<uint4*>(f.dst + ((size_t)(2 * by + 1) * f.W + 16 * gx) * 3);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        d0[q] = make_uint4(r0[4 * q], r0[4 * q + 1], r0[4 * q + 2], r0[4 * q + 3]);
        d1[q] = make_uint4(r1[4 * q], r1[4 * q + 1], r1[4 * q + 2], r1[4 * q + 3]);
    }
}

__global__ __launch_bounds__(256) void yuv_to_bgr_kernel(const YuvFrameDesc* __restrict__ frames) {
    const YuvFrameDesc f = frames[blockIdx.y];
    const int per_row = f.vec ? f.W >> 4 : f.W >> 1;                       // lanes per row pair
    const long total = (long)(f.H >> 1) * per_row;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int by = (int)(i / per_row), x = (int)(i - (long)by * per_row);
        if (f.vec) yuv_lane16(f, x, by);
        else yuv_block_bytes(f, x, by);
    }
}

}  // namespace

bool yuv_vector_ok(const YuvFrameDesc& f) {
    auto al = [](const void* p, size_t m) { return ((size_t)p & (m - 1)) == 0; };
    if ((f.W & 15) || !al(f.y, 16) || (f.y_stride & 15) || !al(f.dst, 16)) return false;
    if (f.format == 1) return al(f.u, 16) && (f.uv_stride & 15) == 0;
    return al(f.u, 8) && al(f.v, 8) && (f.uv_stride & 7) == 0;
}

const char* launch_yuv_to_bgr(const YuvFrameDesc* frames_dev, const YuvFrameDesc* frames_host, int B, hipStream_t st) {
    for (int b0 = 0; b0 < B; b0 += 32768) {                                 // grid.y is limited to 65535
        const int nb = B - b0 < 32768 ? B - b0 : 32768;
        long most = 1;
        for (int b = b0; b < b0 + nb; ++b) {
            const YuvFrameDesc& f = frames_host[b];
            const long lanes = (long)(f.H >> 1) * (f.vec ? f.W >> 4 : f.W >> 1);
            most = lanes > most ? lanes : most;
        }
        const unsigned gx = (unsigned)((most + 255) / 256 < 4096 ? (most + 255) / 256 : 4096);
        hipLaunchKernelGGL(yuv_to_bgr_kernel, dim3(gx, (unsigned)nb), dim3(256), 0, st, frames_dev + b0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hipGetErrorString(e);
    }
    return nullptr;
}

void yuv_to_bgr_host(const YuvFrameDesc* frames, int B) {
    for (int b = 0; b < B; ++b)
        for (int by = 0; by < frames[b].H / 2; ++by)
            for (int bx = 0; bx < frames[b].W / 2; ++bx) yuv_block_bytes(frames[b], bx, by);
}

}  // namespace mi355
