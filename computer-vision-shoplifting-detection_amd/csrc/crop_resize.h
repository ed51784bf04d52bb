// Person crops (include/mi355_yolo.h "crops"): the rules of cutting a rectangle out of a BGR frame and resampling it,
// stated once for the kernel (crop_kernels.hip) and its host twin (crops_host.cpp).  Integers only on both targets: the one floating
// point step of cv2.resize(INTER_LINEAR) -- the tap tables -- is made on the host (crop_tap_table below, which is also what
// engine_internal.h:resize_table builds the letterbox kernel's tables with) and travels with the descriptors, so kernel and twin read
// the same numbers.
//
// A crop is one CropDesc.  Its output is out_h x out_w pixels; the INNER region in_h x in_w at (off_y, off_x) receives the rectangle
// [y1, y1 + ch) x [x1, x1 + cw) of the frame, everything else is `fill`:
//   xtab < 0   copy: in_h x in_w == ch x cw (native crops, and a resize to the crop's own size)
//   else       OpenCV's 11-bit fixed point: per destination index a source index s and two taps (a0, a1), the second tap at
//              min(s + 1, side - 1) -- clamped at the CROP's edge, never the frame's; horizontal pass in int32, vertical pass
//              (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2.
// An empty rectangle (cw == 0 or ch == 0) has an empty inner region: the whole output is `fill`.
// Offsets inside a frame are 32-bit: the checks refuse frames and outputs of 2 GiB or more.
#pragma once
#include <stdint.h>

#ifndef MI355_HD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MI355_HD __host__ __device__ __forceinline__
#else
#define MI355_HD inline
#endif
#endif

namespace mi355 {

constexpr int kCropMaxSide = 1 << 14;           // of a frame and of an output
constexpr int kCropThreads = 256;
constexpr int kCropItemsPerThread = 4;          // units of (up to) four output bytes a lane handles

struct CropDesc {
    const uint8_t* src;                         // first pixel of the FRAME (or of its staged rows: y1 counts from there)
    uint8_t* dst;
    int src_pitch, dst_pitch;
    int x1, y1, cw, ch;                         // the rectangle
    int out_w, out_h;
    int in_w, in_h, off_x, off_y;               // the inner region of the output
    int xtab, ytab;                             // first int32 of the x / y tap table (3 per destination index), -1: copy
    int fill;
    int blk0;                                   // first block of the launch that works on this crop
    int units;                                  // units per output row: (3 out_w + 6) / 4
    int pad_;
};

// units of one output row: a unit is an aligned dword of the destination, so a row whose address is a (mod 4) spans ceil((3 w + a) / 4)
MI355_HD int crop_row_units(int out_w) { return (3 * out_w + 6) / 4; }

// byte j (0 .. 3 out_w) of output row y
MI355_HD unsigned crop_byte(const CropDesc& d, const int* __restrict__ tabs, int y, int j) {
    const int px = j / 3, c = j - px * 3;
    const int ix = px - d.off_x, iy = y - d.off_y;
    if ((unsigned)ix >= (unsigned)d.in_w || (unsigned)iy >= (unsigned)d.in_h) return (unsigned)d.fill;
    const uint8_t* base = d.src + (uint32_t)(d.y1 * d.src_pitch + d.x1 * 3);
    if (d.xtab < 0) return base[(uint32_t)(iy * d.src_pitch + ix * 3 + c)];
    const int* xt = tabs + d.xtab + ix * 3;
    const int* yt = tabs + d.ytab + iy * 3;
    const int sx0 = xt[0], sx1 = sx0 + 1 < d.cw ? sx0 + 1 : d.cw - 1;
    const int sy0 = yt[0], sy1 = sy0 + 1 < d.ch ? sy0 + 1 : d.ch - 1;
    const uint8_t* r0 = base + (uint32_t)(sy0 * d.src_pitch);
    const uint8_t* r1 = base + (uint32_t)(sy1 * d.src_pitch);
    const int h0 = (int)r0[sx0 * 3 + c] * xt[1] + (int)r0[sx1 * 3 + c] * xt[2];
    const int h1 = (int)r1[sx0 * 3 + c] * xt[1] + (int)r1[sx1 * 3 + c] * xt[2];
    int v = (((yt[1] * (h0 >> 4)) >> 16) + ((yt[2] * (h1 >> 4)) >> 16) + 2) >> 2;
    v = v < 0 ? 0 : v > 255 ? 255 : v;
    return (unsigned)v;
}

}  // namespace mi355

// ---- host only from here on ---------------------------------------------------------------------------------------------------------------
#include <cmath>
#include <string>
#include <vector>

#include "../../include/mi355_yolo.h"
namespace mi355 {

// cv2.resize(INTER_LINEAR) coefficients, 3 int32 per destination index: source index, two taps in 1/2048 units: double for
// (d + 0.5) * scale - 0.5, float32 from there on.  The one builder of such tables (engine_internal.h:resize_table calls it); it lives
// here because this header also builds without HIP.
inline void crop_tap_table(int dn, int sn, int* tab) {
    const double scale = (double)sn / dn;
    for (int d = 0; d < dn; ++d) {
        float fx = (float)((d + 0.5) * scale - 0.5);
        int s = (int)std::floor(fx);
        fx -= (float)s;
        if (s < 0) { s = 0; fx = 0.f; }
        if (s >= sn - 1) { s = sn - 1; fx = 0.f; }
        tab[d * 3] = s;
        tab[d * 3 + 1] = (int)std::lrintf((1.f - fx) * 2048.f);
        tab[d * 3 + 2] = (int)std::lrintf(fx * 2048.f);
    }
}

// the host twin of one crop
inline void crop_host(const CropDesc& d, const int* tabs) {
    for (int y = 0; y < d.out_h; ++y) {
        uint8_t* row = d.dst + (size_t)y * d.dst_pitch;
        for (int j = 0; j < 3 * d.out_w; ++j) row[j] = (uint8_t)crop_byte(d, tabs, y, j);
    }
}

// ---- one call: what the checks leave behind for the host twin or the GPU half

struct CropPlan {
    std::vector<CropDesc> desc;                 // src / dst: the caller's pointers
    std::vector<int> tabs;                      // every crop's tap tables
    std::vector<int> frame_of;                  // crop -> frame
    std::vector<int> row0, row1;                // per frame: the rows [row0, row1) its rectangles span (row1 <= row0: none)
    long long blocks = 0;                       // of the launch
};
// crops_host.cpp: checks (MI355_EINVAL with a message, nothing written), descriptors and tables; then the host twin (device < 0) or
// crops_run_gpu (crop_kernels.hip) with `ctx`, a CropCtx or NULL for scratch of the call's own
int crops_call(void* ctx, int device, const mi355_render_frame* frames, int n, const int32_t* const* rects, const int* n_rects,
               const mi355_crop_spec* spec, const mi355_render_out* outs, void* stream, float* launch_ms);
int crops_run_gpu(void* ctx, int device, const mi355_render_frame* frames, int n, const mi355_render_out* outs, CropPlan& plan, void* stream,
                  float* launch_ms);

}  // namespace mi355
