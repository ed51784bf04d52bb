// BoT-SORT global motion compensation on the GPU: pyramidal Lucas-Kanade tracking of sparse corners between two gray frames
// (what cv2.calcOpticalFlowPyrLK does for ultralytics/trackers/utils/gmc.py:GMC.apply_sparseoptflow, reached from
// /root/reference/model.py:38 through model.track).  The algorithm and its parameters are stated once, in numpy, in
// cvsd_amd/gmc.py:calc_optical_flow_pyr_lk_numpy; csrc/gmc_host.cpp is the same arithmetic as host loops.  On the host the
// 1000-corner budget of goodFeaturesToTrack costs 27 us per point -- 10-27 ms per frame, thirty times the whole detector pass
// (0.42 ms at batch 1), so the reference's frame loop (model.track -> CSV) ran at the tracker's pace.  Here every point is one
// wavefront: its 21 x 21 window is 441 pixels = 7 per lane, the window's I / Ix / Iy samples stay in registers for all
// iterations of a level, the 2 x 2 normal equations are wave reductions, all in float64 (the same formulae as the host code;
// window sums are associated differently -- lane-wise then butterfly -- so results agree to rounding, not bit for bit).
// The pyramids (5-tap Gaussian pyrDown, integer arithmetic: exact) are built by a kernel per level.
#include "../../include/mi355_yolo.h"
#include "dev_buf.h"

#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

#pragma clang fp contract(off)

namespace {

constexpr int kMaxLevels = 8;          // pyramid levels held (level 0 = the frame)
constexpr int kMaxPer = 7;             // window pixels per lane: win <= 21 (441 = 6.9 * 64; OpenCV's and Ultralytics' default window)

__device__ __forceinline__ int reflect101(int i, int n) {          // BORDER_REFLECT_101, any distance (as the host code)
    if (n == 1) return 0;
    while (i < 0 || i >= n) i = i < 0 ? -i : 2 * (n - 1) - i;
    return i;
}

// cv2.pyrDown on uint8: separable [1 4 6 4 1] / 16 twice, reflect-101 borders, every second pixel, (s + 128) >> 8
// blockIdx.y = frame of a batch (mi355_gmc_track_batch): planes of consecutive frames are `fstride` bytes apart (0 for one frame)
// one output pixel of pyrDown (shared by the single-frame / batch kernel and the per-camera one below: one statement of the arithmetic)
__device__ __forceinline__ uint8_t pyr_down_px(const uint8_t* src, int h, int w, int nw, int idx) {
    const int y = idx / nw, x = idx - y * nw;
    const int k[5] = {1, 4, 6, 4, 1};
    int s = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const uint8_t* row = src + (size_t)reflect101(2 * y + i - 2, h) * w;
        int r = 0;
#pragma unroll
        for (int j = 0; j < 5; ++j) r += k[j] * row[reflect101(2 * x + j - 2, w)];
        s += k[i] * r;
    }
    return (uint8_t)((s + 128) >> 8);
}
__global__ __launch_bounds__(256) void pyr_down_kernel(const uint8_t* src, int h, int w, uint8_t* dst, int nh, int nw, size_t fstride = 0) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= nh * nw) return;
    src += blockIdx.y * fstride; dst += blockIdx.y * fstride;
    dst[idx] = pyr_down_px(src, h, w, nw, idx);
}

struct LkArgs {
    const uint8_t* prev[kMaxLevels]; const uint8_t* cur[kMaxLevels];
    int h[kMaxLevels], w[kMaxLevels];
    int top, n, win, max_iters, width, height;
    double eps2, min_eig;
    const float* pts; float* next; uint8_t* status;
    // batch of frame pairs (blockIdx.y = pair; mi355_gmc_track_batch): pair p tracks n_arr[p] points from plane p into plane p + 1, the
    // planes of consecutive frames `pair_stride` bytes apart, its points / results at p * max_pts.  One pair: all zero / null.
    size_t pair_stride; int max_pts; const int* n_arr;
    // the view lk_point reads its frame pair through (the per-camera kernel has another: LkCamView)
    __device__ __forceinline__ const uint8_t* prev_at(int l) const { return prev[l]; }
    __device__ __forceinline__ const uint8_t* cur_at(int l) const { return cur[l]; }
    __device__ __forceinline__ int h_at(int l) const { return h[l]; }
    __device__ __forceinline__ int w_at(int l) const { return w[l]; }
};

// Sum over the 64 lanes, the same bits in every lane.  Four row_shr steps inside each row of 16 lanes (data-parallel-primitive moves:
// a few cycles each, against ~100 for the LDS-crossbar permute a generic shuffle becomes), two row broadcasts, one read of lane 63.
// The iteration of the Lucas-Kanade loop is latency-bound and does two of these back to back.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_add(double v) {
    const long long b = __builtin_bit_cast(long long, v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)b, CTRL, ROW_MASK, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, ROW_MASK, 0xf, true);
    const double o = __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned)lo);    // 0.0 where the source lane is outside the row / masked
    return v + o;
}
__device__ __forceinline__ double wave_sum(double v) {
    v = dpp_add<0x111, 0xf>(v);          // row_shr:1
    v = dpp_add<0x112, 0xf>(v);          // row_shr:2
    v = dpp_add<0x114, 0xf>(v);          // row_shr:4
    v = dpp_add<0x118, 0xf>(v);          // row_shr:8  -> lane 15 of every row holds the row's sum
    v = dpp_add<0x142, 0xa>(v);          // row_bcast:15 into rows 1 and 3
    v = dpp_add<0x143, 0xc>(v);          // row_bcast:31 into rows 2 and 3 -> lane 63 holds the total
    const long long b = __builtin_bit_cast(long long, v);
    const int lo = __builtin_amdgcn_readlane((int)b, 63), hi = __builtin_amdgcn_readlane((int)(b >> 32), 63);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned)lo);
}

// value of plane `kind` (0 = intensity, 1 = Scharr d/dx, 2 = Scharr d/dy of the same image) at integer position (y, x) of the
// reflect-padded plane: the host code pads the plane of gradients, so the position is reflected first and the stencil
// reflects its own neighbours
template <int KIND>
__device__ __forceinline__ double plane_at(const uint8_t* img, int h, int w, int y, int x) {
    y = reflect101(y, h); x = reflect101(x, w);
    if (KIND == 0) return (double)img[(size_t)y * w + x];
    const int ym = reflect101(y - 1, h), yp = reflect101(y + 1, h), xm = reflect101(x - 1, w), xp = reflect101(x + 1, w);
    auto A = [&](int yy, int xx) { return (int)img[(size_t)yy * w + xx]; };
    if (KIND == 1) return (double)(3 * (A(ym, xp) - A(ym, xm)) + 10 * (A(y, xp) - A(y, xm)) + 3 * (A(yp, xp) - A(yp, xm)));
    return (double)(3 * (A(yp, xm) - A(ym, xm)) + 10 * (A(yp, x) - A(ym, x)) + 3 * (A(yp, xp) - A(ym, xp)));
}

// this lane's samples of the win x win bilinear patch whose top-left corner is (px - half, py - half): window pixel k = lane + 64 j
template <int KIND>
__device__ __forceinline__ void patch(const uint8_t* img, int h, int w, double px, double py, int win, int lane, double (&out)[kMaxPer], int per) {
    const int half = win / 2;
    const double x = px - half, y = py - half;
    const double fx = floor(x), fy = floor(y);
    const int ix = (int)fx, iy = (int)fy;
    const double ax = x - fx, ay = y - fy;
    const double w00 = (1 - ay) * (1 - ax), w01 = (1 - ay) * ax, w10 = ay * (1 - ax), w11 = ay * ax;
    const int W2 = win * win;
#pragma unroll
    for (int j = 0; j < kMaxPer; ++j) {
        if (j >= per) break;
        const int k = lane + 64 * j;
        double v = 0.0;
        if (k < W2) {
            const int r = k / win, c = k - r * win;
            const int yy = iy + r, xx = ix + c;
            v = w00 * plane_at<KIND>(img, h, w, yy, xx) + w01 * plane_at<KIND>(img, h, w, yy, xx + 1) +
                w10 * plane_at<KIND>(img, h, w, yy + 1, xx) + w11 * plane_at<KIND>(img, h, w, yy + 1, xx + 1);
        }
        out[j] = v;
    }
}

// The iteration reads the current frame through a per-wavefront LDS copy of the neighbourhood it is walking in: (win + 1 + 2 M)^2
// reflect-padded intensities (bytes), refilled only when the window's corner leaves the margin M.  The values are those
// plane_at<0> returns, so the arithmetic -- and every bit of the result -- is that of reading global memory each time; what goes
// away is four byte loads with reflected addresses per window pixel per iteration (three quarters of the kernel's instructions).
constexpr int kMargin = 3;
constexpr int kRegMax = 21 + 1 + 2 * kMargin;          // region side for the largest window

__device__ __forceinline__ void fill_region(const uint8_t* img, int h, int w, int ry, int rx, int R, int lane, uint8_t* reg) {
    for (int k = lane; k < R * R; k += 64) {
        const int r = k / R, c = k - r * R;
        reg[k] = img[(size_t)reflect101(ry + r, h) * w + reflect101(rx + c, w)];
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// The previous frame's window samples of one level (I, Scharr Ix, Iy at the win x win bilinear positions around (px, py)), this lane's
// share.  patch<> evaluates every sample's four corners from global memory -- for the gradients six reflected byte loads per corner,
// 364 loads per lane and level, four fifths of the kernel's time.  Here each INTEGER position of the (win + 1)^2 grid is evaluated
// once: the image bytes the grid and its 3x3 stencils touch (a box of at most (win + 3)^2 pixels after reflection) are copied to LDS,
// the three planes (byte, int16, int16 -- the stencil sums are integers, so nothing is rounded) are built from that copy, and the
// bilinear samples read the planes.  Same integers, same float64 expression per sample: the same bits as patch<>.
constexpr int kGridMax = 21 + 1;                                   // win + 1
struct LkScratch {
    uint8_t box[(21 + 3) * (21 + 3)];                              // image bytes under the grid and its stencils
    uint8_t pI[kGridMax * kGridMax];
    short pIx[kGridMax * kGridMax], pIy[kGridMax * kGridMax];
};

__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ void setup_patches(const uint8_t* img, int h, int w, double px, double py, int win, int lane, uint8_t* box, uint8_t* pI,
                                              short* pIx, short* pIy, double (&I)[kMaxPer], double (&Ix)[kMaxPer], double (&Iy)[kMaxPer], int per) {
    const int half = win / 2, G = win + 1;
    const double x = px - half, y = py - half;
    const double fx = floor(x), fy = floor(y);
    const int ix = (int)fx, iy = (int)fy;
    const double ax = x - fx, ay = y - fy;
    const double w00 = (1 - ay) * (1 - ax), w01 = (1 - ay) * ax, w10 = ay * (1 - ax), w11 = ay * ax;
    // image rows / columns the grid's reflected positions fall on (wave-uniform), one pixel more on each side for the stencils
    int ylo = h, yhi = -1, xlo = w, xhi = -1;
    for (int r = 0; r < G; ++r) {
        const int yy = reflect101(iy + r, h), xx = reflect101(ix + r, w);
        ylo = min(ylo, yy); yhi = max(yhi, yy); xlo = min(xlo, xx); xhi = max(xhi, xx);
    }
    ylo = max(0, ylo - 1); yhi = min(h - 1, yhi + 1); xlo = max(0, xlo - 1); xhi = min(w - 1, xhi + 1);
    const int Hb = yhi - ylo + 1, Wb = xhi - xlo + 1;              // <= win + 3 each
    wave_lds_fence();                                              // the previous level's readers of the box and the planes are done
    for (int k = lane; k < Hb * Wb; k += 64) {
        const int r = k / Wb, c = k - r * Wb;
        box[k] = img[(size_t)(ylo + r) * w + (xlo + c)];
    }
    wave_lds_fence();
    auto A = [&](int yy, int xx) { return (int)box[(yy - ylo) * Wb + (xx - xlo)]; };
    for (int k = lane; k < G * G; k += 64) {
        const int r = k / G, c = k - r * G;
        const int yy = reflect101(iy + r, h), xx = reflect101(ix + c, w);
        const int ym = reflect101(yy - 1, h), yp = reflect101(yy + 1, h), xm = reflect101(xx - 1, w), xp = reflect101(xx + 1, w);
        pI[k] = (uint8_t)A(yy, xx);
        pIx[k] = (short)(3 * (A(ym, xp) - A(ym, xm)) + 10 * (A(yy, xp) - A(yy, xm)) + 3 * (A(yp, xp) - A(yp, xm)));
        pIy[k] = (short)(3 * (A(yp, xm) - A(ym, xm)) + 10 * (A(yp, xx) - A(ym, xx)) + 3 * (A(yp, xp) - A(ym, xp)));
    }
    wave_lds_fence();
    const int W2 = win * win;
#pragma unroll
    for (int j = 0; j < kMaxPer; ++j) {
        if (j >= per) break;
        const int k = lane + 64 * j;
        double vi = 0.0, vx = 0.0, vy = 0.0;
        if (k < W2) {
            const int r = k / win, c = k - r * win;
            const int q = r * G + c;
            vi = w00 * (double)pI[q] + w01 * (double)pI[q + 1] + w10 * (double)pI[q + G] + w11 * (double)pI[q + G + 1];
            vx = w00 * (double)pIx[q] + w01 * (double)pIx[q + 1] + w10 * (double)pIx[q + G] + w11 * (double)pIx[q + G + 1];
            vy = w00 * (double)pIy[q] + w01 * (double)pIy[q + 1] + w10 * (double)pIy[q + G] + w11 * (double)pIy[q + G + 1];
        }
        I[j] = vi; Ix[j] = vx; Iy[j] = vy;
    }
}

// one wavefront per point; block = kLkWaves wavefronts (4: eight or sixteen points per block, meant to leave more CUs to the detector
// pass this kernel runs beside, measured equal / 5-10 % slower on the track loop -- tools/lk_waves_ab.sh)
#ifndef MI355_LK_WAVES
#define MI355_LK_WAVES 4
#endif
constexpr int kLkWaves = MI355_LK_WAVES;
// point i of the frame pair `a` describes, on this wavefront (reg / sc: its LDS)
template <class A>
__device__ __forceinline__ void lk_point(const A& a, int i, int lane, uint8_t* reg, LkScratch& sc) {
    const int win = a.win, half = win / 2, W2 = win * win;
    const int per = (W2 + 63) / 64;
    const int R = win + 1 + 2 * kMargin;
    const double s = 1.0 / (double)(1 << 20);                    // OpenCV's scaling of the gradient products
    const double p0x = (double)a.pts[2 * i], p0y = (double)a.pts[2 * i + 1];
    bool ok = true;
    double nx = 0, ny = 0;
    double I[kMaxPer], Ix[kMaxPer], Iy[kMaxPer];
    int koff[kMaxPer];                                           // this lane's window pixels as offsets inside the region
#pragma unroll
    for (int j = 0; j < kMaxPer; ++j) {
        const int k = lane + 64 * j;
        const int r = k / win, c = k - r * win;
        koff[j] = (j < per && k < W2) ? r * R + c : -1;
    }
    for (int l = a.top; l >= 0; --l) {
        const int h = a.h_at(l), w = a.w_at(l);
        const double px = p0x / (double)(1 << l), py = p0y / (double)(1 << l);
        if (l == a.top) { nx = px; ny = py; } else { nx *= 2.0; ny *= 2.0; }
        const double tlx = floor(px - half), tly = floor(py - half);
        const bool inside = tlx >= -win && tlx < w && tly >= -win && tly < h;
        if (!inside) { if (l == 0) ok = false; continue; }
        const double cx = fmin(fmax(px, (double)-half), (double)(w - 1 + half));
        const double cy = fmin(fmax(py, (double)-half), (double)(h - 1 + half));
#if MI355_LK_GLOBAL_SETUP
        patch<0>(a.prev_at(l), h, w, cx, cy, win, lane, I, per);
        patch<1>(a.prev_at(l), h, w, cx, cy, win, lane, Ix, per);
        patch<2>(a.prev_at(l), h, w, cx, cy, win, lane, Iy, per);
#else
        setup_patches(a.prev_at(l), h, w, cx, cy, win, lane, sc.box, sc.pI, sc.pIx, sc.pIy, I, Ix, Iy, per);
#endif
        double a11 = 0, a12 = 0, a22 = 0;
#pragma unroll
        for (int j = 0; j < kMaxPer; ++j) {
            if (j >= per) break;
            a11 += Ix[j] * Ix[j]; a12 += Ix[j] * Iy[j]; a22 += Iy[j] * Iy[j];
        }
        a11 = wave_sum(a11) * s; a12 = wave_sum(a12) * s; a22 = wave_sum(a22) * s;
        const double det = a11 * a22 - a12 * a12;
        const double mineig = (a22 + a11 - sqrt((a11 - a22) * (a11 - a22) + 4 * a12 * a12)) / (2.0 * W2);
        if (!(mineig >= a.min_eig) || !(det >= (double)1.1920928955078125e-07)) { if (l == 0) ok = false; continue; }
        double pdx = 0, pdy = 0;
        int rx = 0, ry = 0; bool have_region = false;
        for (int it = 0; it < a.max_iters; ++it) {
            const double qx = floor(nx - half), qy = floor(ny - half);
            if (!(qx >= -win && qx < w && qy >= -win && qy < h)) { if (l == 0) ok = false; break; }
            const double ccx = fmin(fmax(nx, (double)-half), (double)(w - 1 + half));
            const double ccy = fmin(fmax(ny, (double)-half), (double)(h - 1 + half));
            // the window's top-left sample (as patch<0> derives it) and its bilinear weights
            const double x = ccx - half, y = ccy - half;
            const double fx = floor(x), fy = floor(y);
            const int ix = (int)fx, iy = (int)fy;
            const double ax = x - fx, ay = y - fy;
            const double w00 = (1 - ay) * (1 - ax), w01 = (1 - ay) * ax, w10 = ay * (1 - ax), w11 = ay * ax;
            if (!have_region || ix < rx || iy < ry || ix > rx + 2 * kMargin || iy > ry + 2 * kMargin) {
                __builtin_amdgcn_wave_barrier();                   // every lane is done reading the old region
                rx = ix - kMargin; ry = iy - kMargin;
                fill_region(a.cur_at(l), h, w, ry, rx, R, lane, reg);
                have_region = true;
            }
            const uint8_t* r0 = reg + (iy - ry) * R + (ix - rx);
            double b1 = 0, b2 = 0;
#pragma unroll
            for (int j = 0; j < kMaxPer; ++j) {
                if (j >= per) break;
                double Jv = 0.0;                                 // lanes past the window hold zeros in I / Ix / Iy too
                if (koff[j] >= 0) {
                    const uint8_t* q = r0 + koff[j];
                    Jv = w00 * (double)q[0] + w01 * (double)q[1] + w10 * (double)q[R] + w11 * (double)q[R + 1];
                }
                const double d = (Jv - I[j]) * 32.0;
                b1 += d * Ix[j]; b2 += d * Iy[j];
            }
            b1 = wave_sum(b1) * s; b2 = wave_sum(b2) * s;
            const double dx = (a12 * b2 - a22 * b1) / det, dy = (a12 * b1 - a11 * b2) / det;
            nx += dx; ny += dy;
            if (dx * dx + dy * dy <= a.eps2) break;
            if (it > 0 && fabs(dx + pdx) < 0.01 && fabs(dy + pdy) < 0.01) { nx -= dx * 0.5; ny -= dy * 0.5; break; }
            pdx = dx; pdy = dy;
        }
        __builtin_amdgcn_wave_barrier();
    }
    if (ok && (nx < 0 || ny < 0 || nx >= a.width || ny >= a.height)) ok = false;
    if (lane == 0) {
        a.next[2 * i] = (float)nx; a.next[2 * i + 1] = (float)ny;
        a.status[i] = ok ? 1 : 0;
    }
}

__global__ __launch_bounds__(64 * kLkWaves) void lk_kernel(LkArgs a) {
    __shared__ uint8_t region[kLkWaves][(kRegMax * kRegMax + 15) & ~15];
    __shared__ LkScratch scratch[kLkWaves];
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * kLkWaves + (threadIdx.x >> 6);
    const int pair = blockIdx.y;
    if (i >= (a.n_arr ? a.n_arr[pair] : a.n)) return;
    {
        const size_t po = (size_t)pair * a.pair_stride;
#pragma unroll
        for (int l = 0; l < kMaxLevels; ++l) { a.prev[l] += po; a.cur[l] += po; }
        const size_t qo = (size_t)pair * (size_t)a.max_pts;
        a.pts += 2 * qo; a.next += 2 * qo; a.status += qo;
    }
    lk_point(a, i, lane, region[threadIdx.x >> 6], scratch[threadIdx.x >> 6]);
}

// ---- frame preparation: cvtColor(BGR2GRAY) + resize(INTER_LINEAR) + the corner map of goodFeaturesToTrack -------------------
// gmc.py states these in numpy (bgr_to_gray, resize_linear, good_features_to_track); the kernels evaluate the same expressions
// in the same order (integers for luma and resize; float64 for the structure tensor, its sums taken in numpy's order), so the
// corner list is the numpy one.

// gray = (1868 B + 9617 G + 4899 R + 8192) >> 14, then INTER_LINEAR with 11-bit coefficients (tables from the host: source index,
// two taps per output column / row), both passes in cv2's fixed point: ((c0 * (h0 >> 4)) >> 16) + ((c1 * (h1 >> 4)) >> 16) + 2) >> 2
// (one output pixel per thread; the *_px functions are shared with the per-camera kernels further down)
__device__ __forceinline__ uint8_t gray_resize_px(const uint8_t* bgr, int H, int W, size_t row_stride, const int* xtab, const int* ytab, int ow, int resize,
                                                  int idx) {
    const int y = idx / ow, x = idx - y * ow;
    auto gray = [&](int yy, int xx) {
        const uint8_t* p = bgr + (size_t)yy * row_stride + (size_t)xx * 3;
        return (int)((p[0] * 1868 + p[1] * 9617 + p[2] * 4899 + 8192) >> 14);
    };
    if (!resize) return (uint8_t)gray(y, x);
    const int xi = xtab[3 * x], xa0 = xtab[3 * x + 1], xa1 = xtab[3 * x + 2];
    const int yi = ytab[3 * y], yb0 = ytab[3 * y + 1], yb1 = ytab[3 * y + 2];
    const int xj = min(xi + 1, W - 1), yj = min(yi + 1, H - 1);
    const int h0 = gray(yi, xi) * xa0 + gray(yi, xj) * xa1;
    const int h1 = gray(yj, xi) * xa0 + gray(yj, xj) * xa1;
    int v = (((yb0 * (h0 >> 4)) >> 16) + ((yb1 * (h1 >> 4)) >> 16) + 2) >> 2;
    v = v < 0 ? 0 : (v > 255 ? 255 : v);
    return (uint8_t)v;
}
__global__ __launch_bounds__(256) void gray_resize_kernel(const uint8_t* bgr, int H, int W, const int* xtab, const int* ytab, uint8_t* out, int oh, int ow,
                                                          int resize, size_t in_fstride = 0, size_t out_fstride = 0) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= oh * ow) return;
    bgr += blockIdx.y * in_fstride; out += blockIdx.y * out_fstride;
    out[idx] = gray_resize_px(bgr, H, W, (size_t)W * 3, xtab, ytab, ow, resize, idx);
}

// cornerMinEigenVal (3x3 Sobel scaled by 1 / (4 * block * 255), block x block box sums of the products, smaller eigenvalue) as
// float32, and its maximum over the plane (non-negative floats order like their bit patterns)
__device__ __forceinline__ float min_eig_px(const uint8_t* g, int h, int w, int idx) {
    const int y = idx / w, x = idx - y * w;
    const double sc = 1.0 / (4.0 * 3.0 * 255.0);
    auto G = [&](int yy, int xx) { return (double)g[(size_t)reflect101(yy, h) * w + reflect101(xx, w)]; };
    double sxx = 0.0, sxy = 0.0, syy = 0.0;                 // Python's sum(): 0 + p00 + p01 + ... in (i, j) row-major order
#pragma unroll
    for (int i = -1; i <= 1; ++i)
#pragma unroll
        for (int j = -1; j <= 1; ++j) {
            const int yy = reflect101(y + i, h), xx = reflect101(x + j, w);     // the product arrays are reflect-padded
            const double dx = ((G(yy - 1, xx + 1) - G(yy - 1, xx - 1)) + 2 * (G(yy, xx + 1) - G(yy, xx - 1)) + (G(yy + 1, xx + 1) - G(yy + 1, xx - 1))) * sc;
            const double dy = ((G(yy + 1, xx - 1) - G(yy - 1, xx - 1)) + 2 * (G(yy + 1, xx) - G(yy - 1, xx)) + (G(yy + 1, xx + 1) - G(yy - 1, xx + 1))) * sc;
            sxx += dx * dx; sxy += dx * dy; syy += dy * dy;
        }
    const double a = sxx * 0.5, b = sxy, c = syy * 0.5;
    return (float)((a + c) - sqrt((a - c) * (a - c) + b * b));
}
// block maximum of e (every thread of the 256-thread block calls), then one atomic per block
__device__ __forceinline__ void block_max_to(float e, unsigned* max_bits) {
    float m = e > 0.f ? e : 0.f;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    __shared__ float wm[4];
    if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(max_bits, __float_as_uint(fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]))));
}
__global__ __launch_bounds__(256) void min_eig_kernel(const uint8_t* g, int h, int w, float* eig, unsigned* max_bits, size_t g_fstride = 0) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    g += blockIdx.y * g_fstride; eig += (size_t)blockIdx.y * h * w; max_bits += blockIdx.y;
    float e = 0.f;
    if (idx < h * w) {
        e = min_eig_px(g, h, w, idx);
        eig[idx] = e;
    }
    block_max_to(e, max_bits);
}

// THRESH_TOZERO at quality * max, 3x3 non-maximum suppression (a corner equals the maximum of its neighbourhood), image border excluded
__device__ __forceinline__ uint8_t corner_mask_px(const float* eig, int h, int w, float mx, double quality, int idx) {
    const int y = idx / w, x = idx - y * w;
    const float thr = (float)((double)mx * quality);
    auto T = [&](int yy, int xx) {
        if (yy < 0 || yy >= h || xx < 0 || xx >= w) return -INFINITY;
        const float v = eig[(size_t)yy * w + xx];
        return v > thr ? v : 0.f;
    };
    const float v = T(y, x);
    float d = -INFINITY;
#pragma unroll
    for (int i = -1; i <= 1; ++i)
#pragma unroll
        for (int j = -1; j <= 1; ++j) d = fmaxf(d, T(y + i, x + j));
    const bool keep = mx > 0.f && v != 0.f && v == d && y > 0 && y < h - 1 && x > 0 && x < w - 1;
    return keep ? 1 : 0;
}
__global__ __launch_bounds__(256) void corner_mask_kernel(const float* eig, int h, int w, const unsigned* max_bits, double quality, uint8_t* ok) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= h * w) return;
    eig += (size_t)blockIdx.y * h * w; ok += (size_t)blockIdx.y * h * w; max_bits += blockIdx.y;
    ok[idx] = corner_mask_px(eig, h, w, __uint_as_float(*max_bits), quality, idx);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------
// Four entry points run the same step -- the one-shot calls on g_ctx, step_begin / step_finish, track_batch, and the multi-camera tick
// further down -- and each piece of it is stated once here: buffers, pyramid geometry, the launches, a camera's state, the host tail.
#define GCHK(x) do { if ((x) != hipSuccess) { (void)hipGetLastError(); return -2; } } while (0)

constexpr size_t al(size_t v) { return (v + 255) & ~(size_t)255; }          // every part of a staging / scratch buffer starts 256 bytes aligned

// the grow-only buffer in device or pinned host memory (dev_buf.h): buf_grow -> 0 as it is, 1 reallocated, -2 HIP error
using mi355::Buf; using mi355::buf_free; using mi355::buf_grow;
// a device buffer and its pinned mirror, a quarter of slack on both
int grow_pair(Buf& d, Buf& h, size_t need) {
    const int rd = buf_grow(d, need, need + need / 4), rh = buf_grow(h, need, need + need / 4);
    return (rd < 0 || rh < 0) ? -2 : (rd | rh);
}
// the device side of a Lucas-Kanade launch: points in [n][2], points out [n][2], status [n]; room for 1024 points at least
struct PtsBufs {
    Buf pts, next, status;
};
int grow_points(PtsBufs& b, int n) {
    const size_t cap = (size_t)std::max(1024, n);
    return (buf_grow(b.pts, (size_t)n * 8, cap * 8) < 0 || buf_grow(b.next, (size_t)n * 8, cap * 8) < 0 || buf_grow(b.status, (size_t)n, cap) < 0) ? -2 : 0;
}
void free_points(PtsBufs& b) { buf_free(b.pts); buf_free(b.next); buf_free(b.status); }

// buildOpticalFlowPyramid's level geometry: level l + 1 is ((h + 1) / 2) x ((w + 1) / 2) and exists while it is larger than the window in
// both directions (at most max_level levels above the plane, kMaxLevels in all).  off[l]: byte offset of level l in a pyramid whose planes
// start 256 bytes aligned; bytes: the pyramid's size.
struct PyrGeom {
    int levels; int hs[kMaxLevels], ws[kMaxLevels];
    size_t off[kMaxLevels], bytes;
};
PyrGeom pyr_geometry(int h0, int w0, int max_level, int win) {
    PyrGeom q{};
    q.levels = 1; q.hs[0] = h0; q.ws[0] = w0;
    for (int l = 0; l < max_level && q.levels < kMaxLevels; ++l) {
        const int nh = (q.hs[q.levels - 1] + 1) / 2, nw = (q.ws[q.levels - 1] + 1) / 2;
        if (nh <= win || nw <= win) break;
        q.hs[q.levels] = nh; q.ws[q.levels] = nw; ++q.levels;
    }
    for (int l = 0; l < q.levels; ++l) { q.off[l] = q.bytes; q.bytes += al((size_t)q.hs[l] * q.ws[l]); }
    return q;
}
// would the same rule without the kMaxLevels bound (the host routine's) build more planes than a pyramid here holds?
bool pyr_too_deep(int h0, int w0, int max_level, int win) {
    int h = h0, w = w0, planes = 1;
    for (int l = 0; l < max_level && planes <= kMaxLevels; ++l) {
        h = (h + 1) / 2; w = (w + 1) / 2;
        if (h <= win || w <= win) break;
        ++planes;
    }
    return planes > kMaxLevels;
}

// level l - 1 -> level l of `count` pyramids that lie `stride` bytes apart
void enqueue_pyr_down(hipStream_t s, int count, uint8_t* pyr, size_t stride, const PyrGeom& q, int l) {
    const int np = q.hs[l] * q.ws[l];
    hipLaunchKernelGGL(pyr_down_kernel, dim3((np + 255) / 256, count), dim3(256), 0, s, pyr + q.off[l - 1], q.hs[l - 1], q.ws[l - 1], pyr + q.off[l], q.hs[l], q.ws[l],
                       stride);
}

// The frame preparation of `count` frames as one set of launches: the BGR frame at src + f * src_stride becomes level 0 of the pyramid at
// pyr + f * pyr_stride (q: its geometry), its min-eigenvalue map and corner mask go to eig / ok + f * plane, its maximum to max_bits[f] (zeroed
// by the caller); then the pyramid's upper levels.  xtab / ytab: the INTER_LINEAR tables on the device (not read unless `resize`).
void enqueue_prepare(hipStream_t s, int count, const uint8_t* src, size_t src_stride, int H, int W, const int* xtab, const int* ytab, int resize, uint8_t* pyr,
                     size_t pyr_stride, float* eig, uint8_t* ok, unsigned* max_bits, double quality, const PyrGeom& q) {
    const int oh = q.hs[0], ow = q.ws[0];
    const dim3 grid((unsigned)(((size_t)oh * ow + 255) / 256), count);
    hipLaunchKernelGGL(gray_resize_kernel, grid, dim3(256), 0, s, src, H, W, xtab, ytab, pyr, oh, ow, resize, src_stride, pyr_stride);
    hipLaunchKernelGGL(min_eig_kernel, grid, dim3(256), 0, s, pyr, oh, ow, eig, max_bits, pyr_stride);
    hipLaunchKernelGGL(corner_mask_kernel, grid, dim3(256), 0, s, eig, oh, ow, max_bits, quality, ok);
    for (int l = 1; l < q.levels; ++l) enqueue_pyr_down(s, count, pyr, pyr_stride, q, l);
}

// Lucas-Kanade from the pyramid at `prev` into the one at `cur` (both of geometry q): n points -- or, with n_arr, `pairs` frame pairs in ONE
// launch: pair p tracks n_arr[p] <= n points from prev + p * pair_stride into cur + p * pair_stride, its points / results at p * n.
struct LkParams {
    int win, max_iters; double eps, min_eig;
};
void enqueue_lk(hipStream_t s, const PyrGeom& q, const uint8_t* prev, const uint8_t* cur, const LkParams& k, const float* pts, float* next, uint8_t* status, int n,
                int pairs = 1, size_t pair_stride = 0, const int* n_arr = nullptr) {
    LkArgs a{};
    for (int l = 0; l < q.levels; ++l) { a.prev[l] = prev + q.off[l]; a.cur[l] = cur + q.off[l]; a.h[l] = q.hs[l]; a.w[l] = q.ws[l]; }
    a.top = q.levels - 1; a.n = n_arr ? 0 : n; a.win = k.win; a.max_iters = k.max_iters; a.width = q.ws[0]; a.height = q.hs[0];
    a.eps2 = k.eps * k.eps; a.min_eig = k.min_eig;
    a.pts = pts; a.next = next; a.status = status;
    a.pair_stride = pair_stride; a.max_pts = n_arr ? n : 0; a.n_arr = n_arr;
    hipLaunchKernelGGL(lk_kernel, dim3((n + kLkWaves - 1) / kLkWaves, pairs), dim3(64 * kLkWaves), 0, s, a);
}

// "run body(i) for i in 0 .. n - 1 on nthreads threads" (inline when that is one); host_threads: how many a step of n items gets
int host_threads(int n) { return std::max(1, std::min(std::min(8, n), (int)std::thread::hardware_concurrency())); }
template <class F>
void parallel_for(int n, int nthreads, F&& body) {
    if (nthreads <= 1) { for (int i = 0; i < n; ++i) body(i); return; }
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; ++t) th.emplace_back([&, t] { for (int i = t; i < n; i += nthreads) body(i); });
    for (auto& t : th) t.join();
}

// ---- GMC.apply_sparseoptflow (ultralytics/trackers/utils/gmc.py): its parameters, one camera's state, the host half of a step ---------
constexpr int kMaxCorners = 1000, kLkLevels = 3;
constexpr LkParams kLk = {21, 30, 0.01, 1e-4};
constexpr double kQuality = 0.01, kRansacThr = 3.0, kRansacConf = 0.99;
constexpr int kRansacIters = 2000;

// INTER_LINEAR sample table of a dn-long axis resampled from sn: (source index, tap 0, tap 1), 11-bit taps, float32 coordinates as cv2
void linear_table(int dn, int sn, std::vector<int>& tab) {
    tab.resize((size_t)dn * 3);
    const double scale = (double)sn / dn;
    for (int d = 0; d < dn; ++d) {
        float fx = (float)((d + 0.5) * scale - 0.5);
        int s0 = (int)floorf(fx);
        fx -= (float)s0;
        if (s0 < 0) { s0 = 0; fx = 0.f; }
        if (s0 >= sn - 1) { s0 = sn - 1; fx = 0.f; }
        tab[d * 3] = s0;
        tab[d * 3 + 1] = (int)lrintf((1.f - fx) * 2048.f);
        tab[d * 3 + 2] = (int)lrintf(fx * 2048.f);
    }
}

// the (height, width, oh, ow) a pair of resize tables belongs to
bool key_is(const int* k, int H, int W, int oh, int ow) { return k[0] == H && k[1] == W && k[2] == oh && k[3] == ow; }
void key_set(int* k, int H, int W, int oh, int ow) { k[0] = H; k[1] = W; k[2] = oh; k[3] = ow; }

// One camera's state between steps: the previous frame's plane and ordered corners on the host, and -- device objects -- which pyramid slot
// holds that frame and which tables the device has.  mi355_gmc has one, mi355_gmc_multi one per camera.
struct CamState {
    std::vector<int> xt, yt; int tkey[4] = {0, 0, 0, 0};       // INTER_LINEAR tables of (height, width, oh, ow)
    std::vector<float> prev_pts, lk_pts; std::vector<uint8_t> prev_gray;
    int prev_h = 0, prev_w = 0; bool have_prev_pts = false;
    int slot = 0; bool have_prev = false; int ph = 0, pw = 0;  // the slot and plane size of the last prepared frame
    int tab_key[4] = {0, 0, 0, 0};                             // (height, width, oh, ow) the resize tables on the device belong to
};
// make the host tables current for (H, W, oh, ow)
void cam_tables(CamState& c, int H, int W, int oh, int ow) {
    if (key_is(c.tkey, H, W, oh, ow)) return;
    linear_table(ow, W, c.xt); linear_table(oh, H, c.yt);
    key_set(c.tkey, H, W, oh, ow);
}
// does the previous frame precede a frame of plane size oh x ow?  (corners known, same size; on_device: and its pyramid is there)
bool cam_follows(const CamState& c, int oh, int ow, bool on_device) {
    return c.have_prev_pts && c.prev_h == oh && c.prev_w == ow && (!on_device || (c.have_prev && c.ph == oh && c.pw == ow));
}
// What this frame tracks: the previous frame's corners, only into a plane of the same size (GMC.apply resets otherwise) -> lk_pts; returns
// their number.  When there are none the device pyramid is no predecessor either.
int cam_decide(CamState& c, int oh, int ow, bool on_device) {
    const bool lk = cam_follows(c, oh, ow, on_device) && !c.prev_pts.empty();
    c.lk_pts.clear();
    if (lk) c.lk_pts = c.prev_pts; else c.have_prev = false;
    return (int)(c.lk_pts.size() / 2);
}
// this frame (its plane in prev_gray, its corners in prev_pts by now) becomes the previous one
void cam_advance(CamState& c, int oh, int ow) { c.prev_h = oh; c.prev_w = ow; c.have_prev_pts = true; }
// a step's results never arrived: nothing precedes the next frame
void cam_lost(CamState& c) { c.have_prev = false; c.have_prev_pts = false; }
// GMC.reset_params
void cam_forget(CamState& c) {
    cam_lost(c);
    c.prev_pts.clear(); c.prev_gray.clear(); c.prev_h = c.prev_w = 0;
}
// the previous frame as the object holds it (tests): plane size, number of corners; gray_out [oh * ow] and pts_out [pts_cap][2] when given
void cam_report(const CamState& c, int* oh, int* ow, int* n_pts, uint8_t* gray_out, float* pts_out, int pts_cap) {
    const int n = c.have_prev_pts ? (int)(c.prev_pts.size() / 2) : 0;
    if (oh) *oh = c.have_prev_pts ? c.prev_h : 0;
    if (ow) *ow = c.have_prev_pts ? c.prev_w : 0;
    if (n_pts) *n_pts = n;
    if (gray_out && c.have_prev_pts) std::memcpy(gray_out, c.prev_gray.data(), c.prev_gray.size());
    if (pts_out && pts_cap > 0 && n > 0) std::memcpy(pts_out, c.prev_pts.data(), (size_t)std::min(n, pts_cap) * 8);
}

// The host half of a step behind the kernels, in two parts (the batched entry point needs them apart: pair f tracks frame f - 1's corners).
// tail_warp: the partial affine transform prev -> cur from the tracked pairs (RANSAC, seed 0) when more than 4 survive, its translation scaled
// back to frame pixels -- else the identity.  tail_corners: a frame's corners, strongest first, as the next step tracks them.
void tail_warp(const float* lk_pts, const float* next_pts, const uint8_t* status, int n, int downscale, double* H) {
    H[0] = 1; H[1] = 0; H[2] = 0; H[3] = 0; H[4] = 1; H[5] = 0;
    std::vector<double> src, dst;
    for (int i = 0; i < n; ++i)
        if (status[i]) {
            src.push_back(lk_pts[2 * i]); src.push_back(lk_pts[2 * i + 1]);
            dst.push_back(next_pts[2 * i]); dst.push_back(next_pts[2 * i + 1]);
        }
    const int m = (int)(src.size() / 2);
    double E[6];
    if (m > 4 && mi355_gmc_affine_partial(src.data(), dst.data(), m, kRansacThr, kRansacConf, kRansacIters, 0ull, E, nullptr) == 1) {
        std::memcpy(H, E, sizeof(E));
        H[2] *= downscale; H[5] *= downscale;
    }
}
void tail_corners(const float* eig, const uint8_t* ok, int oh, int ow, std::vector<float>& pts) {
    pts.resize((size_t)kMaxCorners * 2);
    const int nc = mi355_gmc_order_corners(eig, ok, oh, ow, kMaxCorners, pts.data());
    pts.resize((size_t)std::max(nc, 0) * 2);
}

// one-shot calls: per-device scratch, grow-only; calls are serialised (the tracker is sequential per video)
struct GmcCtx {
    hipStream_t stream = nullptr;
    Buf planes;                                                // [prev pyramid | cur pyramid]
    PtsBufs lk;
    Buf h_pin{true};                                           // pinned staging: frames + points in, points + status out
    Buf front, h_front{true};                                  // frame preparation: [bgr | gray | eig | ok | tables | max]
};
std::mutex g_mu;
GmcCtx g_ctx[16];
int one_shot_ctx(int device, GmcCtx** out) {
    GCHK(hipSetDevice(device));
    GmcCtx& c = g_ctx[device];
    if (!c.stream) GCHK(hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking));
    *out = &c;
    return 0;
}

}  // namespace

// Same contract as mi355_gmc_pyr_lk (gmc_host.cpp) with the work done on GPU `device`: 0 = ok, -1 = bad argument (win > 21 and a pyramid of
// more than kMaxLevels planes among them), -2 = HIP error.
extern "C" int mi355_gmc_pyr_lk_device(int device, const uint8_t* prev, const uint8_t* cur, int height, int width, const float* pts, int n,
                                       int win, int max_level, int max_iters, double eps, double min_eig, float* next_pts, uint8_t* status) {
    if (!prev || !cur || height <= 0 || width <= 0 || n < 0 || (n > 0 && (!pts || !next_pts || !status)) || win < 3 || !(win & 1) || win > 21 ||
        device < 0 || device >= 16 || max_level < 0)
        return -1;
    // a pyramid the host routine would build deeper than kMaxLevels planes is refused, not tracked from a lower top level
    if (pyr_too_deep(height, width, max_level, win)) return -1;
    if (n == 0) return 0;
    std::lock_guard<std::mutex> lock(g_mu);
    GmcCtx* ctx = nullptr;
    if (one_shot_ctx(device, &ctx)) return -2;
    GmcCtx& c = *ctx;
    const PyrGeom q = pyr_geometry(height, width, max_level, win);
    const size_t frame = (size_t)height * width;
    const size_t pin_need = 2 * frame + (size_t)n * 8 + (size_t)n * 8 + (size_t)n + 64;
    if (buf_grow(c.planes, 2 * q.bytes) < 0 || grow_points(c.lk, n) < 0 || buf_grow(c.h_pin, pin_need) < 0) return -2;
    uint8_t* h_prev = c.h_pin.p; uint8_t* h_cur = h_prev + frame;
    float* h_pts = (float*)(c.h_pin.p + ((2 * frame + 15) & ~(size_t)15));             // 16-byte aligned behind the frames
    float* h_next = h_pts + 2 * (size_t)n;
    uint8_t* h_status = (uint8_t*)(h_next + 2 * (size_t)n);
    std::memcpy(h_prev, prev, frame); std::memcpy(h_cur, cur, frame); std::memcpy(h_pts, pts, (size_t)n * 8);
    uint8_t* dp = c.planes.p; uint8_t* dc = c.planes.p + q.bytes;
    float* d_pts = (float*)c.lk.pts.p; float* d_next = (float*)c.lk.next.p;
    GCHK(hipMemcpyAsync(dp, h_prev, frame, hipMemcpyHostToDevice, c.stream));
    GCHK(hipMemcpyAsync(dc, h_cur, frame, hipMemcpyHostToDevice, c.stream));
    GCHK(hipMemcpyAsync(d_pts, h_pts, (size_t)n * 8, hipMemcpyHostToDevice, c.stream));
    for (int l = 1; l < q.levels; ++l) { enqueue_pyr_down(c.stream, 1, dp, 0, q, l); enqueue_pyr_down(c.stream, 1, dc, 0, q, l); }
    enqueue_lk(c.stream, q, dp, dc, LkParams{win, max_iters, eps, min_eig}, d_pts, d_next, c.lk.status.p, n);
    GCHK(hipGetLastError());
    GCHK(hipMemcpyAsync(h_next, d_next, (size_t)n * 8, hipMemcpyDeviceToHost, c.stream));
    GCHK(hipMemcpyAsync(h_status, c.lk.status.p, (size_t)n, hipMemcpyDeviceToHost, c.stream));
    GCHK(hipStreamSynchronize(c.stream));
    std::memcpy(next_pts, h_next, (size_t)n * 8); std::memcpy(status, h_status, (size_t)n);
    return 0;
}

// Frame preparation of GMC.apply on GPU `device`: BGR frame [height][width][3] -> gray plane of (height / downscale) x (width /
// downscale) (cv2.cvtColor + cv2.resize INTER_LINEAR, bit for bit the fixed-point arithmetic gmc.py states), the float32
// min-eigenvalue map of cornerMinEigenVal and the 0/1 mask of the corners goodFeaturesToTrack keeps before it orders them
// (quality threshold, 3x3 non-maximum suppression, border excluded).  xtab / ytab: per output column / row (source index, tap 0,
// tap 1) as gmc._linear_coeffs gives them; ignored when downscale == 1.  Outputs are host buffers of oh * ow elements.
extern "C" int mi355_gmc_prepare_device(int device, const uint8_t* bgr, int height, int width, int oh, int ow, const int* xtab, const int* ytab,
                                        double quality, uint8_t* gray_out, float* eig_out, uint8_t* ok_out) {
    if (!bgr || height <= 0 || width <= 0 || oh <= 0 || ow <= 0 || !gray_out || !eig_out || !ok_out || device < 0 || device >= 16) return -1;
    const int resize = !(oh == height && ow == width);
    if (resize && (!xtab || !ytab)) return -1;
    std::lock_guard<std::mutex> lock(g_mu);
    GmcCtx* ctx = nullptr;
    if (one_shot_ctx(device, &ctx)) return -2;
    GmcCtx& c = *ctx;
    const size_t nb = (size_t)height * width * 3, np = (size_t)oh * ow;
    const size_t o_gray = al(nb), o_eig = o_gray + al(np), o_ok = o_eig + al(np * 4), o_xt = o_ok + al(np), o_yt = o_xt + al((size_t)ow * 12),
                 o_max = o_yt + al((size_t)oh * 12), total = o_max + 256;
    const size_t h_in = al(nb) + al((size_t)ow * 12) + al((size_t)oh * 12), h_total = h_in + al(np) + al(np * 4) + al(np);
    if (buf_grow(c.front, total) < 0 || buf_grow(c.h_front, h_total) < 0) return -2;
    uint8_t* D = c.front.p; uint8_t* hp = c.h_front.p;
    uint8_t* h_bgr = hp; uint8_t* h_xt = hp + al(nb); uint8_t* h_yt = h_xt + al((size_t)ow * 12);
    uint8_t* h_gray = hp + h_in; uint8_t* h_eig = h_gray + al(np); uint8_t* h_ok = h_eig + al(np * 4);
    std::memcpy(h_bgr, bgr, nb);
    GCHK(hipMemcpyAsync(D, h_bgr, nb, hipMemcpyHostToDevice, c.stream));
    if (resize) {
        std::memcpy(h_xt, xtab, (size_t)ow * 12); std::memcpy(h_yt, ytab, (size_t)oh * 12);
        GCHK(hipMemcpyAsync(D + o_xt, h_xt, (size_t)ow * 12, hipMemcpyHostToDevice, c.stream));
        GCHK(hipMemcpyAsync(D + o_yt, h_yt, (size_t)oh * 12, hipMemcpyHostToDevice, c.stream));
    }
    GCHK(hipMemsetAsync(D + o_max, 0, 4, c.stream));
    // the plane alone: a pyramid of one level
    enqueue_prepare(c.stream, 1, D, 0, height, width, (const int*)(D + o_xt), (const int*)(D + o_yt), resize, D + o_gray, 0, (float*)(D + o_eig), D + o_ok,
                    (unsigned*)(D + o_max), quality, pyr_geometry(oh, ow, 0, 3));
    GCHK(hipGetLastError());
    GCHK(hipMemcpyAsync(h_gray, D + o_gray, np, hipMemcpyDeviceToHost, c.stream));
    GCHK(hipMemcpyAsync(h_eig, D + o_eig, np * 4, hipMemcpyDeviceToHost, c.stream));
    GCHK(hipMemcpyAsync(h_ok, D + o_ok, np, hipMemcpyDeviceToHost, c.stream));
    GCHK(hipStreamSynchronize(c.stream));
    std::memcpy(gray_out, h_gray, np); std::memcpy(eig_out, h_eig, np * 4); std::memcpy(ok_out, h_ok, np);
    return 0;
}

// ---- one motion-compensation step as two calls: enqueue, then collect ------------------------------------------------------------
// model.track() enqueues the step for a frame BEFORE the detector runs on it and collects it when the tracker asks for the warp: the
// frame preparation and the optical flow (0.7 ms for a thousand corners) then run beside the detector pass on a stream of their own
// instead of after it.  The object keeps the previous frame's pyramid on the device (two slots, swapped per step).
struct mi355_gmc {
    int device = 0;
    hipStream_t stream = nullptr;
    Buf d_front;                                               // [bgr | eig | ok | x table | y table | max]
    Buf d_pyr[2];                                              // both of one size; cam.slot holds the last prepared frame's pyramid
    PtsBufs d_lk;
    Buf h_pin{true};
    hipEvent_t ev_up = nullptr; int up_h = 0, up_w = 0;        // recorded behind the pending step's frame upload (mi355_gmc_pending_frame)
    // the pending step
    bool pending = false; int oh = 0, ow = 0, n_lk = 0;
    size_t o_hgray = 0, o_heig = 0, o_hok = 0, o_hnext = 0, o_hstatus = 0;
    // ---- GMC.apply_sparseoptflow's state machine (mi355_gmc_track_*): the previous frame's plane and ordered corners live here, so a
    // step is two calls from the tracker's language binding (enqueue, collect -> 2 x 3 matrix) and nothing per frame is done in it
    bool host = false;                                         // mi355_gmc_create(-1): every stage in host C++ (csrc/gmc_host.cpp)
    int downscale = 2;
    CamState cam;
    std::vector<uint8_t> cur_gray, ok, status; std::vector<float> eig, next_pts;
    bool track_pending = false; int t_oh = 0, t_ow = 0, t_n = 0;
    std::vector<uint8_t> host_frame; int hf_h = 0, hf_w = 0;   // host object: the frame of the pending step
    // collect worker (device objects): the host half of a step -- wait for the stream, order the new corners, RANSAC -- runs on a thread of
    // its own from the moment track_begin has enqueued the step, i.e. beside the detector pass the caller runs next; track_finish joins it
    std::thread worker; std::mutex mu; std::condition_variable cv;
    bool job_ready = false, job_done = false, worker_stop = false; int job_rc = 0; double job_H[6] = {1, 0, 0, 0, 1, 0};
    // mi355_gmc_batch_frames: the frames of the batch a (concurrent) mi355_gmc_track_batch call has uploaded
    hipEvent_t ev_batch_up = nullptr; unsigned long long batch_up_seq = 0; int batch_n = 0, batch_h = 0, batch_w = 0; size_t batch_fstride = 0;
    bool job_active = false;                                   // written by the calling thread only: this step's collect belongs to the worker
    // mi355_gmc_track_batch: device buffers of one batch (grow-only) and their pinned mirror
    Buf d_batch, h_batch{true};
};

namespace {
// Both pyramid slots hold `bytes`: 0 = they did, 1 = reallocated, -2 = HIP error; after the last two no frame on the device precedes the next.
int grow_pyramids(mi355_gmc* g, size_t bytes) {
    const int r0 = buf_grow(g->d_pyr[0], bytes), r1 = buf_grow(g->d_pyr[1], bytes);
    if (r0 || r1) g->cam.have_prev = false;
    return (r0 < 0 || r1 < 0) ? -2 : (r0 | r1);
}
}  // namespace

extern "C" int mi355_gmc_create(int device, mi355_gmc** out) {
    if (!out || device < -1) return -1;
    *out = nullptr;
    if (device >= 0) GCHK(hipSetDevice(device));
    mi355_gmc* g = new mi355_gmc();
    g->device = device; g->host = device == -1;
    *out = g;
    if (g->host) return 0;                                      // host object: no HIP call is ever made through it
    // The step runs BESIDE the detector pass (model.track enqueues it first), on a stream of its own at the default priority.  Measured
    // (tools/track_prio_ab.sh, round 4): giving this stream the LOWEST and the detector's the HIGHEST priority does not speed the detector
    // up (637-644 us per frame either way) and delays the collect (119-139 -> 163-171 us): 805-838 -> 863-893 us per frame.
    // MI355_GMC_PRIO=1 asks for the lowest priority (A/B only).
    int least = 0, greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
    static const bool low_prio = getenv("MI355_GMC_PRIO") && atoi(getenv("MI355_GMC_PRIO")) == 1;
    if (hipStreamCreateWithPriority(&g->stream, hipStreamNonBlocking, low_prio ? least : 0) != hipSuccess) { (void)hipGetLastError(); delete g; *out = nullptr; return -2; }
    return 0;
}

extern "C" void mi355_gmc_destroy(mi355_gmc* g) {
    if (g && g->worker.joinable()) {
        { std::lock_guard<std::mutex> lk(g->mu); g->worker_stop = true; }
        g->cv.notify_all();
        g->worker.join();
    }
    if (!g) return;
    if (g->host) { delete g; return; }
    (void)hipSetDevice(g->device);
    if (g->stream) { (void)hipStreamSynchronize(g->stream); (void)hipStreamDestroy(g->stream); }
    if (g->ev_up) (void)hipEventDestroy(g->ev_up);
    if (g->ev_batch_up) (void)hipEventDestroy(g->ev_batch_up);
    for (Buf* b : {&g->d_front, &g->d_pyr[0], &g->d_pyr[1], &g->h_pin, &g->d_batch, &g->h_batch}) buf_free(*b);
    free_points(g->d_lk);
    delete g;
}

// Enqueue one step: frame preparation of `bgr` (as mi355_gmc_prepare_device) and, when n_prev > 0, Lucas-Kanade tracking of the
// n_prev points `prev_pts` from the PREVIOUS step's plane into this one (as mi355_gmc_pyr_lk_device; the previous step must have
// prepared a plane of the same oh x ow).  Returns at once; nothing of `bgr` / `prev_pts` is read after the call returns.
extern "C" int mi355_gmc_step_begin(mi355_gmc* g, const uint8_t* bgr, int height, int width, int oh, int ow, const int* xtab, const int* ytab,
                                    double quality, const float* prev_pts, int n_prev, int win, int max_level, int max_iters, double eps,
                                    double min_eig) {
    if (g && g->host) return -1;
    if (!g || !bgr || height <= 0 || width <= 0 || oh <= 0 || ow <= 0 || n_prev < 0 || (n_prev > 0 && !prev_pts) || win < 3 || !(win & 1) || win > 21 ||
        max_level < 0)
        return -1;
    const int resize = !(oh == height && ow == width);
    if (resize && (!xtab || !ytab)) return -1;
    if (g->pending) return -1;                                  // collect the previous step first
    CamState& c = g->cam;
    if (n_prev > 0 && !(c.have_prev && c.ph == oh && c.pw == ow)) return -1;
    GCHK(hipSetDevice(g->device));
    const size_t nb = (size_t)height * width * 3, np = (size_t)oh * ow;
    const PyrGeom q = pyr_geometry(oh, ow, max_level, win);    // of the oh x ow plane
    {
        const int r = grow_pyramids(g, q.bytes);
        if (r < 0) return -2;
        if (r && n_prev > 0) return -1;                         // the plane the points were to be tracked from went with the old pyramids
    }
    const size_t o_eig = al(nb), o_ok = o_eig + al(np * 4), o_xt = o_ok + al(np), o_yt = o_xt + al((size_t)ow * 12), o_max = o_yt + al((size_t)oh * 12),
                 total = o_max + 256;
    {
        const int r = buf_grow(g->d_front, total);
        if (r) c.tab_key[0] = 0;                                // the tables went with the old buffer
        if (r < 0) return -2;
    }
    if (grow_points(g->d_lk, n_prev) < 0) return -2;
    // pinned staging: [bgr | x table | y table | prev points] in, [gray | eig | ok | next points | status] out
    const size_t i_xt = al(nb), i_yt = i_xt + al((size_t)ow * 12), i_pts = i_yt + al((size_t)oh * 12), i_end = i_pts + al((size_t)n_prev * 8);
    g->o_hgray = i_end; g->o_heig = g->o_hgray + al(np); g->o_hok = g->o_heig + al(np * 4); g->o_hnext = g->o_hok + al(np);
    g->o_hstatus = g->o_hnext + al((size_t)n_prev * 8);
    if (buf_grow(g->h_pin, g->o_hstatus + al((size_t)n_prev) + 256) < 0) return -2;
    uint8_t* hp = g->h_pin.p; uint8_t* D = g->d_front.p;
    std::memcpy(hp, bgr, nb);
    GCHK(hipMemcpyAsync(D, hp, nb, hipMemcpyHostToDevice, g->stream));
    if (!g->ev_up) GCHK(hipEventCreateWithFlags(&g->ev_up, hipEventDisableTiming));
    GCHK(hipEventRecord(g->ev_up, g->stream)); g->up_h = height; g->up_w = width;
    if (resize && !key_is(c.tab_key, height, width, oh, ow)) {
        std::memcpy(hp + i_xt, xtab, (size_t)ow * 12); std::memcpy(hp + i_yt, ytab, (size_t)oh * 12);
        GCHK(hipMemcpyAsync(D + o_xt, hp + i_xt, (size_t)ow * 12, hipMemcpyHostToDevice, g->stream));
        GCHK(hipMemcpyAsync(D + o_yt, hp + i_yt, (size_t)oh * 12, hipMemcpyHostToDevice, g->stream));
        key_set(c.tab_key, height, width, oh, ow);
    }
    GCHK(hipMemsetAsync(D + o_max, 0, 4, g->stream));
    const int nslot = c.slot ^ 1;
    uint8_t* dc = g->d_pyr[nslot].p;
    uint8_t* dp = g->d_pyr[c.slot].p;
    enqueue_prepare(g->stream, 1, D, 0, height, width, (const int*)(D + o_xt), (const int*)(D + o_yt), resize, dc, 0, (float*)(D + o_eig), D + o_ok,
                    (unsigned*)(D + o_max), quality, q);
    if (n_prev > 0) {
        float* d_pts = (float*)g->d_lk.pts.p; float* d_next = (float*)g->d_lk.next.p;
        std::memcpy(hp + i_pts, prev_pts, (size_t)n_prev * 8);
        GCHK(hipMemcpyAsync(d_pts, hp + i_pts, (size_t)n_prev * 8, hipMemcpyHostToDevice, g->stream));
        enqueue_lk(g->stream, q, dp, dc, LkParams{win, max_iters, eps, min_eig}, d_pts, d_next, g->d_lk.status.p, n_prev);
        GCHK(hipMemcpyAsync(hp + g->o_hnext, d_next, (size_t)n_prev * 8, hipMemcpyDeviceToHost, g->stream));
        GCHK(hipMemcpyAsync(hp + g->o_hstatus, g->d_lk.status.p, (size_t)n_prev, hipMemcpyDeviceToHost, g->stream));
    }
    GCHK(hipGetLastError());
    GCHK(hipMemcpyAsync(hp + g->o_hgray, dc, np, hipMemcpyDeviceToHost, g->stream));
    GCHK(hipMemcpyAsync(hp + g->o_heig, D + o_eig, np * 4, hipMemcpyDeviceToHost, g->stream));
    GCHK(hipMemcpyAsync(hp + g->o_hok, D + o_ok, np, hipMemcpyDeviceToHost, g->stream));
    c.slot = nslot; c.have_prev = true; c.ph = oh; c.pw = ow;
    g->pending = true; g->oh = oh; g->ow = ow; g->n_lk = n_prev;
    return 0;
}

// The frame of the pending step as it sits on the device (dense BGR [height][width][3], uploaded once by mi355_gmc_step_begin): waits -- on
// the host, ~10 us -- until that upload has landed and hands out the pointer, so that the detector pass of the same frame
// (mi355_yolo_infer_device) reads this copy instead of uploading its own.  Besides saving the second upload this is what lets the two
// overlap at all: a second host -> device copy queues up behind the step's device -> host copies, which wait for its Lucas-Kanade launch
// (measured: the detector's first kernel started when the whole step was over, tools/track_timeline.py).  Valid until the next step_begin.
extern "C" int mi355_gmc_pending_frame(mi355_gmc* g, const uint8_t** dev_bgr, int* height, int* width) {
    if (!g || g->host || !(g->pending || g->track_pending) || !g->ev_up || !dev_bgr || !height || !width) return -1;
    GCHK(hipSetDevice(g->device));
    GCHK(hipEventSynchronize(g->ev_up));
    *dev_bgr = g->d_front.p; *height = g->up_h; *width = g->up_w;
    return 0;
}

// Collect the enqueued step: gray / eig / ok of oh * ow elements, next_pts [n_prev][2] and status [n_prev] (untouched when the step
// had n_prev == 0).
extern "C" int mi355_gmc_step_finish(mi355_gmc* g, uint8_t* gray_out, float* eig_out, uint8_t* ok_out, float* next_pts, uint8_t* status) {
    if (!g || g->host || !g->pending || !gray_out || !eig_out || !ok_out || (g->n_lk > 0 && (!next_pts || !status))) return -1;
    GCHK(hipSetDevice(g->device));
    g->pending = false;
    if (hipStreamSynchronize(g->stream) != hipSuccess) { (void)hipGetLastError(); g->cam.have_prev = false; return -2; }
    const size_t np = (size_t)g->oh * g->ow;
    const uint8_t* hp = g->h_pin.p;
    std::memcpy(gray_out, hp + g->o_hgray, np); std::memcpy(eig_out, hp + g->o_heig, np * 4); std::memcpy(ok_out, hp + g->o_hok, np);
    if (g->n_lk > 0) { std::memcpy(next_pts, hp + g->o_hnext, (size_t)g->n_lk * 8); std::memcpy(status, hp + g->o_hstatus, (size_t)g->n_lk); }
    return 0;
}

// ---- the whole step of GMC.apply_sparseoptflow on the object (ultralytics/trackers/utils/gmc.py, reached from /root/reference/model.py:38) ----
// track_begin = enqueue: frame preparation of `bgr` and Lucas-Kanade tracking of the previous frame's corners into it (GPU object: on the
// object's stream, returns at once; host object: the frame is copied and the work happens in track_finish).  track_finish = collect:
// orders the new frame's corners (kept for the next step), estimates the partial affine transform prev -> cur from the tracked pairs
// (RANSAC, seed 0) when more than 4 survive, scales its translation back to frame pixels.  H_out: 6 doubles, row-major 2 x 3; the
// identity on the first frame of a plane size, when the previous frame had no corners, or when too few points were tracked.
static void collect_worker(mi355_gmc* g);
extern "C" int mi355_gmc_track_begin(mi355_gmc* g, const uint8_t* bgr, int height, int width, int downscale) {
    if (!g || !bgr || height <= 0 || width <= 0 || downscale < 1 || g->track_pending) return -1;
    const int oh = downscale > 1 ? height / downscale : height, ow = downscale > 1 ? width / downscale : width;
    if (oh <= 0 || ow <= 0) return -1;
    g->downscale = downscale;
    CamState& c = g->cam;
    if (downscale > 1) cam_tables(c, height, width, oh, ow);
    const int n = cam_decide(c, oh, ow, false);                 // whether the device pyramid fits is step_begin's check
    if (g->host) {
        g->host_frame.assign(bgr, bgr + (size_t)height * width * 3); g->hf_h = height; g->hf_w = width;
    } else {
        const int rc = mi355_gmc_step_begin(g, bgr, height, width, oh, ow, downscale > 1 ? c.xt.data() : nullptr, downscale > 1 ? c.yt.data() : nullptr,
                                            kQuality, n ? c.lk_pts.data() : nullptr, n, kLk.win, kLkLevels, kLk.max_iters, kLk.eps, kLk.min_eig);
        if (rc) return rc;
    }
    g->track_pending = true; g->t_oh = oh; g->t_ow = ow; g->t_n = n;
    static const bool async_collect = !getenv("MI355_GMC_ASYNC") || atoi(getenv("MI355_GMC_ASYNC")) != 0;
    if (!g->host && async_collect) {
        if (!g->worker.joinable()) g->worker = std::thread(collect_worker, g);
        { std::lock_guard<std::mutex> lk(g->mu); g->job_ready = true; g->job_done = false; }
        g->job_active = true;
        g->cv.notify_all();
    }
    return 0;
}

static int track_collect(mi355_gmc* g, double* H_out);
static void collect_worker(mi355_gmc* g) {
    (void)hipSetDevice(g->device);
    std::unique_lock<std::mutex> lk(g->mu);
    for (;;) {
        g->cv.wait(lk, [&] { return g->job_ready || g->worker_stop; });
        if (g->worker_stop) return;
        g->job_ready = false;
        lk.unlock();
        const int rc = track_collect(g, g->job_H);
        lk.lock();
        g->job_rc = rc; g->job_done = true;
        g->cv.notify_all();
    }
}

extern "C" int mi355_gmc_track_finish(mi355_gmc* g, double* H_out) {
    if (!g || !H_out || !g->track_pending) return -1;
    if (g->job_active) {                                        // this step's collect waits, runs or ran on the worker
        std::unique_lock<std::mutex> lk(g->mu);
        g->cv.wait(lk, [&] { return g->job_done; });
        g->job_done = false; g->job_active = false; g->track_pending = false;
        std::memcpy(H_out, g->job_H, sizeof(g->job_H));
        return g->job_rc;
    }
    g->track_pending = false;
    return track_collect(g, H_out);
}

static int track_collect(mi355_gmc* g, double* H_out) {
    CamState& c = g->cam;
    const int oh = g->t_oh, ow = g->t_ow, n = g->t_n;
    const size_t np = (size_t)oh * ow;
    g->cur_gray.resize(np); g->eig.resize(np); g->ok.resize(np);
    g->next_pts.assign((size_t)n * 2, 0.f); g->status.assign((size_t)n, 0);
    if (g->host) {
        int rc = mi355_gmc_prepare_host(g->host_frame.data(), g->hf_h, g->hf_w, oh, ow, g->downscale > 1 ? c.xt.data() : nullptr,
                                        g->downscale > 1 ? c.yt.data() : nullptr, kQuality, g->cur_gray.data(), g->eig.data(), g->ok.data());
        if (rc) return rc;
        if (n > 0) {
            rc = mi355_gmc_pyr_lk(c.prev_gray.data(), g->cur_gray.data(), oh, ow, c.lk_pts.data(), n, kLk.win, kLkLevels, kLk.max_iters, kLk.eps, kLk.min_eig,
                                  g->next_pts.data(), g->status.data());
            if (rc) return rc;
        }
    } else {
        const int rc = mi355_gmc_step_finish(g, g->cur_gray.data(), g->eig.data(), g->ok.data(), n ? g->next_pts.data() : nullptr, n ? g->status.data() : nullptr);
        if (rc) { c.have_prev_pts = false; return rc; }
    }
    tail_warp(c.lk_pts.data(), g->next_pts.data(), g->status.data(), n, g->downscale, H_out);
    tail_corners(g->eig.data(), g->ok.data(), oh, ow, c.prev_pts);
    c.prev_gray.swap(g->cur_gray);
    cam_advance(c, oh, ow);
    return 0;
}

// n consecutive frames of one video in ONE call (a batched sweep holds the frames of a detector batch before the tracker needs their
// warps): the frame preparation of all n frames as one set of launches, the corner ordering of the n planes on host threads, the
// Lucas-Kanade tracking of all n frame pairs as ONE launch (n x <= 1000 wavefronts instead of n dependent launches of <= 1000), RANSAC
// per pair on host threads.  Same kernels, same arithmetic and the same state transitions as n track_begin / track_finish steps --
// H_out [n][6] equals theirs bit for bit -- at a fraction of the latency: a step's kernels are latency-bound (148 us for 1000 corners
// whatever the chip could do beside them).  Continues from / leaves behind the object's previous frame.  frames: n pointers to BGR
// frames of height x width.  Host objects run the n steps one after the other.
extern "C" int mi355_gmc_track_batch(mi355_gmc* g, const uint8_t* const* frames, int n, int height, int width, int downscale, double* H_out) {
    if (!g || !frames || n <= 0 || height <= 0 || width <= 0 || downscale < 1 || !H_out || g->track_pending) return -1;
    for (int f = 0; f < n; ++f) if (!frames[f]) return -1;
    if (g->host) {
        for (int f = 0; f < n; ++f) {
            int rc = mi355_gmc_track_begin(g, frames[f], height, width, downscale); if (rc) return rc;
            rc = mi355_gmc_track_finish(g, H_out + 6 * f); if (rc) return rc;
        }
        return 0;
    }
    const int oh = downscale > 1 ? height / downscale : height, ow = downscale > 1 ? width / downscale : width;
    if (oh <= 0 || ow <= 0) return -1;
    GCHK(hipSetDevice(g->device));
    g->downscale = downscale;
    CamState& c = g->cam;
    const int resize = downscale > 1;
    if (resize) cam_tables(c, height, width, oh, ow);
    const size_t nb = (size_t)height * width * 3, np = (size_t)oh * ow;
    const PyrGeom q = pyr_geometry(oh, ow, kLkLevels, kLk.win);
    // does the object's previous frame precede frames[0]?  (same plane size, corners known, its pyramid on the device)
    const bool cont = cam_follows(c, oh, ow, true) && g->d_pyr[1].cap >= q.bytes;
    // device: [frames n x nb | pyramids (n + 1) x q.bytes | eig n x np x 4 | ok n x np | x table | y table | max n x 4 | pts n x kMaxCorners x 8 |
    //          next (same) | status n x kMaxCorners | counts n x 4]
    const size_t fstride = (nb % 16 == 0) ? nb : al(nb);       // dense frames when 16-byte aligned: the detector may read them in place (mi355_gmc_batch_frames)
    const size_t o_pyr = al((size_t)n * fstride), o_eig = o_pyr + (size_t)(n + 1) * q.bytes, o_ok = o_eig + al((size_t)n * np * 4), o_xt = o_ok + al((size_t)n * np),
                 o_yt = o_xt + al((size_t)ow * 12), o_max = o_yt + al((size_t)oh * 12), o_pts = o_max + al((size_t)n * 4),
                 o_next = o_pts + al((size_t)n * kMaxCorners * 8), o_st = o_next + al((size_t)n * kMaxCorners * 8), o_cnt = o_st + al((size_t)n * kMaxCorners),
                 d_total = o_cnt + al((size_t)n * 4);
    // pinned: [frames | tables | eig | ok | pts | next | status | counts | last gray]
    const size_t p_xt = al((size_t)n * fstride), p_yt = p_xt + al((size_t)ow * 12), p_eig = p_yt + al((size_t)oh * 12), p_ok = p_eig + al((size_t)n * np * 4),
                 p_pts = p_ok + al((size_t)n * np), p_next = p_pts + al((size_t)n * kMaxCorners * 8), p_st = p_next + al((size_t)n * kMaxCorners * 8),
                 p_cnt = p_st + al((size_t)n * kMaxCorners), p_gray = p_cnt + al((size_t)n * 4), h_total = p_gray + al(np);
    if (buf_grow(g->d_batch, d_total) < 0 || buf_grow(g->h_batch, h_total) < 0) return -2;
    uint8_t* D = g->d_batch.p; uint8_t* P = g->h_batch.p;
    const int nthreads = host_threads(n);
    // frames -> pinned staging on a few threads (64 frames of 320 x 240 are 14.7 MB: 2.5 ms on one core, a third of this call)
    parallel_for(n, (size_t)n * nb < (1u << 20) ? 1 : nthreads, [&](int f) { std::memcpy(P + (size_t)f * fstride, frames[f], nb); });
    GCHK(hipMemcpyAsync(D, P, (size_t)n * fstride, hipMemcpyHostToDevice, g->stream));
    if (!g->ev_batch_up) GCHK(hipEventCreateWithFlags(&g->ev_batch_up, hipEventDisableTiming));
    GCHK(hipEventRecord(g->ev_batch_up, g->stream));
    { std::lock_guard<std::mutex> lk(g->mu); g->batch_n = n; g->batch_h = height; g->batch_w = width; g->batch_fstride = fstride; ++g->batch_up_seq; }
    g->cv.notify_all();
    if (resize) {
        std::memcpy(P + p_xt, c.xt.data(), (size_t)ow * 12); std::memcpy(P + p_yt, c.yt.data(), (size_t)oh * 12);
        GCHK(hipMemcpyAsync(D + o_xt, P + p_xt, (size_t)ow * 12, hipMemcpyHostToDevice, g->stream));
        GCHK(hipMemcpyAsync(D + o_yt, P + p_yt, (size_t)oh * 12, hipMemcpyHostToDevice, g->stream));
    }
    GCHK(hipMemsetAsync(D + o_max, 0, (size_t)n * 4, g->stream));
    if (cont) GCHK(hipMemcpyAsync(D + o_pyr, g->d_pyr[c.slot].p, q.bytes, hipMemcpyDeviceToDevice, g->stream));   // slot 0 = the previous frame's pyramid
    uint8_t* pyr1 = D + o_pyr + q.bytes;                       // frame f's pyramid at pyr1 + f * q.bytes
    enqueue_prepare(g->stream, n, D, fstride, height, width, (const int*)(D + o_xt), (const int*)(D + o_yt), resize, pyr1, q.bytes, (float*)(D + o_eig), D + o_ok,
                    (unsigned*)(D + o_max), kQuality, q);
    GCHK(hipGetLastError());
    GCHK(hipMemcpyAsync(P + p_eig, D + o_eig, (size_t)n * np * 4, hipMemcpyDeviceToHost, g->stream));
    GCHK(hipMemcpyAsync(P + p_ok, D + o_ok, (size_t)n * np, hipMemcpyDeviceToHost, g->stream));
    GCHK(hipMemcpyAsync(P + p_gray, pyr1 + (size_t)(n - 1) * q.bytes, np, hipMemcpyDeviceToHost, g->stream));
    if (hipStreamSynchronize(g->stream) != hipSuccess) { (void)hipGetLastError(); cam_lost(c); return -2; }
    // corners of every frame, strongest first (host threads); pair f tracks the corners of frame f - 1 (f = 0: the object's previous frame)
    std::vector<std::vector<float>> corners(n);
    parallel_for(n, nthreads, [&](int f) { tail_corners((const float*)(P + p_eig) + (size_t)f * np, P + p_ok + (size_t)f * np, oh, ow, corners[f]); });
    int* cnt = (int*)(P + p_cnt);
    float* hp = (float*)(P + p_pts);
    int any = 0;
    for (int f = 0; f < n; ++f) {
        const std::vector<float>* src = f == 0 ? (cont && !c.prev_pts.empty() ? &c.prev_pts : nullptr) : &corners[f - 1];
        cnt[f] = src ? (int)(src->size() / 2) : 0;
        if (cnt[f]) std::memcpy(hp + (size_t)f * kMaxCorners * 2, src->data(), src->size() * sizeof(float));
        any |= cnt[f];
    }
    if (any) {
        GCHK(hipMemcpyAsync(D + o_pts, P + p_pts, (size_t)n * kMaxCorners * 8, hipMemcpyHostToDevice, g->stream));
        GCHK(hipMemcpyAsync(D + o_cnt, P + p_cnt, (size_t)n * 4, hipMemcpyHostToDevice, g->stream));
        enqueue_lk(g->stream, q, D + o_pyr, pyr1, kLk, (const float*)(D + o_pts), (float*)(D + o_next), D + o_st, kMaxCorners, n, q.bytes, (const int*)(D + o_cnt));
        GCHK(hipGetLastError());
        GCHK(hipMemcpyAsync(P + p_next, D + o_next, (size_t)n * kMaxCorners * 8, hipMemcpyDeviceToHost, g->stream));
        GCHK(hipMemcpyAsync(P + p_st, D + o_st, (size_t)n * kMaxCorners, hipMemcpyDeviceToHost, g->stream));
    }
    // the last frame's pyramid becomes the object's previous one (the per-frame entry points continue from it)
    if (grow_pyramids(g, q.bytes) < 0) return -2;
    GCHK(hipMemcpyAsync(g->d_pyr[c.slot].p, pyr1 + (size_t)(n - 1) * q.bytes, q.bytes, hipMemcpyDeviceToDevice, g->stream));
    if (hipStreamSynchronize(g->stream) != hipSuccess) { (void)hipGetLastError(); cam_lost(c); return -2; }
    c.have_prev = true; c.ph = oh; c.pw = ow;
    const float* hn = (const float*)(P + p_next);
    const uint8_t* hst = P + p_st;
    parallel_for(n, nthreads, [&](int f) {
        tail_warp(hp + (size_t)f * kMaxCorners * 2, hn + (size_t)f * kMaxCorners * 2, hst + (size_t)f * kMaxCorners, cnt[f], downscale, H_out + 6 * f);
    });
    c.prev_pts = corners[n - 1];
    c.prev_gray.assign(P + p_gray, P + p_gray + np);
    cam_advance(c, oh, ow);
    return 0;
}

// The frames of the batch that a mi355_gmc_track_batch call -- running on ANOTHER thread, or already returned -- has uploaded: blocks until that
// call has issued its upload (at most timeout_ms) and the upload has landed, then hands out the device pointer (frame f at dev + f * stride).
// The detector pass of the same batch reads them in place (mi355_yolo_infer_device when stride == height * width * 3): one staging copy and one
// upload per batch instead of two of each.  Each upload is handed out once; valid until the next mi355_gmc_track_batch call on the object.
// after_seq: the value of mi355_gmc_batch_seq taken BEFORE that call was started (uploads are numbered; an older one is never handed out).
// Returns 0, 1 on timeout / nothing new, -1 on bad arguments, -2 on a HIP error.
extern "C" int mi355_gmc_batch_frames(mi355_gmc* g, unsigned long long after_seq, int timeout_ms, const uint8_t** dev, int* n, int* height, int* width,
                                      long long* stride) {
    if (!g || g->host || !dev || !n || !height || !width || !stride) return -1;
    {
        std::unique_lock<std::mutex> lk(g->mu);
        if (!g->cv.wait_for(lk, std::chrono::milliseconds(timeout_ms < 0 ? 0 : timeout_ms), [&] { return g->batch_up_seq > after_seq; })) return 1;
        *n = g->batch_n; *height = g->batch_h; *width = g->batch_w; *stride = (long long)g->batch_fstride;
    }
    GCHK(hipSetDevice(g->device));
    GCHK(hipEventSynchronize(g->ev_batch_up));
    *dev = g->d_batch.p;
    return 0;
}

extern "C" unsigned long long mi355_gmc_batch_seq(mi355_gmc* g) {
    if (!g) return 0;
    std::lock_guard<std::mutex> lk(g->mu);
    return g->batch_up_seq;
}

// Forget the previous frame (GMC.reset_params); a pending step is collected and dropped.
extern "C" int mi355_gmc_track_reset(mi355_gmc* g) {
    if (!g) return -1;
    if (g->track_pending) { double H[6]; (void)mi355_gmc_track_finish(g, H); }
    cam_forget(g->cam);
    return 0;
}

// The previous frame as the object holds it (tests): plane size, number of corners; gray_out [oh * ow] and pts_out [pts_cap][2] when given.
extern "C" int mi355_gmc_track_state(const mi355_gmc* g, int* oh, int* ow, int* n_pts, uint8_t* gray_out, float* pts_out, int pts_cap) {
    if (!g) return -1;
    cam_report(g->cam, oh, ow, n_pts, gray_out, pts_out, pts_cap);
    return 0;
}

// ---- several cameras, one step per tick: mi355_gmc_multi -------------------------------------------------------------------------------
// A store has N cameras of different resolutions and every tick brings one frame of each (or of some).  N mi355_gmc objects cost N streams,
// N worker threads and N sets of small launches; here the tick is ONE launch per stage (per pyramid level), whatever the frames' sizes: the
// kernels read a device array of per-camera descriptors (GmcCam) and a host-built prefix table that maps a block to (camera, block of that
// camera's plane).  The arithmetic per pixel / per point is the *_px / lk_point functions above -- the bits of N single objects.
namespace {

struct GmcCam {
    const uint8_t* src; int H, W, row_stride, resize;       // the tick's frame on the device (dense BGR)
    int oh, ow;                                              // plane size
    unsigned long long xtab, ytab;                           // arena offsets of the INTER_LINEAR tables
    unsigned long long prev, cur;                            // arena offsets of the previous / this frame's pyramid; level l at + lvl[l]
    unsigned lvl[kMaxLevels]; int h[kMaxLevels], w[kMaxLevels]; int top;
    unsigned long long gray, eig, ok;                        // tick-output offsets: copy of the plane, min-eigenvalue map, corner mask
    int max_idx;                                             // its word among the tick's maxima
    int n_pts; unsigned long long pts, next, status;         // points tracked from `prev` (tick-input offset), results (tick-output offsets)
};
static_assert(sizeof(GmcCam) % 8 == 0, "descriptor array stride");

// prefix tables behind the descriptors, (n + 1) ints each: blocks of the plane kernels, of lk, of pyrDown into level 1 .. kMaxLevels - 1
constexpr int kPrefixPlane = 0, kPrefixLk = 1, kPrefixLevel1 = 2, kPrefixTables = 2 + (kMaxLevels - 1);
constexpr int prefix_level(int l) { return kPrefixLevel1 + (l - 1); }          // l = 1 .. kMaxLevels - 1

struct MultiArgs {
    const GmcCam* cams; const int* prefix;                   // this launch's prefix table
    int n;                                                   // cameras in the array
    uint8_t* arena; const uint8_t* tin; uint8_t* tout;
};

// this block's camera and its block number inside that camera's work; false = nothing to do.  Block-uniform: the table sits in scalar registers.
// (A grid with one row per camera, as wide as the largest camera needs, was measured against this lookup and dropped: DESIGN 3.6b.)
__device__ __forceinline__ bool locate(const MultiArgs& m, int& cam, int& b) {
    const int g = blockIdx.x;
    int lo = 0, hi = m.n;                                    // largest cam with prefix[cam] <= g (g < prefix[n] by the grid size)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (m.prefix[mid] <= g) lo = mid; else hi = mid;
    }
    cam = __builtin_amdgcn_readfirstlane(lo); b = g - m.prefix[cam];
    return b < m.prefix[cam + 1] - m.prefix[cam];
}

__global__ __launch_bounds__(256) void gray_resize_multi_kernel(MultiArgs m) {
    int cam, b;
    if (!locate(m, cam, b)) return;
    const GmcCam& c = m.cams[cam];
    const int idx = b * 256 + threadIdx.x;
    if (idx >= c.oh * c.ow) return;
    const uint8_t v = gray_resize_px(c.src, c.H, c.W, (size_t)c.row_stride, (const int*)(m.arena + c.xtab), (const int*)(m.arena + c.ytab), c.ow, c.resize, idx);
    (m.arena + c.cur)[idx] = v;                              // level 0 of this frame's pyramid
    (m.tout + c.gray)[idx] = v;                              // ... and the copy that goes back to the host with the tick's results
}

__global__ __launch_bounds__(256) void min_eig_multi_kernel(MultiArgs m) {
    int cam, b;
    if (!locate(m, cam, b)) return;
    const GmcCam& c = m.cams[cam];
    const int idx = b * 256 + threadIdx.x;
    float e = 0.f;
    if (idx < c.oh * c.ow) {
        e = min_eig_px(m.arena + c.cur, c.oh, c.ow, idx);
        ((float*)(m.tout + c.eig))[idx] = e;
    }
    block_max_to(e, (unsigned*)m.tout + c.max_idx);
}

__global__ __launch_bounds__(256) void corner_mask_multi_kernel(MultiArgs m, double quality) {
    int cam, b;
    if (!locate(m, cam, b)) return;
    const GmcCam& c = m.cams[cam];
    const int idx = b * 256 + threadIdx.x;
    if (idx >= c.oh * c.ow) return;
    (m.tout + c.ok)[idx] = corner_mask_px((const float*)(m.tout + c.eig), c.oh, c.ow, __uint_as_float(((const unsigned*)m.tout)[c.max_idx]), quality, idx);
}

__global__ __launch_bounds__(256) void pyr_down_multi_kernel(MultiArgs m, int l) {          // level l - 1 -> level l of every camera that has one
    int cam, b;
    if (!locate(m, cam, b)) return;
    const GmcCam& c = m.cams[cam];
    const int idx = b * 256 + threadIdx.x;
    if (l > c.top || idx >= c.h[l] * c.w[l]) return;
    uint8_t* pyr = m.arena + c.cur;
    (pyr + c.lvl[l])[idx] = pyr_down_px(pyr + c.lvl[l - 1], c.h[l - 1], c.w[l - 1], c.w[l], idx);
}

struct LkCamView {
    const GmcCam* c; const uint8_t* arena;
    int top, win, max_iters, width, height;
    double eps2, min_eig;
    const float* pts; float* next; uint8_t* status;
    __device__ __forceinline__ const uint8_t* prev_at(int l) const { return arena + c->prev + c->lvl[l]; }
    __device__ __forceinline__ const uint8_t* cur_at(int l) const { return arena + c->cur + c->lvl[l]; }
    __device__ __forceinline__ int h_at(int l) const { return c->h[l]; }
    __device__ __forceinline__ int w_at(int l) const { return c->w[l]; }
};

__global__ __launch_bounds__(64 * kLkWaves) void lk_multi_kernel(MultiArgs m, int win, int max_iters, double eps2, double min_eig) {
    __shared__ uint8_t region[kLkWaves][(kRegMax * kRegMax + 15) & ~15];
    __shared__ LkScratch scratch[kLkWaves];
    int cam, b;
    if (!locate(m, cam, b)) return;
    const GmcCam& c = m.cams[cam];
    const int lane = threadIdx.x & 63;
    const int i = b * kLkWaves + (threadIdx.x >> 6);
    if (i >= c.n_pts) return;
    LkCamView a;
    a.c = &c; a.arena = m.arena; a.top = c.top; a.win = win; a.max_iters = max_iters; a.width = c.ow; a.height = c.oh; a.eps2 = eps2; a.min_eig = min_eig;
    a.pts = (const float*)(m.tin + c.pts); a.next = (float*)(m.tout + c.next); a.status = m.tout + c.status;
    lk_point(a, i, lane, region[threadIdx.x >> 6], scratch[threadIdx.x >> 6]);
}

struct MultiCam {
    CamState s;                                              // GMC.apply_sparseoptflow's state of this camera (as mi355_gmc holds it for one)
    // its region of the arena: [pyramid slot 0 | pyramid slot 1 | x table | y table]
    size_t region = 0, region_cap = 0, pyr_bytes = 0;
    // the pending tick
    bool active = false; int H = 0, W = 0, oh = 0, ow = 0, n = 0;
    size_t t_frame = 0, t_pts = 0, o_gray = 0, o_eig = 0, o_ok = 0, o_next = 0, o_status = 0;
    double Hm[6] = {1, 0, 0, 0, 1, 0}; int rc = 0;
};

}  // namespace

struct mi355_gmc_multi {
    int device = -1, n = 0; bool host = false;
    std::vector<mi355_gmc*> single;                           // host object: one host mi355_gmc per camera
    std::vector<MultiCam> cams;
    hipStream_t stream = nullptr; hipEvent_t ev_up = nullptr, ev_done = nullptr;
    Buf arena; size_t arena_used = 0;
    Buf d_tin, h_tin{true};                                   // the tick's frames + points (pinned mirror): ONE upload
    Buf d_tout, h_tout{true};                                 // maxima + per camera gray / eig / ok / next / status: ONE download
    Buf d_desc, h_desc{true}; size_t desc_bytes = 0;
    std::vector<int> active;                                  // cameras of the pending tick, in camera order
    std::vector<std::thread> workers;
    bool job_active = false;                                  // written by the calling thread only: a tick has been begun and not collected
    int downscale = 2;
};

extern "C" int mi355_gmc_multi_create(int device, int n_cameras, mi355_gmc_multi** out) {
    if (!out || device < -1 || n_cameras <= 0 || n_cameras > 4096) return -1;
    *out = nullptr;
    mi355_gmc_multi* g = new mi355_gmc_multi();
    g->device = device; g->n = n_cameras; g->host = device == -1;
    g->cams.resize((size_t)n_cameras);
    if (g->host) {
        g->single.assign((size_t)n_cameras, nullptr);
        for (int i = 0; i < n_cameras; ++i) if (mi355_gmc_create(-1, &g->single[i])) { mi355_gmc_multi_destroy(g); return -1; }
        *out = g;
        return 0;
    }
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&g->ev_up, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&g->ev_done, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError(); mi355_gmc_multi_destroy(g); return -2;
    }
    *out = g;
    return 0;
}

extern "C" void mi355_gmc_multi_destroy(mi355_gmc_multi* g) {
    if (!g) return;
    for (auto& t : g->workers) if (t.joinable()) t.join();
    for (mi355_gmc* s : g->single) if (s) mi355_gmc_destroy(s);
    if (!g->host) {
        (void)hipSetDevice(g->device);
        if (g->stream) { (void)hipStreamSynchronize(g->stream); (void)hipStreamDestroy(g->stream); }
        if (g->ev_up) (void)hipEventDestroy(g->ev_up);
        if (g->ev_done) (void)hipEventDestroy(g->ev_done);
        for (Buf* b : {&g->arena, &g->d_tin, &g->h_tin, &g->d_tout, &g->h_tout, &g->d_desc, &g->h_desc}) buf_free(*b);
    }
    delete g;
}

namespace {
// the host half of camera ci's step, on a worker: wait for the tick's results, then the warp and the corners
void multi_collect(mi355_gmc_multi* g, int ci) {
    MultiCam& c = g->cams[ci];
    if (g->host) { c.rc = mi355_gmc_track_finish(g->single[ci], c.Hm); return; }
    if (hipEventSynchronize(g->ev_done) != hipSuccess) { (void)hipGetLastError(); c.rc = -2; cam_lost(c.s); return; }
    const uint8_t* P = g->h_tout.p;
    tail_warp(c.s.lk_pts.data(), (const float*)(P + c.o_next), P + c.o_status, c.n, g->downscale, c.Hm);
    tail_corners((const float*)(P + c.o_eig), P + c.o_ok, c.oh, c.ow, c.s.prev_pts);
    c.s.prev_gray.assign(P + c.o_gray, P + c.o_gray + (size_t)c.oh * c.ow);
    cam_advance(c.s, c.oh, c.ow);
    c.rc = 0;
}

// the workers outlive the call that starts them: mi355_gmc_multi_finish joins them
void multi_start_workers(mi355_gmc_multi* g) {
    const int na = (int)g->active.size(), nt = host_threads(na);
    g->workers.clear();
    for (int t = 0; t < nt; ++t)
        g->workers.emplace_back([g, t, nt, na] {
            if (!g->host) (void)hipSetDevice(g->device);
            for (int k = t; k < na; k += nt) multi_collect(g, g->active[k]);
        });
    g->job_active = true;
}

int multi_begin_device(mi355_gmc_multi* g, const uint8_t* const* frames, const int* heights, const int* widths, int downscale) {
    GCHK(hipSetDevice(g->device));
    const int na = (int)g->active.size();
    const int resize = downscale > 1;
    // per camera: plane and pyramid geometry, its region of the arena, what it tracks
    size_t t_total = 0, o_total = al((size_t)na * 4);
    std::vector<GmcCam> desc((size_t)na);
    std::vector<int> prefix((size_t)kPrefixTables * (na + 1), 0);
    int max_top = 0;
    size_t new_bytes = 0;
    std::vector<int> placed;                                    // cameras given a new region this tick: theirs only once the arena holds it
    for (int k = 0; k < na; ++k) {
        const int ci = g->active[k];
        MultiCam& c = g->cams[ci];
        c.H = heights[ci]; c.W = widths[ci];
        c.oh = resize ? c.H / downscale : c.H; c.ow = resize ? c.W / downscale : c.W;
        if (resize) cam_tables(c.s, c.H, c.W, c.oh, c.ow);
        c.n = cam_decide(c.s, c.oh, c.ow, true);
        GmcCam& d = desc[k];
        std::memset(&d, 0, sizeof(d));
        const PyrGeom q = pyr_geometry(c.oh, c.ow, kLkLevels, kLk.win);
        for (int l = 0; l < q.levels; ++l) { d.h[l] = q.hs[l]; d.w[l] = q.ws[l]; d.lvl[l] = (unsigned)q.off[l]; }
        d.top = q.levels - 1; max_top = std::max(max_top, d.top);
        const size_t need = 2 * q.bytes + al((size_t)c.ow * 12) + al((size_t)c.oh * 12);
        bool moved = c.pyr_bytes != q.bytes;
        if (c.region_cap < need) {                              // a larger plane than this camera ever had: a new region at the arena's end
            c.region = al(g->arena_used + new_bytes); new_bytes = c.region + need - g->arena_used; c.region_cap = need;
            placed.push_back(ci);
            moved = true;
        }
        if (moved) { c.pyr_bytes = q.bytes; c.s.have_prev = false; c.s.tab_key[0] = 0; c.n = 0; c.s.lk_pts.clear(); }     // neither pyramid nor tables are where they were
        d.H = c.H; d.W = c.W; d.row_stride = c.W * 3; d.resize = resize; d.oh = c.oh; d.ow = c.ow;
        d.xtab = c.region + 2 * q.bytes; d.ytab = d.xtab + al((size_t)c.ow * 12);
        d.prev = c.region + (size_t)c.s.slot * q.bytes; d.cur = c.region + (size_t)(c.s.slot ^ 1) * q.bytes;
        d.n_pts = c.n; d.max_idx = k;
        const size_t np = (size_t)c.oh * c.ow;
        c.t_frame = t_total; t_total += al((size_t)c.H * c.W * 3);                  // frame starts 256-byte aligned: the detector reads them in place
        c.o_gray = o_total; o_total += al(np);
        c.o_eig = o_total; o_total += al(np * 4);
        c.o_ok = o_total; o_total += al(np);
        c.o_next = o_total; o_total += al((size_t)c.n * 8);
        c.o_status = o_total; o_total += al((size_t)c.n);
        d.gray = c.o_gray; d.eig = c.o_eig; d.ok = c.o_ok; d.next = c.o_next; d.status = c.o_status;
    }
    const size_t t_frames_end = t_total;
    for (int k = 0; k < na; ++k) { MultiCam& c = g->cams[g->active[k]]; c.t_pts = t_total; desc[k].pts = c.t_pts; t_total += al((size_t)c.n * 8); }
    std::vector<size_t> t_tab((size_t)na, 0);                   // resize tables that have to go up, staged behind the points
    for (int k = 0; k < na; ++k) {
        MultiCam& c = g->cams[g->active[k]];
        if (resize && !key_is(c.s.tab_key, c.H, c.W, c.oh, c.ow)) { t_tab[k] = t_total; t_total += al((size_t)c.ow * 12) + al((size_t)c.oh * 12); }
    }
    if (new_bytes) {
        const size_t need = g->arena_used + new_bytes;
        if (g->arena.cap < need) {                              // grow-only: the cameras' previous pyramids move with it
            Buf a;
            auto unplace = [&] { for (int ci : placed) g->cams[ci].region = g->cams[ci].region_cap = 0; };
            if (buf_grow(a, need, std::max(need + need / 2, (size_t)1 << 20)) < 0) { unplace(); return -2; }
            if (g->arena.p && g->arena_used) {
                if (hipMemcpyAsync(a.p, g->arena.p, g->arena_used, hipMemcpyDeviceToDevice, g->stream) != hipSuccess || hipStreamSynchronize(g->stream) != hipSuccess) {
                    (void)hipGetLastError(); buf_free(a); unplace(); return -2;
                }
            }
            buf_free(g->arena);
            g->arena = a;
        }
        g->arena_used = need;
    }
    if (grow_pair(g->d_tin, g->h_tin, t_total) < 0 || grow_pair(g->d_tout, g->h_tout, o_total) < 0) return -2;
    // descriptors (+ prefix tables): one image, uploaded only when its bytes differ from what the device holds
    for (int k = 0; k < na; ++k) {
        const MultiCam& c = g->cams[g->active[k]];
        const GmcCam& d = desc[k];
        desc[k].src = g->d_tin.p + c.t_frame;
        int* p = prefix.data();
        p[kPrefixPlane * (na + 1) + k + 1] = p[kPrefixPlane * (na + 1) + k] + (int)(((size_t)c.oh * c.ow + 255) / 256);
        for (int l = 1; l < kMaxLevels; ++l)
            p[prefix_level(l) * (na + 1) + k + 1] = p[prefix_level(l) * (na + 1) + k] + (l <= d.top ? (d.h[l] * d.w[l] + 255) / 256 : 0);
        p[kPrefixLk * (na + 1) + k + 1] = p[kPrefixLk * (na + 1) + k] + (c.n + kLkWaves - 1) / kLkWaves;
    }
    const size_t desc_b = al((size_t)na * sizeof(GmcCam)), bytes = desc_b + al(prefix.size() * 4);
    {
        const int r = grow_pair(g->d_desc, g->h_desc, bytes);
        if (r) g->desc_bytes = 0;                               // the device holds no image any more
        if (r < 0) return -2;
    }
    std::vector<char> img(bytes, 0);
    std::memcpy(img.data(), desc.data(), (size_t)na * sizeof(GmcCam));
    std::memcpy(img.data() + desc_b, prefix.data(), prefix.size() * 4);
    // stage the frames (a few threads when they are large) and the points, then ONE upload
    uint8_t* P = g->h_tin.p;
    parallel_for(na, t_frames_end < ((size_t)1 << 20) ? 1 : host_threads(na), [&](int k) {
        const int ci = g->active[k]; const MultiCam& c = g->cams[ci];
        std::memcpy(P + c.t_frame, frames[ci], (size_t)c.H * c.W * 3);
    });
    for (int k = 0; k < na; ++k) {
        const MultiCam& c = g->cams[g->active[k]];
        if (c.n) std::memcpy(P + c.t_pts, c.s.lk_pts.data(), (size_t)c.n * 8);
        if (t_tab[k]) { std::memcpy(P + t_tab[k], c.s.xt.data(), (size_t)c.ow * 12); std::memcpy(P + t_tab[k] + al((size_t)c.ow * 12), c.s.yt.data(), (size_t)c.oh * 12); }
    }
    GCHK(hipMemcpyAsync(g->d_tin.p, P, t_total, hipMemcpyHostToDevice, g->stream));
    GCHK(hipEventRecord(g->ev_up, g->stream));
    for (int k = 0; k < na; ++k) {
        MultiCam& c = g->cams[g->active[k]];
        if (!t_tab[k]) continue;
        GCHK(hipMemcpyAsync(g->arena.p + desc[k].xtab, g->d_tin.p + t_tab[k], (size_t)c.ow * 12, hipMemcpyDeviceToDevice, g->stream));
        GCHK(hipMemcpyAsync(g->arena.p + desc[k].ytab, g->d_tin.p + t_tab[k] + al((size_t)c.ow * 12), (size_t)c.oh * 12, hipMemcpyDeviceToDevice, g->stream));
        key_set(c.s.tab_key, c.H, c.W, c.oh, c.ow);
    }
    if (g->desc_bytes != bytes || std::memcmp(g->h_desc.p, img.data(), bytes) != 0) {
        // the previous upload out of h_desc has completed: every tick is collected (ev_done) before the next begins
        std::memcpy(g->h_desc.p, img.data(), bytes);
        GCHK(hipMemcpyAsync(g->d_desc.p, g->h_desc.p, bytes, hipMemcpyHostToDevice, g->stream));
        g->desc_bytes = bytes;
    }
    GCHK(hipMemsetAsync(g->d_tout.p, 0, (size_t)na * 4, g->stream));
    MultiArgs m{};
    m.cams = (const GmcCam*)g->d_desc.p; m.n = na; m.arena = g->arena.p; m.tin = g->d_tin.p; m.tout = g->d_tout.p;
    const int* d_prefix = (const int*)(g->d_desc.p + desc_b);
    auto grid_of = [&](int table) { return dim3((unsigned)prefix[(size_t)table * (na + 1) + na]); };      // blocks of a launch: the table's total
    {
        m.prefix = d_prefix + (size_t)kPrefixPlane * (na + 1);
        const dim3 gr = grid_of(kPrefixPlane);
        hipLaunchKernelGGL(gray_resize_multi_kernel, gr, dim3(256), 0, g->stream, m);
        hipLaunchKernelGGL(min_eig_multi_kernel, gr, dim3(256), 0, g->stream, m);
        hipLaunchKernelGGL(corner_mask_multi_kernel, gr, dim3(256), 0, g->stream, m, kQuality);
    }
    for (int l = 1; l <= max_top; ++l) {
        m.prefix = d_prefix + (size_t)prefix_level(l) * (na + 1);
        hipLaunchKernelGGL(pyr_down_multi_kernel, grid_of(prefix_level(l)), dim3(256), 0, g->stream, m, l);
    }
    if (prefix[(size_t)kPrefixLk * (na + 1) + na] > 0) {
        m.prefix = d_prefix + (size_t)kPrefixLk * (na + 1);
        hipLaunchKernelGGL(lk_multi_kernel, grid_of(kPrefixLk), dim3(64 * kLkWaves), 0, g->stream, m, kLk.win, kLk.max_iters, kLk.eps * kLk.eps, kLk.min_eig);
    }
    GCHK(hipGetLastError());
    GCHK(hipMemcpyAsync(g->h_tout.p, g->d_tout.p, o_total, hipMemcpyDeviceToHost, g->stream));
    GCHK(hipEventRecord(g->ev_done, g->stream));
    for (int k = 0; k < na; ++k) { MultiCam& c = g->cams[g->active[k]]; c.s.slot ^= 1; c.s.have_prev = true; c.s.ph = c.oh; c.s.pw = c.ow; }
    return 0;
}
}  // namespace

// One tick: frames[i] = camera i's BGR frame of heights[i] x widths[i], or NULL when that camera delivered none (its state stays as it is).
// Device object: stages the frames, enqueues every stage of every present camera on the object's stream and returns; the host half per
// camera (corner ordering, RANSAC) runs on at most min(present, 8) worker threads from now on.  Host object (device -1): the same through the
// host routines.  0 = ok, -1 = bad argument / a tick is pending, -2 = HIP error.
extern "C" int mi355_gmc_multi_begin(mi355_gmc_multi* g, const uint8_t* const* frames, const int* heights, const int* widths, int downscale) {
    if (!g || !frames || !heights || !widths || downscale < 1 || g->job_active) return -1;
    g->active.clear();
    for (int i = 0; i < g->n; ++i) {
        g->cams[i].active = false;
        if (!frames[i]) continue;
        if (heights[i] <= 0 || widths[i] <= 0 || heights[i] / downscale <= 0 || widths[i] / downscale <= 0) return -1;
        g->active.push_back(i);
    }
    g->downscale = downscale;
    for (int ci : g->active) { g->cams[ci].active = true; g->cams[ci].rc = 0; }
    if (g->active.empty()) { g->job_active = true; return 0; }
    if (g->host) {
        for (int ci : g->active) {
            const int rc = mi355_gmc_track_begin(g->single[ci], frames[ci], heights[ci], widths[ci], downscale);
            if (rc) {                                           // drop what has been begun: nothing of this tick stays pending
                for (int cj : g->active) { if (cj == ci) break; double H[6]; (void)mi355_gmc_track_finish(g->single[cj], H); }
                return rc;
            }
        }
    } else {
        const int rc = multi_begin_device(g, frames, heights, widths, downscale);
        if (rc) {
            (void)hipStreamSynchronize(g->stream); (void)hipGetLastError();
            for (int ci : g->active) cam_lost(g->cams[ci].s);
            return rc;
        }
    }
    multi_start_workers(g);
    return 0;
}

// Collect the tick: joins the workers; H_out [n_cameras][6] row-major 2 x 3 per camera, rows of absent cameras untouched.
extern "C" int mi355_gmc_multi_finish(mi355_gmc_multi* g, double* H_out) {
    if (!g || !H_out || !g->job_active) return -1;
    for (auto& t : g->workers) if (t.joinable()) t.join();
    g->workers.clear();
    g->job_active = false;
    int rc = 0;
    for (int ci : g->active) {
        const MultiCam& c = g->cams[ci];
        if (c.rc) { if (!rc) rc = c.rc; continue; }
        std::memcpy(H_out + 6 * (size_t)ci, c.Hm, sizeof(c.Hm));
    }
    return rc;
}

// The pending tick's frames as they sit on the device (dense BGR, each start 256-byte aligned; NULL for an absent camera), after one event
// wait for the upload -- the detector pass of the same tick reads them in place (mi355_yolo_infer_multi, frames_on_device = 1).  Valid until
// the next mi355_gmc_multi_begin.
extern "C" int mi355_gmc_multi_frames(mi355_gmc_multi* g, const uint8_t** dev_frames) {
    if (!g || g->host || !g->job_active || !dev_frames) return -1;
    GCHK(hipSetDevice(g->device));
    if (!g->active.empty()) GCHK(hipEventSynchronize(g->ev_up));
    for (int i = 0; i < g->n; ++i) dev_frames[i] = g->cams[i].active ? g->d_tin.p + g->cams[i].t_frame : nullptr;
    return 0;
}

// Forget camera `camera`'s previous frame (-1: every camera's); a pending tick is collected and dropped.
extern "C" int mi355_gmc_multi_reset(mi355_gmc_multi* g, int camera) {
    if (!g || camera < -1 || camera >= g->n) return -1;
    if (g->job_active) { std::vector<double> H((size_t)g->n * 6); (void)mi355_gmc_multi_finish(g, H.data()); }
    for (int i = 0; i < g->n; ++i) {
        if (camera >= 0 && i != camera) continue;
        if (g->host) (void)mi355_gmc_track_reset(g->single[i]); else cam_forget(g->cams[i].s);
    }
    return 0;
}

// Camera `camera`'s previous frame as the object holds it (tests), as mi355_gmc_track_state.
extern "C" int mi355_gmc_multi_state(const mi355_gmc_multi* g, int camera, int* oh, int* ow, int* n_pts, uint8_t* gray_out, float* pts_out, int pts_cap) {
    if (!g || camera < 0 || camera >= g->n || g->job_active) return -1;
    if (g->host) return mi355_gmc_track_state(g->single[camera], oh, ow, n_pts, gray_out, pts_out, pts_cap);
    cam_report(g->cams[camera].s, oh, ow, n_pts, gray_out, pts_out, pts_cap);
    return 0;
}
