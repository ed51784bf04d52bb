// Pose windows: retained poses [P][V_src][2] and window starts -> the normalised windows [n][2][seq_len][V] fp32 that
// cvsd_amd/shopformer.py:_window_tensor builds on the host, bit for bit.  ONE statement of the per-window arithmetic, pose_window<F>,
// compiled for both targets: a wave of the kernel runs it with 64 lanes, the host twin (device = -1) with one.  Every operation is in
// the poses' own type F (float or double) in numpy's order, with one rounding to fp32 at the end; no contraction, IEEE division.
#include "engine_internal.h"
#include "pose_windows.h"

#include <cstddef>
#include <limits>
#include <string>
#include <vector>

#pragma clang fp contract(off)

namespace mi355 {
namespace {

__host__ __device__ inline float pw_abs(float a) { return __builtin_fabsf(a); }
__host__ __device__ inline double pw_abs(double a) { return __builtin_fabs(a); }

// np.max: the larger, a NaN if either is one (so the result does not depend on the order)
template <class F> __host__ __device__ inline F pw_max(F a, F b) { return a != a ? a : b != b ? b : a > b ? a : b; }

// the phases of a window hand their results to the other lanes through `scratch` (LDS): a workgroup barrier on the device, every
// wave of the workgroup runs the same phases; nothing on the host, where one lane runs them in turn
__host__ __device__ inline void pw_sync() {
#if defined(__HIP_DEVICE_COMPILE__)
    __syncthreads();
#endif
}

template <class F> __host__ __device__ inline F pw_lanes_max(F m) {
#if defined(__HIP_DEVICE_COMPILE__)
    for (int d = 32; d >= 1; d >>= 1) m = pw_max(m, __shfl_xor(m, d, 64));
#endif
    return m;
}

// a shoulder is missing when np.allclose(xy, 0) says so: |x| <= 1e-8 and |y| <= 1e-8, compared in double
template <class F> __host__ __device__ inline bool pw_missing(F x, F y) {
    return pw_abs((double)x) <= 1e-8 && pw_abs((double)y) <= 1e-8;
}

// One window.  `pose0` = the first of its seq_len consecutive poses, `scratch` = 2 * T * V + 4 values of F shared by the lanes, `out`
// = its [2][T][V] floats (written when `store`).  Lane `lane` of `nlanes` takes the joints lane, lane + nlanes, ... of the (t, v) order.
template <class F>
__host__ __device__ inline void pose_window(const F* pose0, int V_src, int T, int V, int neck, F* scratch, float* out, int lane, int nlanes,
                                            bool store) {
    const int TV = T * V, vin = neck ? 17 : V;
    F *sx = scratch, *sy = scratch + TV, *cen = scratch + 2 * TV;
    // 1. gather: joints the source does not deliver are zero; joint 17 of a neck window is made from the shoulders (joints 5, 6)
    for (int i = lane; i < TV; i += nlanes) {
        const int t = i / V, v = i - t * V;
        const F* p = pose0 + (size_t)t * V_src * 2;
        F x = F(0), y = F(0);
        if (v < vin && v < V_src) {
            x = p[2 * v]; y = p[2 * v + 1];
        } else if (neck && v == 17) {
            const F lx = p[10], ly = p[11], rx = p[12], ry = p[13];
            const bool l0 = pw_missing(lx, ly), r0 = pw_missing(rx, ry);
            if (l0 && r0) { x = F(0); y = F(0); }
            else if (l0) { x = rx; y = ry; }
            else if (r0) { x = lx; y = ly; }
            else { x = (lx + rx) / F(2); y = (ly + ry) / F(2); }
        }
        sx[i] = x; sy[i] = y;
    }
    pw_sync();
    // 2. the centre: per coordinate ONE chain over the valid joints in (t, v) order, as np.add.reduce walks the rows (it starts from the
    //    first valid row, which differs from 0 + row only in the sign of a zero); one lane per coordinate
    for (int c = lane; c < 2; c += nlanes) {
        F s = F(0);
        int m = 0;
#pragma unroll 4
        for (int i = 0; i < TV; ++i) {                 // selects, not branches: the loads of later joints need not wait for the chain
            const F x = sx[i], y = sy[i], v = c ? y : x;
            const bool valid = x != F(0) || y != F(0);
            s = !valid ? s : m ? s + v : v;
            m += valid;
        }
        cen[c] = m ? s / F(m) : F(0);
        if (c == 0) cen[2] = F(m);
    }
    pw_sync();
    // 3. the scale: the largest |offset| of a valid joint (any order), + 1e-6 in F; a window without a valid joint keeps scale 1
    const F cx = cen[0], cy = cen[1];
    const bool any = cen[2] != F(0);
    F mx = F(0);
    for (int i = lane; i < TV; i += nlanes)
        if (sx[i] != F(0) || sy[i] != F(0)) mx = pw_max(pw_max(mx, pw_abs(sx[i] - cx)), pw_abs(sy[i] - cy));
    mx = pw_lanes_max(mx);
    const F scale = any ? mx + F(1e-6) : F(1);
    // 4. every joint, the invalid ones too; np.nan_to_num(nan=0, posinf=0, neginf=0) before the one rounding to fp32
    if (!store) return;
    for (int i = lane; i < TV; i += nlanes) {
        F a = (sx[i] - cx) / scale, b = (sy[i] - cy) / scale;
        if (!(pw_abs(a) <= std::numeric_limits<F>::max())) a = F(0);
        if (!(pw_abs(b) <= std::numeric_limits<F>::max())) b = F(0);
        out[i] = (float)a; out[TV + i] = (float)b;
    }
}

// a wave per window, PW_WAVES windows per workgroup; the waves of the last workgroup that have no window redo the last one without
// storing it, so that every wave meets every barrier
template <class F>
__global__ __launch_bounds__(PW_WAVES * 64) void pose_windows_kernel(const F* __restrict__ poses, const int* __restrict__ starts, int n, int V_src,
                                                                     int T, int V, int neck, float* __restrict__ windows) {
    extern __shared__ double pw_lds[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * PW_WAVES + wave;
    const bool live = w < n;
    const size_t wi = live ? (size_t)w : (size_t)n - 1;
    F* scratch = reinterpret_cast<F*>(pw_lds) + (size_t)wave * (2 * T * V + 4);
    pose_window<F>(poses + (size_t)starts[wi] * V_src * 2, V_src, T, V, neck, scratch, windows + wi * 2 * T * V, lane, 64, live);
}

template <class F>
void pose_windows_host(const F* poses, int V_src, const int* starts, int n, int T, int V, int neck, float* windows) {
    std::vector<F> scratch((size_t)2 * T * V + 4);
    for (int i = 0; i < n; ++i)
        pose_window<F>(poses + (size_t)starts[i] * V_src * 2, V_src, T, V, neck, scratch.data(), windows + (size_t)i * 2 * T * V, 0, 1, true);
}

struct DevBuf {                        // mi355_pose_windows' three allocations, freed on every way out
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
};

}  // namespace

int pose_windows_validate(const void* poses, int dtype, int P, int V_src, const int* starts, int n, int seq_len, int V, int neck) {
    if (dtype != MI355_POSE_F32 && dtype != MI355_POSE_F64) return fail(MI355_EINVAL, "pose windows: dtype must be MI355_POSE_F32 or MI355_POSE_F64");
    if (n < 0 || P < 0) return fail(MI355_EINVAL, "pose windows: negative count");
    if (V_src < 1) return fail(MI355_EINVAL, "pose windows: V_src must be at least 1");
    if (seq_len < 1 || V < 1 || (long long)seq_len * V > PW_MAX_TV) return fail(MI355_EINVAL, "pose windows: seq_len and V must be positive with seq_len * V <= " + std::to_string(PW_MAX_TV));
    if (neck && V != 18) return fail(MI355_EINVAL, "pose windows: neck needs V = 18 (17 COCO joints + the neck)");
    if (neck && V_src < 7) return fail(MI355_EINVAL, "pose windows: neck needs both shoulders (V_src >= 7)");
    if (n > 0 && (!poses || !starts)) return fail(MI355_EINVAL, "pose windows: null argument");
    for (int i = 0; i < n; ++i)
        if (starts[i] < 0 || (long long)starts[i] + seq_len > P)
            return fail(MI355_EINVAL, "pose windows: starts[" + std::to_string(i) + "] = " + std::to_string(starts[i]) + " leaves the " + std::to_string(P) + " poses");
    return MI355_OK;
}

const char* launch_pose_windows(const void* poses_dev, int dtype, int V_src, const int* starts_dev, int n, int seq_len, int V, int neck,
                                float* windows_dev, hipStream_t stream, long long* launches) {
    const dim3 grid((n + PW_WAVES - 1) / PW_WAVES), block(PW_WAVES * 64);
    const size_t per = (size_t)2 * seq_len * V + 4;
    if (dtype == MI355_POSE_F64)
        hipLaunchKernelGGL(pose_windows_kernel<double>, grid, block, PW_WAVES * per * sizeof(double), stream, (const double*)poses_dev, starts_dev, n,
                           V_src, seq_len, V, neck, windows_dev);
    else
        hipLaunchKernelGGL(pose_windows_kernel<float>, grid, block, PW_WAVES * per * sizeof(float), stream, (const float*)poses_dev, starts_dev, n,
                           V_src, seq_len, V, neck, windows_dev);
    ++*launches;
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

}  // namespace mi355

using namespace mi355;

extern "C" int mi355_pose_windows(int device, const void* poses, int dtype, int P, int V_src, const int* starts, int n, int seq_len, int V,
                                  int neck, float* windows_out) {
    const int rc = pose_windows_validate(poses, dtype, P, V_src, starts, n, seq_len, V, neck);
    if (rc) return rc;
    if (n == 0) return MI355_OK;
    if (!windows_out) return fail(MI355_EINVAL, "pose windows: null output");
    if (device < 0) {
        if (dtype == MI355_POSE_F64) pose_windows_host((const double*)poses, V_src, starts, n, seq_len, V, neck, windows_out);
        else pose_windows_host((const float*)poses, V_src, starts, n, seq_len, V, neck, windows_out);
        return MI355_OK;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(MI355_EHIP, "no HIP device: the pose-window kernel needs an MI355X (device = -1 runs its host twin)");
    if (device >= ndev) return fail(MI355_EINVAL, "device index out of range");
    HIPCHK(hipSetDevice(device));
    const size_t pose_bytes = (size_t)P * V_src * 2 * (dtype == MI355_POSE_F64 ? 8 : 4), out_bytes = (size_t)n * 2 * seq_len * V * 4;
    DevBuf dp, ds, dw;
    HIPCHK(hipMalloc(&dp.p, pose_bytes));
    HIPCHK(hipMalloc(&ds.p, (size_t)n * 4));
    HIPCHK(hipMalloc(&dw.p, out_bytes));
    HIPCHK(hipMemcpy(dp.p, poses, pose_bytes, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ds.p, starts, (size_t)n * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dw.p, windows_out, out_bytes, hipMemcpyHostToDevice));      // what the caller pre-filled stays where the kernel does not write
    long long launches = 0;
    KCHK(launch_pose_windows(dp.p, dtype, V_src, (const int*)ds.p, n, seq_len, V, neck, (float*)dw.p, nullptr, &launches));
    HIPCHK(hipMemcpy(windows_out, dw.p, out_bytes, hipMemcpyDeviceToHost));
    return MI355_OK;
}
