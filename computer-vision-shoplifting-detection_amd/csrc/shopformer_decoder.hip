// The GCAE decoder of both Shopformer variants as ONE kernel: tokens [n][ntok][L*V] -> poses [n][2][T][V] and,
// when the input windows are given, pose_error [n][T][V] = mean over the 2 channels of (pose - window)^2.
//
// After initial_proj nothing mixes rows: a (2,1)/(2,1) transposed convolution makes frames 2t and 2t+1 from frame t alone with one
// H x H matrix per parity, a 1x1 convolution is pointwise.  So a tile of 16 (window, token, joint) rows fans out 1 -> 2 -> 4 (-> 8)
// tiles through the layers and never leaves the registers of its wave: the accumulators of v_mfma_f32_16x16x4_f32 (weights as the A
// operand) hold 4 consecutive output features of one row per lane, which is exactly the B-operand fragment of the next layer.
// Only initial_proj, whose rows are (window, token), and the optional interpolation along time go through LDS.
//
// Order rule: an output element is one k-ordered fma chain per layer whose order depends on the layer alone; a row's chain never
// reads another row.  The interpolation and pose_error are written with explicitly rounded operations (no contraction), in the
// order the header states, so that a numpy float32 restatement gives the same bits.
#include "shopformer.h"

namespace mi355 {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// y = act(W[:, tap, :] . x + b) for the 16 rows of a tile: x[cb] / y[c] are fragments of 16 features (lane: 4 features of one row)
__device__ __forceinline__ void sd_layer(const f32x4 (&x)[4], f32x4 (&y)[4], const float* __restrict__ w, const float* __restrict__ b,
                                         int nct, int cib, int ntaps, int tap, bool relu, int lane) {
    const int q = lane >> 4;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (c < nct) {
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
                if (cb < cib) {
                    const f32x4 wv = *reinterpret_cast<const f32x4*>(w + ((size_t)(c * ntaps + tap) * cib + cb) * 256 + lane * 4);
#pragma unroll
                    for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[s], x[cb][s], acc, 0, 0, 0);
                }
            acc += *reinterpret_cast<const f32x4*>(b + c * 16 + q * 4);
            if (relu)
#pragma unroll
                for (int s = 0; s < 4; ++s) acc[s] = __builtin_fmaxf(acc[s], 0.f);
        }
        y[c] = acc;
    }
}

__global__ __launch_bounds__(SF_THREADS) void shopformer_decoder_kernel(const SfDecParams* __restrict__ pp, const float* __restrict__ tokens,
                                                                         int n, float* __restrict__ poses, float* __restrict__ pose_error,
                                                                         const float* __restrict__ windows) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const SfDecParams& p = *pp;             // device memory, uniform
    const int w0 = blockIdx.x * p.G, nwin = min(p.G, n - w0);
    if (nwin <= 0) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const int j = lane & 15, q = lane >> 4;
    const int V = p.V, H = p.H, Din = p.Din, nt = p.ntok, T = p.T, Td = p.Td, R = nwin * nt;
    float* tok = lds + p.offTok;            // [R][csT]
    float* X = lds + p.offX;                // [R * V][csH]: initial_proj's output as (window, token, joint) rows of H channels
    float* ob = lds + p.offOut;             // [nwin][2][Td][V]: what the layers emit, before the interpolation

    for (int it = threadIdx.x; it < R * Din; it += blockDim.x) tok[(it / Din) * p.csT + it % Din] = tokens[(size_t)w0 * nt * Din + it];
    __syncthreads();

    // ---- initial_proj: rows (window, token), K = Din, N = V * H with the output features already in (joint, channel) order
    {
        const int nct2 = (V * H) >> 5, cib = (Din + 15) >> 4, mtiles = (R + 15) >> 4;
        for (int job = wave; job < mtiles * nct2; job += nwaves) {
            const int ct = (job % nct2) * 2, m = (job / nct2) * 16 + j, mc = min(m, R - 1);
            f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
            for (int cb = 0; cb < cib; ++cb) {
                const int k0 = cb * 16 + q * 4;
                const f32x4 xv = k0 < Din ? *reinterpret_cast<const f32x4*>(tok + mc * p.csT + k0) : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const f32x4 wv = *reinterpret_cast<const f32x4*>(p.ipw + ((size_t)(ct + c) * cib + cb) * 256 + lane * 4);
#pragma unroll
                    for (int s = 0; s < 4; ++s) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[s], xv[s], acc[c], 0, 0, 0);
                }
            }
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int n0 = (ct + c) * 16 + q * 4, v = n0 / H, h = n0 - v * H;
                if (m < R) *reinterpret_cast<f32x4*>(X + (mc * V + v) * p.csH + h) = acc[c] + *reinterpret_cast<const f32x4*>(p.ipb + n0);
            }
        }
    }
    __syncthreads();

    // ---- the four layers: a tile of 16 rows stays in the wave's registers from X to the 2 output channels of its 4 or 8 frames
    {
        const int NR = R * V, tiles = (NR + 15) >> 4, hct = H >> 4;
        const int f0 = p.f[0], f1 = p.f[1], f2 = p.f[2];
        for (int tile = wave; tile < tiles; tile += nwaves) {
            const int r = tile * 16 + j, rc = min(r, NR - 1);
            const int wt = rc / V, v = rc - wt * V, w = wt / nt, tk = wt - w * nt;
            f32x4 x0[4], y0[4], y1[4], y2[4], y3[4];
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
                x0[cb] = cb < hct ? *reinterpret_cast<const f32x4*>(X + rc * p.csH + cb * 16 + q * 4) : (f32x4){0.f, 0.f, 0.f, 0.f};
            for (int p0 = 0; p0 < f0; ++p0) {
                sd_layer(x0, y0, p.w[0], p.b[0], hct, hct, f0, p0, true, lane);
                for (int p1 = 0; p1 < f1; ++p1) {
                    sd_layer(y0, y1, p.w[1], p.b[1], hct, hct, f1, p1, true, lane);
                    for (int p2 = 0; p2 < f2; ++p2) {
                        sd_layer(y1, y2, p.w[2], p.b[2], hct, hct, f2, p2, true, lane);
                        sd_layer(y2, y3, p.w[3], p.b[3], 1, hct, 1, 0, false, lane);
                        const int fr = ((tk * f0 + p0) * f1 + p1) * f2 + p2;
                        if (r < NR && q == 0) {
                            ob[((w * 2 + 0) * Td + fr) * V + v] = y3[0][0];
                            ob[((w * 2 + 1) * Td + fr) * V + v] = y3[0][1];
                        }
                    }
                }
            }
        }
    }
    __syncthreads();

    // ---- frames Td -> T (align_corners=False, linear along time only), the output, and the squared error against the window
    const int TV = T * V;
    for (int it = threadIdx.x; it < nwin * TV; it += blockDim.x) {
        const int w = it / TV, rem = it - w * TV, t = rem / V, v = rem - t * V;
        float r[2];
        if (p.interp) {
            float src = __fsub_rn(__fmul_rn(p.scale, (float)t + 0.5f), 0.5f);
            src = __builtin_fmaxf(src, 0.f);
            const int i0 = min((int)src, Td - 1), i1 = min(i0 + 1, Td - 1);
            const float wgt = src - (float)i0, wa = 1.0f - wgt;
#pragma unroll
            for (int c = 0; c < 2; ++c)
                r[c] = __fadd_rn(__fmul_rn(wa, ob[((w * 2 + c) * Td + i0) * V + v]), __fmul_rn(wgt, ob[((w * 2 + c) * Td + i1) * V + v]));
        } else {
#pragma unroll
            for (int c = 0; c < 2; ++c) r[c] = ob[((w * 2 + c) * Td + t) * V + v];
        }
        const size_t base = (size_t)(w0 + w) * 2 * TV;
        poses[base + rem] = r[0];
        poses[base + TV + rem] = r[1];
        if (pose_error) {
            const float d0 = r[0] - windows[base + rem], d1 = r[1] - windows[base + TV + rem];
            pose_error[(size_t)(w0 + w) * TV + rem] = __fmul_rn(0.5f, __fadd_rn(__fmul_rn(d0, d0), __fmul_rn(d1, d1)));
        }
    }
}

}  // namespace

const char* prepare_shopformer_decoder_device() {
    const hipError_t e = hipFuncSetAttribute((const void*)shopformer_decoder_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, SF_LDS_BYTES);
    return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

const char* launch_shopformer_decoder(const SfDecParams* p_dev, int group, int lds_bytes, const float* tokens, int n, float* poses,
                                      float* pose_error, const float* windows, hipStream_t stream, long long* launches) {
    hipLaunchKernelGGL(shopformer_decoder_kernel, dim3((n + group - 1) / group), dim3(SF_THREADS), lds_bytes, stream, p_dev, tokens, n, poses,
                       pose_error, windows);
    ++*launches;
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

}  // namespace mi355
