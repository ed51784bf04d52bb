// The two operators YOLO11 adds to the engine (fp32 storage and arithmetic, canonical exp):
//   * depthwise 3x3 conv, stride 1 (DWConv of the non-legacy Detect/Pose class branch, Attention.pe) + bias (+SiLU) (+residual);
//   * PSA attention (C2PSA -> PSABlock -> Attention, between its qkv and pe convs): per frame and head,
//     softmax_j(q_i . k_j * key_dim^-0.5) applied to v, over the N = H/32 x W/32 pixels of the P5 map.
// Both read and write channel views of NHWC buffers (pixel stride `cs` floats), launch without allocating or synchronising
// (graph-capture safe) and take the frame count of the pass (tail chunks).  Every output element is one fixed sequence of
// operations that depends on its own frame only: deterministic and batch-invariant.
#include "common.h"
#include "detmath.h"

#include <algorithm>

namespace mi355 {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------------- depthwise conv
// Memory-bound (9 MACs per 4-byte output): a lane owns 4 consecutive channels of DW_ROWS vertically stacked output pixels and
// keeps the (DW_ROWS + K - 1) x K input window in flight as 16-byte loads, each loaded once and used by up to K outputs (3.0
// loads per output instead of 9 for K = 3); the K x K x 4 weights and the bias stay in registers.  Consecutive lanes take
// consecutive channel quads of one pixel, then the next pixel of the row: every wave reads whole pixel rows of the view.
// Per output: acc = +0, taps in (ky, kx) order as fma, + bias, SiLU, + residual -- the order of the conv epilogues.
constexpr int DW_ROWS = 4;

template <int K>
__global__ __launch_bounds__(256) void dwconv_kernel(DwConvArgs a) {
    constexpr int P = K / 2;
    const int nq = (a.C + 3) / 4;
    const int strips = (a.H + DW_ROWS - 1) / DW_ROWS;
    const long total = (long)a.B * strips * a.W * nq;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int q = (int)(i % nq);
        long r = i / nq;
        const int x = (int)(r % a.W); r /= a.W;
        const int y0 = (int)(r % strips) * DW_ROWS;
        const int b = (int)(r / strips);
        const int c = 4 * q;
        f32x4 w[K * K];
#pragma unroll
        for (int t = 0; t < K * K; ++t) w[t] = *(const f32x4*)(a.w + (size_t)t * a.c_pad + c);
        f32x4 acc[DW_ROWS];
#pragma unroll
        for (int o = 0; o < DW_ROWS; ++o) acc[o] = (f32x4){0.f, 0.f, 0.f, 0.f};
        const float* img = a.src + (size_t)b * a.H * a.W * a.src_cs + c;
#pragma unroll
        for (int iy = 0; iy < DW_ROWS + K - 1; ++iy) {
            const int yy = y0 - P + iy;
            const bool row_ok = yy >= 0 && yy < a.H;
#pragma unroll
            for (int kx = 0; kx < K; ++kx) {
                const int xx = x - P + kx;
                f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
                if (row_ok && xx >= 0 && xx < a.W) v = *(const f32x4*)(img + ((size_t)yy * a.W + xx) * a.src_cs);
#pragma unroll
                for (int o = 0; o < DW_ROWS; ++o) {
                    const int ky = iy - o;                              // output row y0 + o uses input row y0 + o - P + ky
                    if (ky >= 0 && ky < K) {
                        const f32x4 wt = w[ky * K + kx];
                        acc[o][0] = __builtin_fmaf(v[0], wt[0], acc[o][0]);
                        acc[o][1] = __builtin_fmaf(v[1], wt[1], acc[o][1]);
                        acc[o][2] = __builtin_fmaf(v[2], wt[2], acc[o][2]);
                        acc[o][3] = __builtin_fmaf(v[3], wt[3], acc[o][3]);
                    }
                }
            }
        }
        const f32x4 bias = *(const f32x4*)(a.bias + c);
        const int nc = a.C - c < 4 ? a.C - c : 4;                       // ragged last quad: scalar stores inside the view
#pragma unroll
        for (int o = 0; o < DW_ROWS; ++o) {
            const int y = y0 + o;
            if (y >= a.H) break;
            const size_t p = ((size_t)b * a.H + y) * a.W + x;
            f32x4 v = acc[o] + bias;
            if (a.act) { v[0] = det_silu(v[0]); v[1] = det_silu(v[1]); v[2] = det_silu(v[2]); v[3] = det_silu(v[3]); }
            float* d = a.dst + p * a.dst_cs + c;
            if (nc == 4) {
                if (a.res) v += *(const f32x4*)(a.res + p * a.res_cs + c);
                *(f32x4*)d = v;
            } else {
                for (int j = 0; j < nc; ++j) d[j] = v[j] + (a.res ? a.res[p * a.res_cs + c + j] : 0.f);
            }
        }
    }
}

const char* launch_dwconv(const DwConvArgs& a, hipStream_t st) {
    if (a.B <= 0 || a.H <= 0 || a.W <= 0 || a.C <= 0) return nullptr;
    if ((a.src_cs & 3) || (a.dst_cs & 3) || (a.res && (a.res_cs & 3)) || (a.c_pad & 3) || a.c_pad < a.C ||
        (((uintptr_t)a.src | (uintptr_t)a.dst | (uintptr_t)a.res | (uintptr_t)a.w | (uintptr_t)a.bias) & 15))
        return "dwconv: channel strides / views must be 16-byte aligned";
    const long total = (long)a.B * ((a.H + DW_ROWS - 1) / DW_ROWS) * a.W * ((a.C + 3) / 4);
    const unsigned grid = (unsigned)std::min<long>((total + 255) / 256, 1 << 16);
    if (a.k != 3) return "dwconv: kernel size must be 3";
    hipLaunchKernelGGL(dwconv_kernel<3>, dim3(grid), dim3(256), 0, st, a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

// -------------------------------------------------------------------------------------------------------- PSA attention
// One block = (query tile of 64 pixels, head, frame), 256 threads, exact softmax in two passes over the keys (no score row is
// stored, so any N fits; LDS holds one 64-key tile):
//   pass 1: per query the row max M and the row sum L = sum_j exp(s_j - M), s_j = (q . k_j) * key_dim^-0.5.  A lane owns one
//           query and 16 keys of every tile (wave w: keys 16w .. 16w+15): a tile's max and sum of its 16 keys are merged into the
//           lane's running pair (two-level, like the engine's blocked conv sums); the 4 lanes of a query merge in wave order.
//   pass 2: p_ij = exp(s_ij - M_i) (recomputed identically) goes to LDS, then lane (query, 16 output dims) adds the tile's
//           sum_j p_ij v_j (one fma chain from +0 per tile) to its accumulator; out = acc / L.
// Scores take the K row as a wave-uniform (broadcast) LDS read; P is read along the lanes (conflict-free) and V broadcast.
constexpr int ATT_QT = 64, ATT_KT = 64, ATT_KD = 32, ATT_HD = 64;

__device__ __forceinline__ float att_score(const float (&q)[ATT_KD], const float* krow, float scale) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < ATT_KD; c += 4) {
        const f32x4 k4 = *(const f32x4*)(krow + c);
        s = __builtin_fmaf(q[c], k4[0], s);
        s = __builtin_fmaf(q[c + 1], k4[1], s);
        s = __builtin_fmaf(q[c + 2], k4[2], s);
        s = __builtin_fmaf(q[c + 3], k4[3], s);
    }
    return s * scale;
}

__global__ __launch_bounds__(256) void psa_attention_kernel(PsaAttnArgs a) {
    __shared__ __attribute__((aligned(16))) float ks[ATT_KT][ATT_KD];
    __shared__ __attribute__((aligned(16))) float vs[ATT_KT][ATT_HD];
    __shared__ __attribute__((aligned(16))) float ps[ATT_KT][ATT_QT];
    __shared__ float red_m[4][ATT_QT], red_l[4][ATT_QT];
    const int t = threadIdx.x, qi = t & 63, wv = t >> 6;
    const int q0 = blockIdx.x * ATT_QT, h = blockIdx.y, b = blockIdx.z;
    const int N = a.N, nh = a.heads;
    const float* base = a.qkv + (size_t)b * N * a.qkv_cs;
    const int qoff = h * ATT_KD, koff = nh * ATT_KD + h * ATT_KD, voff = 2 * nh * ATT_KD + h * ATT_HD;
    const int qn = q0 + qi;
    float q[ATT_KD];
#pragma unroll
    for (int c = 0; c < ATT_KD; c += 4) {
        f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (qn < N) v = *(const f32x4*)(base + (size_t)qn * a.qkv_cs + qoff + c);
        q[c] = v[0]; q[c + 1] = v[1]; q[c + 2] = v[2]; q[c + 3] = v[3];
    }
    const float NEG = -__builtin_huge_valf();
    const int ntiles = (N + ATT_KT - 1) / ATT_KT;
    auto load_k = [&](int j0) {
        for (int e = t; e < ATT_KT * ATT_KD / 4; e += 256) {
            const int j = e / (ATT_KD / 4), c = 4 * (e % (ATT_KD / 4));
            f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (j0 + j < N) v = *(const f32x4*)(base + (size_t)(j0 + j) * a.qkv_cs + koff + c);
            *(f32x4*)&ks[j][c] = v;
        }
    };
    // ---- pass 1: row max and row sum
    float m = NEG, l = 0.f;
    for (int tile = 0; tile < ntiles; ++tile) {
        const int j0 = tile * ATT_KT;
        __syncthreads();
        load_k(j0);
        __syncthreads();
        const int nk = min(16, N - j0 - 16 * wv);                      // valid keys of this lane's 16 (wave-uniform)
        if (nk <= 0) continue;
        float s[16];
        float tm = NEG;
#pragma unroll
        for (int jj = 0; jj < 16; ++jj) {
            s[jj] = jj < nk ? att_score(q, ks[16 * wv + jj], a.scale) : NEG;
            tm = fmaxf(tm, s[jj]);
        }
        float ts = 0.f;
#pragma unroll
        for (int jj = 0; jj < 16; ++jj) if (jj < nk) ts += det_expf(s[jj] - tm);
        const float mn = fmaxf(m, tm);
        l = (l > 0.f ? l * det_expf(m - mn) : 0.f) + ts * det_expf(tm - mn);
        m = mn;
    }
    red_m[wv][qi] = m; red_l[wv][qi] = l;
    __syncthreads();
    float M = NEG;
#pragma unroll
    for (int g = 0; g < 4; ++g) M = fmaxf(M, red_m[g][qi]);
    float L = 0.f;
#pragma unroll
    for (int g = 0; g < 4; ++g) if (red_l[g][qi] > 0.f) L += red_l[g][qi] * det_expf(red_m[g][qi] - M);
    // ---- pass 2: P V
    float acc[16];
#pragma unroll
    for (int d = 0; d < 16; ++d) acc[d] = 0.f;
    for (int tile = 0; tile < ntiles; ++tile) {
        const int j0 = tile * ATT_KT;
        __syncthreads();
        load_k(j0);
        for (int e = t; e < ATT_KT * ATT_HD / 4; e += 256) {
            const int j = e / (ATT_HD / 4), c = 4 * (e % (ATT_HD / 4));
            f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (j0 + j < N) v = *(const f32x4*)(base + (size_t)(j0 + j) * a.qkv_cs + voff + c);
            *(f32x4*)&vs[j][c] = v;
        }
        __syncthreads();
#pragma unroll
        for (int jj = 0; jj < 16; ++jj) {
            const int j = 16 * wv + jj;
            ps[j][qi] = j0 + j < N ? det_expf(att_score(q, ks[j], a.scale) - M) : 0.f;
        }
        __syncthreads();
        float part[16];
#pragma unroll
        for (int d = 0; d < 16; ++d) part[d] = 0.f;
        const int nkt = min(ATT_KT, N - j0);
        for (int j = 0; j < nkt; ++j) {
            const float p = ps[j][qi];
#pragma unroll
            for (int d = 0; d < 16; d += 4) {
                const f32x4 v4 = *(const f32x4*)&vs[j][16 * wv + d];
                part[d] = __builtin_fmaf(p, v4[0], part[d]);
                part[d + 1] = __builtin_fmaf(p, v4[1], part[d + 1]);
                part[d + 2] = __builtin_fmaf(p, v4[2], part[d + 2]);
                part[d + 3] = __builtin_fmaf(p, v4[3], part[d + 3]);
            }
        }
#pragma unroll
        for (int d = 0; d < 16; ++d) acc[d] += part[d];
    }
    if (qn >= N) return;
    float* out = a.dst + ((size_t)b * N + qn) * a.dst_cs + h * ATT_HD + 16 * wv;
#pragma unroll
    for (int d = 0; d < 16; d += 4)
        *(f32x4*)(out + d) = (f32x4){acc[d] / L, acc[d + 1] / L, acc[d + 2] / L, acc[d + 3] / L};
}

const char* launch_psa_attention(const PsaAttnArgs& a, hipStream_t st) {
    if (a.B <= 0 || a.N <= 0) return nullptr;
    if (a.key_dim != ATT_KD || a.head_dim != ATT_HD) return "psa attention: only key_dim 32 / head_dim 64 (every YOLO11 scale)";
    if (a.heads <= 0 || a.heads > 65535 || a.B > 65535) return "psa attention: bad head / frame count";
    if ((a.qkv_cs & 3) || (a.dst_cs & 3) || (((uintptr_t)a.qkv | (uintptr_t)a.dst) & 15))
        return "psa attention: channel strides / views must be 16-byte aligned";
    hipLaunchKernelGGL(psa_attention_kernel, dim3((a.N + ATT_QT - 1) / ATT_QT, a.heads, a.B), dim3(256), 0, st, a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

}  // namespace mi355
