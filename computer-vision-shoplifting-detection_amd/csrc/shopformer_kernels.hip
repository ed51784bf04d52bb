// Shopformer score path as ONE kernel.  A workgroup of 512 threads owns G consecutive windows; every activation of
// those windows lives in LDS from the normalised input to the score, HBM is touched for the input window, the weights (L2-resident,
// pre-packed as MFMA A-operand fragments) and the outputs.
//
// Every matrix product -- X.W of the graph convolutions, the 9 x 1 temporal convolutions as implicit GEMM (K = 9 taps x C), the 1 x 1
// residual convolutions, every transformer linear layer -- goes through sf_mm(): v_mfma_f32_16x16x4_f32 with the weights as the A operand
// (16 output features) and 16 activation rows read from LDS as the B operand, so a lane ends up with 4 consecutive output features of one
// row (one float4 store).  Each output element is one accumulator: a k-ordered fma chain over (tap, input feature) whose order depends on
// nothing but the layer, so a window's score has the same bits alone, in any batch and at any position of it.  Taps that fall into the
// zero padding of the time axis are skipped per output frame (they would add +0).
#include "shopformer.h"
#include "detmath.h"

namespace mi355 {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

enum { MM_RELU = 1, MM_ACC_INIT = 2, MM_FIRST = 4, MM_GELU = 8 };

// exact (erf) GELU; the device library's erff is straight-line code on its argument: the same bits at every position
__device__ __forceinline__ float sf_gelu(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

struct Mm {
    const float* in; int in_cs, K;        // LDS rows of K features (K % 4 == 0); MM_FIRST: rows of 2 floats (A.X of the input)
    float* out; int out_cs, N;            // LDS rows of N features (N % 4 == 0); may alias `in` when one job covers all N (N <= 64)
    const float* w; const float* bias;    // global: [N tile][ntaps][K block 16][lane][4], bias padded to 16
    int ntaps, stride, pad;               // input frame = out frame * stride + tap - pad
    int V, R;                             // rows per (window, frame); rows per output frame of the group (= windows * V)
    int in_w, out_w;                      // rows between two windows of the group
    int Tin, Tout;
    int flags;
    const float *w0, *b0;                 // MM_FIRST: block 0's graph-conv weights [H][2] and bias (global)
    int ncm;                              // output tiles of 16 a wave takes per job: 0 = 4; 1 or 2 spread a narrow layer over more waves
};

// B-operand fragment: 4 consecutive input features of one activation row (zeros beyond K)
__device__ __forceinline__ f32x4 sf_load_b(const Mm& a, int row, int k0) {
    if (k0 >= a.K) return (f32x4){0.f, 0.f, 0.f, 0.f};
    if (a.flags & MM_FIRST) {             // relu((A.X)[row] . W0 + b0), recomputed instead of stored: the 64 x T x V map never exists
        const float2 ax = *reinterpret_cast<const float2*>(a.in + row * 2);
        f32x4 r;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const float2 w = *reinterpret_cast<const float2*>(a.w0 + (k0 + s) * 2);
            r[s] = __builtin_fmaxf(__builtin_fmaf(ax.y, w.y, __builtin_fmaf(ax.x, w.x, 0.f)) + a.b0[k0 + s], 0.f);
        }
        return r;
    }
    return *reinterpret_cast<const f32x4*>(a.in + row * a.in_cs + k0);
}

// out[row(t_o, m)][n] = epilogue(sum over valid taps, k of in[row(t_in, m)][k] * W[n][tap][k]); the whole workgroup calls it
__device__ void sf_mm(const Mm& a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const int j = lane & 15, q = lane >> 4;
    const int mtiles = (a.R + 15) >> 4, mpairs = (mtiles + 1) >> 1;
    const int ncm = a.ncm ? a.ncm : 4;    // a chain's order does not depend on how the output tiles are dealt out
    const int nct = (a.N + 15) >> 4, nchunks = (nct + ncm - 1) / ncm, cib = (a.K + 15) >> 4;
    const int njobs = a.Tout * mpairs * nchunks;
    for (int job = wave; job < njobs; job += nwaves) {
        const int chunk = job % nchunks, mp = (job / nchunks) % mpairs, to = job / (nchunks * mpairs);
        const int ct0 = chunk * ncm, nc = min(ncm, nct - ct0);
        int in_base[2], out_row[2];
        bool live[2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const int m = (mp * 2 + mt) * 16 + j;
            const int mc = min(m, a.R - 1), win = mc / a.V, v = mc - win * a.V;
            live[mt] = m < a.R;
            in_base[mt] = win * a.in_w + v;
            out_row[mt] = win * a.out_w + to * a.V + v;
        }
        f32x4 acc[4][2];
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const int n0 = (ct0 + c) * 16 + q * 4;
                acc[c][mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
                if ((a.flags & MM_ACC_INIT) && c < nc && live[mt] && n0 < a.N)
                    acc[c][mt] = *reinterpret_cast<const f32x4*>(a.out + out_row[mt] * a.out_cs + n0);
            }
        for (int tap = 0; tap < a.ntaps; ++tap) {
            const int tin = to * a.stride + tap - a.pad;
            if (tin < 0 || tin >= a.Tin) continue;                 // zero padding of the time axis: uniform over the job
            for (int cb = 0; cb < cib; ++cb) {
                f32x4 x[2], w[4];
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) x[mt] = sf_load_b(a, in_base[mt] + tin * a.V, cb * 16 + q * 4);
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (c < nc) w[c] = *reinterpret_cast<const f32x4*>(a.w + ((size_t)((ct0 + c) * a.ntaps + tap) * cib + cb) * 256 + lane * 4);
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (c < nc)
#pragma unroll
                            for (int mt = 0; mt < 2; ++mt)
                                acc[c][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[c][s], x[mt][s], acc[c][mt], 0, 0, 0);
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const int n0 = (ct0 + c) * 16 + q * 4;
                if (c < nc && live[mt] && n0 < a.N) {
                    f32x4 r = acc[c][mt];
                    if (a.bias) r += *reinterpret_cast<const f32x4*>(a.bias + n0);
                    if (a.flags & MM_RELU)
#pragma unroll
                        for (int s = 0; s < 4; ++s) r[s] = __builtin_fmaxf(r[s], 0.f);
                    if (a.flags & MM_GELU)
#pragma unroll
                        for (int s = 0; s < 4; ++s) r[s] = sf_gelu(r[s]);
                    *reinterpret_cast<f32x4*>(a.out + out_row[mt] * a.out_cs + n0) = r;
                }
            }
    }
}

// plain rows x K -> rows x N
__device__ void sf_linear(const float* in, int in_cs, int K, float* out, int out_cs, int N, SfLin l, int rows, int flags, int ncm = 0) {
    Mm a{};
    a.ncm = ncm;
    a.in = in; a.in_cs = in_cs; a.K = K; a.out = out; a.out_cs = out_cs; a.N = N; a.w = l.w; a.bias = l.b;
    a.ntaps = 1; a.stride = 1; a.pad = 0; a.V = rows; a.R = rows; a.in_w = 0; a.out_w = 0; a.Tin = 1; a.Tout = 1; a.flags = flags;
    sf_mm(a);
}

// in place: x[(w, t, v)][c] <- sum_u adj[v][u] x[(w, t, u)][c]; a thread owns 4 channels of one (window, frame)
__device__ void sf_adj_inplace(float* x, int cs, int C, int frames, int V, int nnz, const float* col, const float* val) {
    const int c4n = C >> 2;
    for (int it = threadIdx.x; it < frames * c4n; it += blockDim.x) {
        const int fr = it / c4n, c0 = (it - fr * c4n) * 4;
        float* base = x + (size_t)fr * V * cs + c0;
        f32x4 o[SF_MAX_V];
#pragma unroll
        for (int v = 0; v < SF_MAX_V; ++v) {
            o[v] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (v < V)
                for (int e = 0; e < nnz; ++e) {
                    const float a = val[v * nnz + e];
                    const f32x4 xv = *reinterpret_cast<const f32x4*>(base + (int)col[v * nnz + e] * cs);
#pragma unroll
                    for (int s = 0; s < 4; ++s) o[v][s] = __builtin_fmaf(a, xv[s], o[v][s]);
                }
        }
#pragma unroll
        for (int v = 0; v < SF_MAX_V; ++v)
            if (v < V) *reinterpret_cast<f32x4*>(base + v * cs) = o[v];
    }
}

// sum over the 16 lanes of a row group, every lane gets the same bits (fixed xor tree)
__device__ __forceinline__ float sf_sum16(float v) {
    v += __shfl_xor(v, 8, 16);
    v += __shfl_xor(v, 4, 16);
    v += __shfl_xor(v, 2, 16);
    v += __shfl_xor(v, 1, 16);
    return v;
}

// out[r] = LayerNorm(a[r] + b[r]) * g + beta, 16 lanes per row (out may alias a)
__device__ void sf_add_norm(const float* a, const float* b, float* out, int cs, int D, int rows, SfNorm n) {
    const int sub = threadIdx.x & 15, grp = threadIdx.x >> 4, ngrp = blockDim.x >> 4;
    for (int r0 = 0; r0 < rows; r0 += ngrp) {                       // uniform trip count: the shuffles need every lane
        const int r = min(r0 + grp, rows - 1);
        float s = 0.f;
        for (int i = sub; i < D; i += 16) s += a[r * cs + i] + b[r * cs + i];
        const float mean = sf_sum16(s) / (float)D;
        float v = 0.f;
        for (int i = sub; i < D; i += 16) { const float d = (a[r * cs + i] + b[r * cs + i]) - mean; v = __builtin_fmaf(d, d, v); }
        const float rstd = 1.0f / sqrtf(sf_sum16(v) / (float)D + 1e-5f);
        if (r0 + grp < rows)
            for (int i = sub; i < D; i += 16) out[r * cs + i] = ((a[r * cs + i] + b[r * cs + i]) - mean) * rstd * n.g[i] + n.b[i];
    }
}

struct SfBufs { float *tok, *src, *tgt, *qkv, *att, *tmp, *ffb, *sc; };

// B.att <- softmax(q k^T * scale) v per window and head; q from x, k / v from kvsrc; all windows of the group, no mask
__device__ void sf_attn_core(const SfParams& p, const SfBufs& B, const float* x, const float* kvsrc, const SfAttn& at, int nwin, int ncm) {
    const int D = p.D, rows = nwin * p.ntok, hd = D / p.heads, nt = p.ntok;
    sf_linear(x, p.csD, D, B.qkv, p.csQ, D, at.q, rows, 0, ncm);
    sf_linear(kvsrc, p.csD, D, B.qkv + D, p.csQ, 2 * D, at.kv, rows, 0, ncm);
    __syncthreads();
    const int cq = p.csQ;
    for (int it = threadIdx.x; it < nwin * p.heads * nt * nt; it += blockDim.x) {
        const int kj = it % nt, qi = (it / nt) % nt, h = (it / (nt * nt)) % p.heads, w = it / (nt * nt * p.heads);
        const float* qv = B.qkv + (w * nt + qi) * cq + h * hd;
        const float* kv = B.qkv + (w * nt + kj) * cq + D + h * hd;
        float s = 0.f;
        for (int d = 0; d < hd; ++d) s = __builtin_fmaf(qv[d], kv[d], s);
        B.sc[it] = s * p.att_scale;
    }
    __syncthreads();
    for (int it = threadIdx.x; it < nwin * p.heads * nt; it += blockDim.x) {
        float* s = B.sc + it * nt;
        float m = s[0];
        for (int k = 1; k < nt; ++k) m = __builtin_fmaxf(m, s[k]);
        float sum = 0.f;
        for (int k = 0; k < nt; ++k) { s[k] = det_expf(s[k] - m); sum += s[k]; }
        for (int k = 0; k < nt; ++k) s[k] = s[k] / sum;
    }
    __syncthreads();
    for (int it = threadIdx.x; it < rows * D; it += blockDim.x) {
        const int r = it / D, f = it - r * D, w = r / nt, qi = r - w * nt, h = f / hd;
        const float* pr = B.sc + ((w * p.heads + h) * nt + qi) * nt;
        float o = 0.f;
        for (int k = 0; k < nt; ++k) o = __builtin_fmaf(pr[k], B.qkv[(w * nt + k) * cq + 2 * D + f], o);
        B.att[r * p.csD + f] = o;
    }
    __syncthreads();
}

// x <- LayerNorm(x + out_proj(attention)): the post-norm form of variant 1
__device__ void sf_attention(const SfParams& p, const SfBufs& B, float* x, const float* kvsrc, const SfAttn& at, SfNorm nrm, int nwin) {
    const int D = p.D, rows = nwin * p.ntok;
    sf_attn_core(p, B, x, kvsrc, at, nwin, 0);
    sf_linear(B.att, p.csD, D, B.tmp, p.csD, D, at.out, rows, 0);
    __syncthreads();
    sf_add_norm(x, B.tmp, x, p.csD, D, rows, nrm);
    __syncthreads();
}

__device__ void sf_ffn(const SfParams& p, const SfBufs& B, float* x, SfLin f1, SfLin f2, SfNorm nrm, int rows) {
    sf_linear(x, p.csD, p.D, B.ffb, p.csF, p.ff, f1, rows, MM_RELU);
    __syncthreads();
    sf_linear(B.ffb, p.csF, p.ff, B.tmp, p.csD, p.D, f2, rows, 0);
    __syncthreads();
    sf_add_norm(x, B.tmp, x, p.csD, p.D, rows, nrm);
    __syncthreads();
}

// the tokenizer both variants share: bn_input and the four ST-GCN blocks for windows w0 .. w0 + nwin - 1, everything in LDS;
// -> the region that holds the tokens as [win][tok][v][c < L] rows of csH floats
__device__ __forceinline__ float* sf_tokenizer(const SfParams& p, const float* __restrict__ windows, int w0, int nwin, float* lds) {
    const int V = p.V, T = p.T, H = p.H, TV = T * V;
    float* xin = lds + p.offXin;       // [win][t][v][2] after bn_input
    float* ax = lds + p.offAx;         // A . xin
    float* P = lds + p.offP;
    float* Q = lds + p.offQ;

    // ---- input: [win][2][T][V] -> bn_input -> [win][t][v][2]
    for (int it = threadIdx.x; it < nwin * 2 * TV; it += blockDim.x) {
        const int w = it / (2 * TV), rem = it - w * 2 * TV, c = rem / TV, tv = rem - c * TV, v = tv % V;
        xin[(w * TV + tv) * 2 + c] = __builtin_fmaf(windows[(size_t)(w0 + w) * 2 * TV + rem], p.in_scale[c * V + v], p.in_shift[c * V + v]);
    }
    __syncthreads();
    for (int it = threadIdx.x; it < nwin * 2 * TV; it += blockDim.x) {
        const int c = it & 1, row = it >> 1, v = row % V, fr = row - v;
        float o = 0.f;
        for (int e = 0; e < p.nnz; ++e) o = __builtin_fmaf(p.adj_val[v * p.nnz + e], xin[(fr + (int)p.adj_col[v * p.nnz + e]) * 2 + c], o);
        ax[it] = o;
    }
    // ---- block 0: residual 1x1 (2 -> H, stride s0) into P, then the temporal conv accumulates on top of it
    {
        const int T1 = p.Tn[1], h4 = H >> 2;
        for (int it = threadIdx.x; it < nwin * T1 * V * h4; it += blockDim.x) {
            const int c0 = (it % h4) * 4, row = it / h4, v = row % V, t = (row / V) % T1, w = row / (V * T1);
            const float2 x = *reinterpret_cast<const float2*>(xin + ((w * T + t * p.s[0]) * V + v) * 2);
            f32x4 r;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const float2 wv = *reinterpret_cast<const float2*>(p.blk[0].rw + (c0 + s) * 2);
                r[s] = __builtin_fmaf(x.y, wv.y, __builtin_fmaf(x.x, wv.x, 0.f)) + p.blk[0].rb[c0 + s];
            }
            *reinterpret_cast<f32x4*>(P + row * p.csH + c0) = r;
        }
        __syncthreads();
        Mm a{};
        a.in = ax; a.in_cs = 2; a.K = H; a.out = P; a.out_cs = p.csH; a.N = H; a.w = p.blk[0].tw; a.bias = p.blk[0].tb;
        a.ntaps = 9; a.stride = p.s[0]; a.pad = 4; a.V = V; a.R = nwin * V; a.in_w = TV; a.out_w = T1 * V; a.Tin = T; a.Tout = T1;
        a.flags = MM_RELU | MM_ACC_INIT | MM_FIRST; a.w0 = p.blk[0].gw; a.b0 = p.blk[0].gb;
        sf_mm(a);
        __syncthreads();
    }
    // ---- blocks 1..3: X in `cur`, result in `oth`
    float *cur = P, *oth = Q;
    for (int b = 1; b < 4; ++b) {
        const int Ti = p.Tn[b], To = p.Tn[b + 1], Co = b == 3 ? p.L : H;
        const SfBlock& k = p.blk[b];
        if (k.rw) {
            Mm a{};
            a.in = cur; a.in_cs = p.csH; a.K = H; a.out = oth; a.out_cs = p.csH; a.N = Co; a.w = k.rw; a.bias = k.rb;
            a.ntaps = 1; a.stride = p.s[b]; a.pad = 0; a.V = V; a.R = nwin * V; a.in_w = Ti * V; a.out_w = To * V; a.Tin = Ti; a.Tout = To;
            sf_mm(a);
        } else {
            for (int it = threadIdx.x; it < nwin * Ti * V * (H >> 2); it += blockDim.x) {
                const int row = it / (H >> 2), c0 = (it - row * (H >> 2)) * 4;
                *reinterpret_cast<f32x4*>(oth + row * p.csH + c0) = *reinterpret_cast<const f32x4*>(cur + row * p.csH + c0);
            }
        }
        __syncthreads();
        sf_adj_inplace(cur, p.csH, H, nwin * Ti, V, p.nnz, p.adj_col, p.adj_val);
        __syncthreads();
        sf_linear(cur, p.csH, H, cur, p.csH, Co, SfLin{k.gw, k.gb}, nwin * Ti * V, MM_RELU);        // in place: one job owns its rows
        __syncthreads();
        Mm a{};
        a.in = cur; a.in_cs = p.csH; a.K = Co; a.out = oth; a.out_cs = p.csH; a.N = Co; a.w = k.tw; a.bias = k.tb;
        a.ntaps = 9; a.stride = p.s[b]; a.pad = 4; a.V = V; a.R = nwin * V; a.in_w = Ti * V; a.out_w = To * V; a.Tin = Ti; a.Tout = To;
        a.flags = MM_RELU | MM_ACC_INIT;
        sf_mm(a);
        __syncthreads();
        float* t = cur; cur = oth; oth = t;
    }
    return cur;
}

__global__ __launch_bounds__(SF_THREADS) void shopformer_kernel(const SfParams* __restrict__ pp, const float* __restrict__ windows, int n,
                                                                 float* __restrict__ scores, float* __restrict__ tokens, float* __restrict__ recon) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const SfParams& p = *pp;              // device memory, uniform: scalar loads, no private copy of the per-layer tables
    const int w0 = blockIdx.x * p.G, nwin = min(p.G, n - w0);
    if (nwin <= 0) return;
    const int V = p.V;
    float* P = lds + p.offP;
    const float* cur = sf_tokenizer(p, windows, w0, nwin, lds);
    // ---- tokens: cur = Q holds [win][tok][v][c < L]; the transformer's buffers take over P
    const int D = p.D, nt = p.ntok, rows = nwin * nt, rowsG = p.G * nt;
    SfBufs B;
    B.tok = P; B.src = B.tok + rowsG * p.csD; B.tgt = B.src + rowsG * p.csD; B.att = B.tgt + rowsG * p.csD; B.tmp = B.att + rowsG * p.csD;
    B.qkv = B.tmp + rowsG * p.csD; B.ffb = B.qkv + rowsG * (p.csQ); B.sc = B.ffb + rowsG * p.csF;
    for (int it = threadIdx.x; it < rows * D; it += blockDim.x) {
        const int r = it / D, f = it - r * D, c = f / V, v = f - c * V, t = r % nt;
        const float tk = cur[(r * V + v) * p.csH + c];
        B.tok[r * p.csD + f] = tk;
        B.src[r * p.csD + f] = tk + p.pe_in[t * D + f];
        B.tgt[r * p.csD + f] = (t == 0 ? 0.f : cur[((r - 1) * V + v) * p.csH + c]) + p.pe_in[t * D + f];
        if (tokens) tokens[((size_t)w0 * nt + r) * D + f] = tk;
    }
    __syncthreads();
    for (int e = 0; e < p.layers; ++e) {
        sf_attention(p, B, B.src, B.src, p.enc[e].sa, p.enc[e].n1, nwin);
        sf_ffn(p, B, B.src, p.enc[e].f1, p.enc[e].f2, p.enc[e].n2, rows);
    }
    for (int e = 0; e < p.layers; ++e) {
        sf_attention(p, B, B.tgt, B.tgt, p.dec[e].sa, p.dec[e].n1, nwin);
        sf_attention(p, B, B.tgt, B.src, p.dec[e].ca, p.dec[e].n2, nwin);
        sf_ffn(p, B, B.tgt, p.dec[e].f1, p.dec[e].f2, p.dec[e].n3, rows);
    }
    sf_linear(B.tgt, p.csD, D, B.tmp, p.csD, D, p.proj, rows, 0);
    __syncthreads();
    // ---- score: mean over (token, feature) of (reconstructed - (token + PE))^2, 16 lanes per window
    if (recon)
        for (int it = threadIdx.x; it < rows * D; it += blockDim.x) recon[((size_t)w0 * nt + it / D) * D + it % D] = B.tmp[(it / D) * p.csD + it % D];
    const int sub = threadIdx.x & 15, grp = threadIdx.x >> 4;
    if (grp < p.G) {                                               // G <= 32 groups of 16 lanes; whole groups take the branch together
        const int w = min(grp, nwin - 1);
        float s = 0.f;
        for (int i = sub; i < nt * D; i += 16) {
            const int t = i / D, f = i - t * D, r = w * nt + t;
            const float d = B.tmp[r * p.csD + f] - (B.tok[r * p.csD + f] + p.pe_score[t * D + f]);
            s = __builtin_fmaf(d, d, s);
        }
        s = sf_sum16(s) / (float)(nt * D);
        if (sub == 0 && grp < nwin) scores[w0 + grp] = s;
    }
}

// ================================================================================================ variant 2
// launch 1: the tokenizer alone; tokens [n][ntok][Din] go to HBM
__global__ __launch_bounds__(SF_THREADS) void shopformer2_tok_kernel(const SfParams* __restrict__ pp, const float* __restrict__ windows, int n,
                                                                      float* __restrict__ tokens) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const SfParams& p = *pp;
    const int w0 = blockIdx.x * p.G, nwin = min(p.G, n - w0);
    if (nwin <= 0) return;
    const float* cur = sf_tokenizer(p, windows, w0, nwin, lds);
    const int V = p.V, Din = p.Din, rows = nwin * p.ntok;
    for (int it = threadIdx.x; it < rows * Din; it += blockDim.x) {
        const int r = it / Din, f = it - r * Din, c = f / V, v = f - c * V;
        tokens[((size_t)w0 * p.ntok + r) * Din + f] = cur[(r * V + v) * p.csH + c];
    }
}

// out[r] = LayerNorm(a[r]) * g + beta, 16 lanes per row: the pre-norm form has the norm alone
__device__ void sf_norm(const float* a, float* out, int cs, int D, int rows, SfNorm n) {
    const int sub = threadIdx.x & 15, grp = threadIdx.x >> 4, ngrp = blockDim.x >> 4;
    for (int r0 = 0; r0 < rows; r0 += ngrp) {                       // uniform trip count: the shuffles need every lane
        const int r = min(r0 + grp, rows - 1);
        float s = 0.f;
        for (int i = sub; i < D; i += 16) s += a[r * cs + i];
        const float mean = sf_sum16(s) / (float)D;
        float v = 0.f;
        for (int i = sub; i < D; i += 16) { const float d = a[r * cs + i] - mean; v = __builtin_fmaf(d, d, v); }
        const float rstd = 1.0f / sqrtf(sf_sum16(v) / (float)D + 1e-5f);
        if (r0 + grp < rows)
            for (int i = sub; i < D; i += 16) out[r * cs + i] = (a[r * cs + i] - mean) * rstd * n.g[i] + n.b[i];
    }
}

// output tiles per job for a layer of N features on `rows` rows: the fewest jobs that still give every wave one (bits do not depend on it)
__device__ __forceinline__ int sf_ncm(int N, int rows, int nwaves) {
    const int nct = (N + 15) >> 4, mpairs = (((rows + 15) >> 4) + 1) >> 1;
    if (((nct + 3) >> 2) * mpairs >= nwaves) return 4;
    if (((nct + 1) >> 1) * mpairs >= nwaves) return 2;
    return 1;
}

// x <- x + out_proj(attention(q from LayerNorm(x), k / v from kv (or from that same LayerNorm(x) when kv == nullptr)))
__device__ void sf_attention_pre(const SfParams& p, const SfBufs& B, float* x, float* nb, const float* kv, const SfAttn& at, SfNorm nrm, int nwin) {
    const int D = p.D, rows = nwin * p.ntok, nw = blockDim.x >> 6;
    sf_norm(x, nb, p.csD, D, rows, nrm);
    __syncthreads();
    sf_attn_core(p, B, nb, kv ? kv : nb, at, nwin, sf_ncm(D, rows, nw));
    sf_linear(B.att, p.csD, D, x, p.csD, D, at.out, rows, MM_ACC_INIT, sf_ncm(D, rows, nw));      // the residual add: x starts the chain
    __syncthreads();
}

// x <- x + linear2(gelu(linear1(LayerNorm(x))))
__device__ void sf_ffn_pre(const SfParams& p, float* x, float* nb, float* ffb, SfLin f1, SfLin f2, SfNorm nrm, int rows) {
    const int nw = blockDim.x >> 6;
    sf_norm(x, nb, p.csD, p.D, rows, nrm);
    __syncthreads();
    sf_linear(nb, p.csD, p.D, ffb, p.csF, p.ff, f1, rows, MM_GELU, sf_ncm(p.ff, rows, nw));
    __syncthreads();
    sf_linear(ffb, p.csF, p.ff, x, p.csD, p.D, f2, rows, MM_ACC_INIT, sf_ncm(p.D, rows, nw));
    __syncthreads();
}

// launch 2: the transformer on the tokens of GT windows per workgroup (GT * ntok rows: with GT = 16 two full 16-row MFMA tiles), the
// reconstruction and the scores.  Pre-norm layers, final norms, decoder fed from the encoder's own input, score without PE.
__global__ __launch_bounds__(SF_THREADS) void shopformer2_tf_kernel(const SfParams* __restrict__ pp, const float* __restrict__ tokens, int n,
                                                                     float* __restrict__ scores, float* __restrict__ token_scores,
                                                                     float* __restrict__ recon) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const SfParams& p = *pp;
    const int w0 = blockIdx.x * p.GT, nwin = min(p.GT, n - w0);
    if (nwin <= 0) return;
    const int D = p.D, Din = p.Din, nt = p.ntok, rows = nwin * nt, rowsG = p.GT * nt, cs = p.csD, nw = blockDim.x >> 6;
    float *tgt = lds + p.offTgt, *x = lds + p.offX, *nb = lds + p.offNb;
    SfBufs B{};
    B.qkv = lds + p.offU; B.att = B.qkv + rowsG * p.csQ; B.ffb = lds + p.offU; B.sc = lds + p.offSc;   // qkv + att and ffb are never live together
    const float* tk = tokens + (size_t)w0 * nt * Din;
    // ---- x0 = input_projection(tokens) + PE: the encoder works on a copy (x), the decoder on x0 itself (tgt)
    for (int it = threadIdx.x; it < rows * Din; it += blockDim.x) nb[(it / Din) * cs + it % Din] = tk[it];
    __syncthreads();
    if (p.in_proj) {
        sf_linear(nb, cs, Din, tgt, cs, D, p.inp, rows, 0, sf_ncm(D, rows, nw));
        __syncthreads();
    }
    for (int it = threadIdx.x; it < rows * D; it += blockDim.x) {
        const int r = it / D, f = it - r * D;
        const float v = (p.in_proj ? tgt[r * cs + f] : nb[r * cs + f]) + p.pe_in[(r % nt) * D + f];
        tgt[r * cs + f] = v;
        x[r * cs + f] = v;
    }
    __syncthreads();
    for (int e = 0; e < p.layers; ++e) {
        sf_attention_pre(p, B, x, nb, nullptr, p.enc[e].sa, p.enc[e].n1, nwin);
        sf_ffn_pre(p, x, nb, B.ffb, p.enc[e].f1, p.enc[e].f2, p.enc[e].n2, rows);
    }
    sf_norm(x, x, cs, D, rows, p.en);                              // memory; a 16-lane group owns its row
    __syncthreads();
    for (int e = 0; e < p.layers; ++e) {
        sf_attention_pre(p, B, tgt, nb, nullptr, p.dec[e].sa, p.dec[e].n1, nwin);
        sf_attention_pre(p, B, tgt, nb, x, p.dec[e].ca, p.dec[e].n2, nwin);
        sf_ffn_pre(p, tgt, nb, B.ffb, p.dec[e].f1, p.dec[e].f2, p.dec[e].n3, rows);
    }
    sf_norm(tgt, nb, cs, D, rows, p.dn);
    __syncthreads();
    const float* rec = nb;
    if (p.out_proj) {
        sf_linear(nb, cs, D, x, cs, Din, p.outp, rows, 0, sf_ncm(Din, rows, nw));
        __syncthreads();
        rec = x;
    }
    if (recon)
        for (int it = threadIdx.x; it < rows * Din; it += blockDim.x) recon[((size_t)w0 * nt + it / Din) * Din + it % Din] = rec[(it / Din) * cs + it % Din];
    // ---- scores: mean over features of (token - reconstruction)^2 per token, and over tokens too per window; 16 lanes per window
    const int sub = threadIdx.x & 15, grp = threadIdx.x >> 4;
    if (grp < p.GT) {                                              // GT <= 32 groups of 16 lanes; whole groups take the branch together
        const int w = min(grp, nwin - 1);
        float tot = 0.f;
        for (int t = 0; t < nt; ++t) {
            const int r = w * nt + t;
            float s = 0.f;
            for (int f = sub; f < Din; f += 16) { const float d = tk[r * Din + f] - rec[r * cs + f]; s = __builtin_fmaf(d, d, s); }
            s = sf_sum16(s);
            tot += s;
            if (token_scores && sub == 0 && grp < nwin) token_scores[(size_t)(w0 + grp) * nt + t] = s / (float)Din;
        }
        if (scores && sub == 0 && grp < nwin) scores[w0 + grp] = tot / (float)(nt * Din);
    }
}

}  // namespace

const char* prepare_shopformer_device() {
    hipError_t e = hipFuncSetAttribute((const void*)shopformer_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, SF_LDS_BYTES);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)shopformer2_tok_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, SF_LDS_BYTES);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)shopformer2_tf_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, SF_LDS_BYTES);
    return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

const char* launch_shopformer2(const SfParams* p_dev, int group, int group_tf, int lds_tok, int lds_tf, const float* windows, int n,
                               float* tokens, float* scores, float* token_scores, float* recon, hipStream_t stream, long long* launches) {
    hipLaunchKernelGGL(shopformer2_tok_kernel, dim3((n + group - 1) / group), dim3(SF_THREADS), lds_tok, stream, p_dev, windows, n, tokens);
    ++*launches;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hipGetErrorString(e);
    hipLaunchKernelGGL(shopformer2_tf_kernel, dim3((n + group_tf - 1) / group_tf), dim3(SF_THREADS), lds_tf, stream, p_dev, tokens, n, scores,
                       token_scores, recon);
    ++*launches;
    e = hipGetLastError();
    return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

const char* launch_shopformer(const SfParams* p_dev, int group, const float* windows, int n, float* scores, float* tokens, float* recon,
                              hipStream_t stream, long long* launches) {
    const int groups = (n + group - 1) / group;
    hipLaunchKernelGGL(shopformer_kernel, dim3(groups), dim3(SF_THREADS), SF_LDS_BYTES, stream, p_dev, windows, n, scores, tokens, recon);
    ++*launches;                                                   // the handle's launch counter (mi355_shopformer_info: launches)
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

}  // namespace mi355
