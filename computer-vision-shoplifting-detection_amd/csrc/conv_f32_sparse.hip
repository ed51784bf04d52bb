// The Detect box branch at the anchors that reach NMS only (fp32 engine).
//
// predict() returns post-NMS rows, and NMS selects its candidates from best[] (class scores) alone, so the box of an anchor is
// needed only where the best class score clears conf.  Per pass: the class branch and the score stage run densely as before, then
//   sparse_lists_kernel   per level: the candidate positions and their 3x3 dilation, compacted (counts on the device)
//   sparse_conv_a_kernel  cv2.i.0 (3x3 over the neck map) + bias + SiLU at the dilated positions -> their own pixels of the
//                         slice the dense launch writes
//   sparse_conv_b_kernel  cv2.i.1 (3x3 over stage A's pixels) + SiLU, cv2.i.2 (1x1) from registers, DFL + dist2bbox + stride
//                         -> the anchor's own slot of `pred`
// Every output is computed in the canonical order of conv_f32.h (per 16-channel block ONE fma chain over taps kh-major, MFMA
// step, k-group, started from +0; block partials added in ascending order; out-of-image taps are MFMAs on exact zeros), on the
// same v_mfma_f32_16x16x4_f32 operand layout, so the bits are those of the dense launches.  When a list would overflow its
// capacity the flag state[8] is raised: the sparse kernels then leave at once and the gated dense launches run instead.
#include "conv_f32.h"        // act4 (the conv epilogues' activation), f32x4
#include <algorithm>

#pragma clang fp contract(off)

namespace mi355 {

// wave-aggregated append: one atomic per wave and list
__device__ __forceinline__ void sp_append(bool flag, int* list, int cap, int* count, int* overflow, int v) {
    const unsigned long long m = __ballot(flag);
    if (m == 0ull) return;
    const int lane = threadIdx.x & 63, leader = __ffsll((long long)m) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(count, __popcll(m));
    base = __shfl(base, leader);
    const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
    if (flag) {
        if (pos < cap) list[pos] = v;
        else *overflow = 1;
    }
}

__global__ __launch_bounds__(256) void sparse_lists_kernel(SparseArgs a) {
    const int b = blockIdx.y, an = blockIdx.x * 256 + threadIdx.x;
    const bool live = an < a.A;
    int l = 0;
#pragma unroll
    for (int j = 1; j < 3; ++j)
        if (j < a.n_levels && an >= a.lv[j].anchor0) l = j;
    const int H = a.lv[l].H, W = a.lv[l].W, a0 = a.lv[l].anchor0;
    bool cand = false, dil = false;
    const int li = live ? an - a0 : 0;
    if (live) {
        const int y = li / W, x = li - y * W;
        const float2* best = a.best + (size_t)b * a.A + a0;
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const int yy = y + dy, xx = x + dx;
                if ((unsigned)yy >= (unsigned)H || (unsigned)xx >= (unsigned)W) continue;
                const float2 bc = best[yy * W + xx];
                bool ok = bc.x > a.conf;                              // nms_collect's predicate
                if (ok && a.class_mask) { const int c = (int)bc.y; ok = (a.class_mask[c >> 5] >> (c & 31)) & 1u; }
                dil |= ok;
                if (dy == 0 && dx == 0) cand = ok;
            }
    }
    const int v = b * H * W + li;
    for (int j = 0; j < a.n_levels; ++j) {
        sp_append(dil && l == j, a.lv[j].dil, a.lv[j].cap_dil, a.state + j, a.state + 8, v);
        sp_append(cand && l == j, a.lv[j].cand, a.lv[j].cap_cand, a.state + 4 + j, a.state + 8, v);
    }
}

// one 3x3 conv over 16 gathered positions x 64 couts (4 cout tiles) for ONE wave: tot[ct] = canonical sum, no bias yet.
// lane (p = lane & 15, g = lane >> 4) fetches, per tap and 16-channel block, the 16 bytes of channels 16 cb + 4 g .. + 3 of its
// position's tap pixel straight from the NHWC map (the MFMA B-operand layout); weights come in packed fragment order.
// Every wave re-reads the conv's 9 * cib * 4 KiB of weight fragments (L2 hits) for its 16 positions: a third or less of the dense
// kernels' efficiency, which the break-even share of positions allows for; not tuned further.
__device__ __forceinline__ void sp_conv3x3_64(const float* map, int cs, int cib, int H, int W, int b, int y, int x, const float* wpk,
                                              int lane, f32x4 (&tot)[4]) {
    const int g = lane >> 4;
    const float* base = map + (size_t)b * H * W * cs + 4 * g;
    int off[9]; bool inb[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
        inb[k] = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
        off[k] = inb[k] ? (yy * W + xx) * cs : 0;
    }
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) tot[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const float* wl = wpk + lane * 4;
    const size_t wct = (size_t)9 * cib * 256;
    for (int cb = 0; cb < cib; ++cb) {
        f32x4 xv[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            xv[k] = *(const f32x4*)(base + off[k] + 16 * cb);
            if (!inb[k]) xv[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        f32x4 acc[4];
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            f32x4 w[4];
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) w[ct] = *(const f32x4*)(wl + ct * wct + ((size_t)k * cib + cb) * 256);
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int ct = 0; ct < 4; ++ct)
                    acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[ct][s], xv[k][s], (k == 0 && s == 0) ? (f32x4){0.f, 0.f, 0.f, 0.f} : acc[ct], 0, 0, 0);
        }
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) tot[ct] += acc[ct];
    }
}

// the wave's 16 list entries: lane p's entry (clamped to the list's last one; `ok` says whether it is the lane's own)
__device__ __forceinline__ int sp_entry(const int* list, int n, int t0, int lane, bool* ok) {
    const int e = t0 + (lane & 15);
    *ok = e < n;
    return list[e < n ? e : n - 1];
}

__global__ __launch_bounds__(256) void sparse_conv_a_kernel(SparseArgs a) {
    if (a.state[8]) return;
    const int l = blockIdx.y;
    const SparseLevel& L = a.lv[l];
    const int n = min(a.state[l], L.cap_dil);
    if ((int)blockIdx.x * 64 >= n) return;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int t0 = (blockIdx.x * 4 + wave) * 16;
    if (t0 >= n) return;
    bool ok;
    const int v = sp_entry(L.dil, n, t0, lane, &ok);
    const int HW = L.H * L.W, b = v / HW, li = v - b * HW, y = li / L.W, x = li - y * L.W;
    f32x4 tot[4];
    sp_conv3x3_64(L.src, L.src_cs, L.cib, L.H, L.W, b, y, x, L.wA, lane, tot);
    if (!ok) return;
    float* dst = L.mid + (size_t)v * L.mid_cs + (lane >> 4) * 4;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
        f32x4 r = tot[ct] + *(const f32x4*)(L.biasA + ct * 16 + (lane >> 4) * 4);
        r = act4(r, a.act);
        *(f32x4*)(dst + ct * 16) = r;
    }
}

constexpr int SP_LDP = 68;      // floats per position of the logits image in LDS (64 + 4: the 16-byte rows of a quad land in different banks)

__global__ __launch_bounds__(256) void sparse_conv_b_kernel(SparseArgs a) {
    __shared__ __attribute__((aligned(16))) float logits[4][16 * SP_LDP];
    if (a.state[8]) return;
    const int l = blockIdx.y;
    const SparseLevel& L = a.lv[l];
    const int n = min(a.state[4 + l], L.cap_cand);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4, p = lane & 15;
    const int t0 = (blockIdx.x * 4 + wave) * 16;
    if (t0 >= n) return;                                     // waves are independent: each uses its own slice of `logits`, no block barrier
    bool ok;
    const int v = sp_entry(L.cand, n, t0, lane, &ok);
    const int HW = L.H * L.W, b = v / HW, li = v - b * HW, y = li / L.W, x = li - y * L.W;
    f32x4 tot[4];
    sp_conv3x3_64(L.mid, L.mid_cs, 4, L.H, L.W, b, y, x, L.wB, lane, tot);
    // cv2.i.1's output: the accumulator of lane (p, g) for cout tile ct holds channels 16 ct + 4 g .. + 3 of position p, which is
    // the B operand of k-block ct of the pointwise conv behind it
    f32x4 x2[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) x2[ct] = act4(tot[ct] + *(const f32x4*)(L.biasB + ct * 16 + g * 4), a.act);
    float* lg = logits[wave];
#pragma unroll
    for (int ct2 = 0; ct2 < 4; ++ct2) {
        f32x4 tot2 = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            const f32x4 w = *(const f32x4*)(L.wC + ((size_t)ct2 * 4 + cb) * 256 + lane * 4);
            f32x4 p2;
#pragma unroll
            for (int s = 0; s < 4; ++s)
                p2 = __builtin_amdgcn_mfma_f32_16x16x4f32(w[s], x2[cb][s], s == 0 ? (f32x4){0.f, 0.f, 0.f, 0.f} : p2, 0, 0, 0);
            tot2 += p2;
        }
        const f32x4 r = tot2 + *(const f32x4*)(L.biasC + ct2 * 16 + g * 4);
        *(f32x4*)(lg + p * SP_LDP + ct2 * 16 + g * 4) = r;
    }
    // the wave's own LDS writes are complete (and not reordered by the compiler) before its lanes read each other's rows
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    // lane (p, g) evaluates DFL side g of position p, as one lane of the dense decode kernel does
    float side[16];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const f32x4 q = *(const f32x4*)(lg + p * SP_LDP + 16 * g + 4 * j);
        side[4 * j] = q[0]; side[4 * j + 1] = q[1]; side[4 * j + 2] = q[2]; side[4 * j + 3] = q[3];
    }
    const float d = det_dfl_side(side);
    const float d0 = __shfl(d, p), d1 = __shfl(d, p + 16), d2 = __shfl(d, p + 32), d3 = __shfl(d, p + 48);
    if (ok && g == 0) {
        const float4 o = det_dist2bbox(d0, d1, d2, d3, (float)x + 0.5f, (float)y + 0.5f, (float)L.stride);
        float* out = a.pred + ((size_t)b * a.A + L.anchor0 + li) * a.no;
        if ((a.no & 3) == 0) *(float4*)out = o;
        else { out[0] = o.x; out[1] = o.y; out[2] = o.z; out[3] = o.w; }
    }
}

const char* launch_sparse_lists(const SparseArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(sparse_lists_kernel, dim3((unsigned)((a.A + 255) / 256), (unsigned)a.B), dim3(256), 0, st, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

const char* launch_sparse_box(const SparseArgs& a, hipStream_t st) {
    int cap_d = 0, cap_c = 0;
    for (int l = 0; l < a.n_levels; ++l) { cap_d = std::max(cap_d, a.lv[l].cap_dil); cap_c = std::max(cap_c, a.lv[l].cap_cand); }
    hipLaunchKernelGGL(sparse_conv_a_kernel, dim3((unsigned)((cap_d + 63) / 64), (unsigned)a.n_levels), dim3(256), 0, st, a);
    hipLaunchKernelGGL(sparse_conv_b_kernel, dim3((unsigned)((cap_c + 63) / 64), (unsigned)a.n_levels), dim3(256), 0, st, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

}  // namespace mi355
