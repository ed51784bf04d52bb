// Head decode (DFL + dist2bbox + sigmoid + keypoint decode) and non_max_suppression + scale-back.
//
// Restates, in the reference's own fp32 operation order (FP contraction is switched OFF in this file):
//   ultralytics/nn/modules/head.py:Detect._inference / Pose.kpts_decode, block.py:DFL, utils/tal.py:dist2bbox
//   ultralytics/utils/nms.py:non_max_suppression (+ torchvision.ops.nms CPU kernel: stable descending sort,
//   suppress IoU > thr, IoU = inter / (area_i + area_j - inter))
//   ultralytics/utils/ops.py:scale_boxes / clip_boxes / scale_coords / clip_coords
// reached from /root/reference/model.py:38-40.
#include "common.h"
#include "../../include/mi355_yolo.h"
#include "detmath.h"
#include <cstdlib>

#pragma clang fp contract(off)
#include "tile_merge.h"

namespace mi355 {

// ---------------------------------------------------------------------------------------------- decode
// Reads the raw head maps (NHWC, per level: 64 box logits | nc class logits | nk kpts) and writes, per anchor, the
// decoded row [4 box | nc scores | nk kpts] (anchor-major) plus (best score, best class).  FULL = also store the nc
// sigmoid scores (only the raw-head parity entry point needs them: NMS reads box, keypoints and `best` only), which cuts
// the kernel's HBM writes from 86 to 6 floats per anchor for an 80-class detector.
// FOUR lanes per anchor and no LDS.  Lane s of a quad owns DFL side s (its 16 logits are 64 contiguous bytes:
// four 16-byte loads), a quarter of the class logits and a quarter of the keypoint values; the four distances, the class
// maximum and the (score, first argmax) pair are combined with wave shuffles.  (Round 1's LDS-staged one-lane-per-anchor
// kernels staged 336 bytes per anchor and so ran at 1.5 waves per SIMD: 0.78 vs 0.36 ms per 256 frames; removed.)  A DFL
// side is evaluated sequentially by one lane in the canonical operation order.
// PART: 0 = the whole row; 1 = the score stage alone (classes -> best[], keypoints: what the candidate filter needs, no box);
// 2 = the box alone, and only when *a.gate != 0 (the dense fall-back of the sparse box branch: engine_run.hip).
template <bool FULL, int PART = 0>
__global__ __launch_bounds__(256) void decode_kernel_quad(DecodeArgs a) {
    if (PART == 2) {
        if (*a.gate == 0) return;
        if (blockIdx.x == 0 && threadIdx.x == 0 && a.fallback_count) atomicAdd(a.fallback_count, 1);
    }
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    const long total = (long)a.B * a.A;
    const long ag0 = gid >> 2;
    const int s = (int)(gid & 3);
    const bool live = ag0 < total;
    const long ag = live ? ag0 : total - 1;                 // dead quads shadow the last anchor (shuffles need all lanes), stores are guarded
    const int b = (int)(ag / a.A), an = (int)(ag - (long)b * a.A);
    int l = 0;
#pragma unroll
    for (int j = 1; j < 4; ++j)
        if (j < a.n_levels && an >= a.lv[j].anchor0) l = j;
    const HeadLevelArgs lv = a.lv[l];
    const int li = an - lv.anchor0;
    const int y = li / lv.W, x = li - y * lv.W;
    const float ax = (float)x + 0.5f, ay = (float)y + 0.5f, st = (float)lv.stride;
    const float* src = lv.buf + ((size_t)b * lv.H * lv.W + li) * lv.cs;
    const int nk = a.nkpt * a.kdim, no = 4 + a.nc + nk;
    float* out = a.pred + (size_t)ag * no;
    const int lane = threadIdx.x & 63, qbase = lane & ~3;

    // ---- box: side s
    if (PART != 1) {
        float v[16];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float4 q4 = *(const float4*)(src + lv.box_off + 16 * s + 4 * j);
            v[4 * j] = q4.x; v[4 * j + 1] = q4.y; v[4 * j + 2] = q4.z; v[4 * j + 3] = q4.w;
        }
        const float d = det_dfl_side(v);
        const float d0 = __shfl(d, qbase), d1 = __shfl(d, qbase + 1), d2 = __shfl(d, qbase + 2), d3 = __shfl(d, qbase + 3);
        if (live && s == 0) {
            const float4 o = det_dist2bbox(d0, d1, d2, d3, ax, ay, st);
            if ((no & 3) == 0) *(float4*)out = o;
            else { out[0] = o.x; out[1] = o.y; out[2] = o.z; out[3] = o.w; }
        }
    }
    if (PART == 2) return;
    // ---- classes: lane s owns classes c = s, s + 4, s + 8, ... (or whole float4 groups, below)
    {
        const float* cl = src + lv.cls_off;
        // 16-byte form when the class slice allows it: lane s owns the float4 groups s, s + 4, ... (classes 4q .. 4q+3)
        const bool vec = (a.nc & 3) == 0 && (lv.cls_off & 3) == 0;
        const int ncq = a.nc >> 2;
        float thr = -__builtin_huge_valf();
        // NMS only needs max_c sigmoid(logit_c) and its FIRST argmax.  sigmoid is monotone, so only classes whose logit is
        // within a hair of the largest one can hold or tie the maximum: evaluate the (35-instruction, bit-exact) sigmoid for
        // those alone -- 1-2 classes instead of 80.  The window is exact, not heuristic: up to 11 the fp32 sigmoid still
        // separates logits 0.01 apart by >= 2.8 ulp (det_expf is within 1.4 ulp of exp; tests/test_oracle_det.py checks the
        // property), beyond that it saturates towards 1.0f, so everything above 10.9 is a candidate; below -80 it
        // underflows and every class is one.
        if (!FULL) {
            float m = -__builtin_huge_valf();
            if (vec) {
                for (int q = s; q < ncq; q += 4) {
                    const float4 v = *(const float4*)(cl + 4 * q);
                    m = fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
                }
            } else {
                for (int c = s; c < a.nc; c += 4) m = fmaxf(m, cl[c]);
            }
            m = fmaxf(m, __shfl_xor(m, 1));
            m = fmaxf(m, __shfl_xor(m, 2));
            thr = m > 11.0f ? 10.9f : (m < -80.0f ? -__builtin_huge_valf() : m - 0.01f);
        }
        float best = -1.f; int bi = 0x7fffffff;
        if (vec) {
            for (int q = s; q < ncq; q += 4) {
                const float4 v = *(const float4*)(cl + 4 * q);
                float lg[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (FULL || lg[j] >= thr) {
                        lg[j] = det_sigmoid(lg[j]);
                        if (lg[j] > best) { best = lg[j]; bi = 4 * q + j; }
                    }
                }
                if (FULL && live) {
                    if ((no & 3) == 0) *(float4*)(out + 4 + 4 * q) = make_float4(lg[0], lg[1], lg[2], lg[3]);
                    else { out[4 + 4 * q] = lg[0]; out[5 + 4 * q] = lg[1]; out[6 + 4 * q] = lg[2]; out[7 + 4 * q] = lg[3]; }
                }
            }
        } else {
            for (int c = s; c < a.nc; c += 4) {
                const float lg = cl[c];
                if (FULL || lg >= thr) {
                    const float sc = det_sigmoid(lg);
                    if (FULL && live) out[4 + c] = sc;
                    if (sc > best) { best = sc; bi = c; }
                }
            }
        }
        // (max score, FIRST class that attains it) over the quad == the reference's ascending `>` scan
#pragma unroll
        for (int off = 1; off <= 2; off <<= 1) {
            const float ob = __shfl_xor(best, off);
            const int oi = __shfl_xor(bi, off);
            if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
        }
        if (bi == 0x7fffffff) bi = 0;                        // no score beat -1 (all NaN): the reference leaves class 0
        if (live && s == 0) a.best[ag] = make_float2(best, (float)bi);
    }
    // ---- keypoints: element e = s, s + 4, ... of the nk values; e = k * kdim + component
    if (nk) {
        const float* kp = src + lv.kpt_off;
        for (int e = s; e < nk; e += 4) {
            const int k = e / a.kdim, comp = e - k * a.kdim;
            float v = kp[e];
            if (comp == 0) v = (v * 2.0f + (ax - 0.5f)) * st;
            else if (comp == 1) v = (v * 2.0f + (ay - 0.5f)) * st;
            else if (a.kdim == 3) v = det_sigmoid(v);
            if (live) out[4 + a.nc + e] = v;
        }
    }
}

const char* launch_decode(const DecodeArgs& a, bool full, hipStream_t st, int part) {
    for (int l = 0; l < a.n_levels; ++l)
        if ((a.lv[l].cs & 3) || (a.lv[l].box_off & 3)) return "decode: box logits must be 16-byte aligned";
    if (part == 2 && !a.gate) return "decode: the gated box stage needs its gate";
    const long lanes = (long)a.B * a.A * 4;
    const dim3 g((unsigned)((lanes + 255) / 256));
    if (part == 1)      hipLaunchKernelGGL((decode_kernel_quad<false, 1>), g, dim3(256), 0, st, a);
    else if (part == 2) hipLaunchKernelGGL((decode_kernel_quad<false, 2>), g, dim3(256), 0, st, a);
    else if (full) hipLaunchKernelGGL(decode_kernel_quad<true>, g, dim3(256), 0, st, a);
    else      hipLaunchKernelGGL(decode_kernel_quad<false>, g, dim3(256), 0, st, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

// [B][rows][cols] -> [B][cols][rows]  (Ultralytics [B, no, A] <-> anchor-major [B, A, no])
__global__ void transpose_kernel(const float* in, float* out, int B, int rows, int cols) {
    const long total = (long)B * rows * cols;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % cols);
        const int r = (int)((i / cols) % rows);
        const int b = (int)(i / ((long)cols * rows));
        out[((size_t)b * cols + c) * rows + r] = in[i];
    }
}
const char* launch_transpose_pred(const float* in, float* out, int B, int rows, int cols, hipStream_t st) {
    const long total = (long)B * rows * cols;
    const unsigned grid = (unsigned)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    hipLaunchKernelGGL(transpose_kernel, dim3(grid), dim3(256), 0, st, in, out, B, rows, cols);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

__global__ void best_kernel(const float* pred, int B, int A, int no, int nc, float2* best) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * A) return;
    const float* p = pred + (size_t)i * no + 4;
    float bs = -1.f; int bi = 0;
    for (int c = 0; c < nc; ++c) if (p[c] > bs) { bs = p[c]; bi = c; }
    best[i] = make_float2(bs, (float)bi);
}
const char* launch_best_from_pred(const float* pred, int B, int A, int no, int nc, float2* best, hipStream_t st) {
    const long total = (long)B * A;
    hipLaunchKernelGGL(best_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, pred, B, A, no, nc, best);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

// ---------------------------------------------------------------------------------------------- NMS
// Kernel 1 (one 256-thread block per image): candidate filter (best score > conf, best class allowed),
// then a bitonic sort of the 64-bit keys (~score_bits << 32 | anchor): ascending key order == descending
// score with ties broken by ascending anchor index == torch's stable descending sort of the anchor-ordered
// candidate list.
__device__ void bitonic_sort(unsigned long long* v, int n2, int tid, int nthreads) {
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < n2; i += nthreads) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const unsigned long long a = v[i], b = v[ixj];
                    const bool up = (i & k) == 0;
                    if ((a > b) == up) { v[i] = b; v[ixj] = a; }
                }
            }
            __syncthreads();
        }
}

constexpr int NMS_LDS_KEYS = 4096;
constexpr int NMS_SORT_THREADS = 1024;

// compare-exchange steps j = j_hi, j_hi/2, .. 1 of merge stage k on the LDS-resident chunk [base, base + NMS_LDS_KEYS) of a
// longer sequence (directions follow the GLOBAL index)
__device__ void bitonic_steps_lds(unsigned long long* sk, int base, int k, int j_hi, int tid) {
    for (int j = j_hi; j > 0; j >>= 1) {
        for (int l = tid; l < NMS_LDS_KEYS; l += NMS_SORT_THREADS) {
            const int lxj = l ^ j;
            if (lxj > l) {
                const unsigned long long a = sk[l], b = sk[lxj];
                const bool up = ((base + l) & k) == 0;
                if ((a > b) == up) { sk[l] = b; sk[lxj] = a; }
            }
        }
        __syncthreads();
    }
}

// More candidates than fit in LDS (conf ~0.001 validation-style calls, or 1280x1280 inputs): the classic hybrid -- every
// compare-exchange at distance < NMS_LDS_KEYS runs on LDS-resident chunks, only the few long-distance steps of the last
// merge stages touch global memory (3 global round trips for 8192 keys instead of 91).
__device__ void bitonic_sort_hybrid(unsigned long long* keys, unsigned long long* sk, int n2, int tid) {
    constexpr int C = NMS_LDS_KEYS;
    for (int base = 0; base < n2; base += C) {                       // stages k = 2 .. C: chunk-local
        for (int l = tid; l < C; l += NMS_SORT_THREADS) sk[l] = keys[base + l];
        __syncthreads();
        for (int k = 2; k <= C; k <<= 1) bitonic_steps_lds(sk, base, k, k >> 1, tid);
        for (int l = tid; l < C; l += NMS_SORT_THREADS) keys[base + l] = sk[l];
        __syncthreads();
    }
    for (int k = 2 * C; k <= n2; k <<= 1) {
        for (int j = k >> 1; j >= C; j >>= 1) {                      // partners live in different chunks
            for (int i = tid; i < n2; i += NMS_SORT_THREADS) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const unsigned long long a = keys[i], b = keys[ixj];
                    const bool up = (i & k) == 0;
                    if ((a > b) == up) { keys[i] = b; keys[ixj] = a; }
                }
            }
            __syncthreads();
        }
        for (int base = 0; base < n2; base += C) {
            for (int l = tid; l < C; l += NMS_SORT_THREADS) sk[l] = keys[base + l];
            __syncthreads();
            bitonic_steps_lds(sk, base, k, C >> 1, tid);
            for (int l = tid; l < C; l += NMS_SORT_THREADS) keys[base + l] = sk[l];
            __syncthreads();
        }
    }
}

// candidate filter of one image: keys[0 .. n) = (~score bits, anchor index) of the anchors that pass conf / class mask, padded with
// ~0 up to the next power of two n2; returns n2 (block-uniform), *n_out = n
__device__ int nms_collect(const NmsArgs& a, int b, unsigned long long* keys, int* scount, int tid, int* n_out) {
    if (tid == 0) *scount = 0;
    __syncthreads();
    const float2* best = a.best + (size_t)b * a.A;
    for (int an = tid; an < a.A; an += NMS_SORT_THREADS) {
        const float2 bc = best[an];
        bool ok = bc.x > a.conf;
        if (ok && a.class_mask) { const int c = (int)bc.y; ok = (a.class_mask[c >> 5] >> (c & 31)) & 1u; }
        if (ok) {
            const int pos = atomicAdd(scount, 1);
            keys[pos] = ((unsigned long long)(~__float_as_uint(bc.x)) << 32) | (unsigned)an;
        }
    }
    __syncthreads();
    const int n = *scount;
    int n2 = 1;
    while (n2 < n) n2 <<= 1;
    for (int i = n + tid; i < n2; i += NMS_SORT_THREADS) keys[i] = ~0ull;
    __syncthreads();
    *n_out = n;
    return n2;
}

__global__ __launch_bounds__(NMS_SORT_THREADS) void nms_sort_kernel(NmsArgs a, int* cand_counts) {
    __shared__ unsigned long long skeys[NMS_LDS_KEYS];
    __shared__ int scount;
    const int b = blockIdx.x, tid = threadIdx.x;
    unsigned long long* keys = a.keys + (size_t)b * a.Apow2;
    int n = 0;
    const int n2 = nms_collect(a, b, keys, &scount, tid, &n);
    if (n2 > 1) {
        if (n2 <= NMS_LDS_KEYS) {
            for (int i = tid; i < n2; i += NMS_SORT_THREADS) skeys[i] = keys[i];
            __syncthreads();
            bitonic_sort(skeys, n2, tid, NMS_SORT_THREADS);
            for (int i = tid; i < n; i += NMS_SORT_THREADS) keys[i] = skeys[i];
        } else {
            bitonic_sort_hybrid(keys, skeys, n2, tid);
        }
    }
    if (tid == 0) cand_counts[b] = n < a.max_nms ? n : a.max_nms;     // "if n > max_nms: keep the top max_nms by conf"
}

// ---- the same sort spread over many blocks, for maps with more than 16384 anchors (1280x1280: 33,600 anchors, tens of thousands of
// candidates at low conf): one block per image sorting 32k keys took 0.68 ms per step, at any batch.  The bitonic network is cut into
// launches: collect (one block per image), chunk-local stages k <= 4096 (one block per 4096-key chunk, in LDS), then per merge stage
// k the few long-distance steps (j >= 4096, global memory, all chunks in parallel) and the LDS-resident rest (j < 4096).  Blocks
// beyond an image's padded length exit at once.  Keys are unique, so the result is the sequence the one-block sort gives.
__global__ __launch_bounds__(NMS_SORT_THREADS) void nms_collect_kernel(NmsArgs a, int* cand_counts, int* sort_len) {
    __shared__ int scount;
    const int b = blockIdx.x, tid = threadIdx.x;
    int n = 0;
    const int n2 = nms_collect(a, b, a.keys + (size_t)b * a.Apow2, &scount, tid, &n);
    if (tid == 0) { cand_counts[b] = n < a.max_nms ? n : a.max_nms; sort_len[b] = n2; }
}

__global__ __launch_bounds__(NMS_SORT_THREADS) void nms_chunk_sort_kernel(NmsArgs a, const int* sort_len, int chunks) {
    __shared__ unsigned long long sk[NMS_LDS_KEYS];
    const int b = blockIdx.x / chunks, base = (blockIdx.x % chunks) * NMS_LDS_KEYS, tid = threadIdx.x;
    const int n2 = sort_len[b];
    if (base >= n2 || n2 < 2) return;
    unsigned long long* keys = a.keys + (size_t)b * a.Apow2;
    const int len = n2 < NMS_LDS_KEYS ? n2 : NMS_LDS_KEYS;            // a short sequence is one (partial) chunk
    for (int l = tid; l < len; l += NMS_SORT_THREADS) sk[l] = keys[base + l];
    __syncthreads();
    for (int k = 2; k <= len; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int l = tid; l < len; l += NMS_SORT_THREADS) {
                const int lxj = l ^ j;
                if (lxj > l) {
                    const unsigned long long x = sk[l], y = sk[lxj];
                    const bool up = ((base + l) & k) == 0;
                    if ((x > y) == up) { sk[l] = y; sk[lxj] = x; }
                }
            }
            __syncthreads();
        }
    for (int l = tid; l < len; l += NMS_SORT_THREADS) keys[base + l] = sk[l];
}

__global__ __launch_bounds__(NMS_SORT_THREADS) void nms_global_step_kernel(NmsArgs a, const int* sort_len, int blocks_per_image, int k, int j) {
    const int b = blockIdx.x / blocks_per_image;
    const int n2 = sort_len[b];
    if (k > n2) return;
    unsigned long long* keys = a.keys + (size_t)b * a.Apow2;
    const int i = (blockIdx.x % blocks_per_image) * NMS_SORT_THREADS + threadIdx.x;       // one thread per lower partner
    // enumerate the indices whose bit j is clear: insert a 0 at bit position log2(j)
    const int lo = i & (j - 1), idx = ((i - lo) << 1) | lo;
    if (idx >= n2) return;
    const unsigned long long x = keys[idx], y = keys[idx | j];
    const bool up = (idx & k) == 0;
    if ((x > y) == up) { keys[idx] = y; keys[idx | j] = x; }
}

__global__ __launch_bounds__(NMS_SORT_THREADS) void nms_lds_steps_kernel(NmsArgs a, const int* sort_len, int chunks, int k) {
    __shared__ unsigned long long sk[NMS_LDS_KEYS];
    const int b = blockIdx.x / chunks, base = (blockIdx.x % chunks) * NMS_LDS_KEYS, tid = threadIdx.x;
    const int n2 = sort_len[b];
    if (k > n2 || base >= n2) return;
    unsigned long long* keys = a.keys + (size_t)b * a.Apow2;
    for (int l = tid; l < NMS_LDS_KEYS; l += NMS_SORT_THREADS) sk[l] = keys[base + l];
    __syncthreads();
    bitonic_steps_lds(sk, base, k, NMS_LDS_KEYS >> 1, tid);
    for (int l = tid; l < NMS_LDS_KEYS; l += NMS_SORT_THREADS) keys[base + l] = sk[l];
}

// Kernel 2 (one block of NMS_WAVES waves per image): greedy suppression over the sorted candidates in chunks of 64, stopping
// at max_det kept boxes, then scale-back and row packing.  The test of a chunk against the boxes kept so far -- the bulk of
// the work: candidates x kept IoUs, each with an IEEE division -- is split over the waves (wave w takes kept boxes w,
// w + NMS_WAVES, ...; the survivor masks are AND-ed through LDS); the greedy pass inside the chunk is inherently serial and is
// run redundantly by every wave, which keeps the kept count uniform without a broadcast.  Decisions are those of the
// sequential algorithm (torchvision.ops.nms order): a candidate dies iff some earlier kept box overlaps it.
constexpr int NMS_MAX_DET = 1024;
constexpr int NMS_WAVES = 8;

struct CandBox { float x1, y1, x2, y2, area; };

__device__ __forceinline__ bool iou_gt(const CandBox& i, const CandBox& j, float thr) {
    const float xx1 = fmaxf(i.x1, j.x1), yy1 = fmaxf(i.y1, j.y1);
    const float xx2 = fminf(i.x2, j.x2), yy2 = fminf(i.y2, j.y2);
    const float w = fmaxf(0.f, xx2 - xx1), h = fmaxf(0.f, yy2 - yy1);
    const float inter = w * h;
    const float ovr = inter / (i.area + j.area - inter);
    return ovr > thr;
}

// WAVES = waves of the block running it (NMS_WAVES stand-alone; the sort kernel's 16 when it runs behind the sort in one launch)
template <int WAVES>
__device__ __forceinline__ void nms_greedy_body(const NmsArgs& a, const int b, const int n) {
    constexpr int NMS_WAVES = WAVES;
    __shared__ float kx1[NMS_MAX_DET], ky1[NMS_MAX_DET], kx2[NMS_MAX_DET], ky2[NMS_MAX_DET], kar[NMS_MAX_DET];
    __shared__ int kan[NMS_MAX_DET];
    __shared__ unsigned long long survive[2][NMS_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long* keys = a.keys + (size_t)b * a.Apow2;
    const float* pred = a.pred + (size_t)b * a.A * a.no;
    const float2* best = a.best + (size_t)b * a.A;
    int nk = 0, it = 0;
    for (int base = 0; base < n && nk < a.max_det; base += 64, ++it) {
        const int j = base + lane;
        const bool valid = j < n;
        int an = 0;
        CandBox me = {0.f, 0.f, 0.f, 0.f, 0.f};
        if (valid) {
            an = (int)(keys[j] & 0xffffffffull);
            const float* p = pred + (size_t)an * a.no;
            // xywh2xyxy, then boxes = x[:, :4] + cls * max_wh
            const float hw = p[2] / 2.0f, hh = p[3] / 2.0f;
            const float c = best[an].y * a.max_wh;
            me.x1 = (p[0] - hw) + c; me.y1 = (p[1] - hh) + c;
            me.x2 = (p[0] + hw) + c; me.y2 = (p[1] + hh) + c;
            me.area = (me.x2 - me.x1) * (me.y2 - me.y1);
        }
        bool alive = valid;
        for (int k = wave; k < nk; k += NMS_WAVES) {               // this wave's share of the kept boxes
            const CandBox kb = {kx1[k], ky1[k], kx2[k], ky2[k], kar[k]};
            if (alive && iou_gt(kb, me, a.iou)) alive = false;
        }
        const unsigned long long mine = __ballot(alive);
        if (lane == 0) survive[it & 1][wave] = mine;
        __syncthreads();
        unsigned long long all = ~0ull;
#pragma unroll
        for (int w = 0; w < NMS_WAVES; ++w) all &= survive[it & 1][w];
        alive = (all >> lane) & 1ull;
        unsigned long long mask = all;
        while (mask) {                                              // greedy pass inside the chunk (every wave, identically)
            const int jj = __ffsll((long long)mask) - 1;
            CandBox kb;
            kb.x1 = __shfl(me.x1, jj); kb.y1 = __shfl(me.y1, jj); kb.x2 = __shfl(me.x2, jj); kb.y2 = __shfl(me.y2, jj);
            kb.area = __shfl(me.area, jj);
            if (wave == 0 && lane == jj) { kx1[nk] = me.x1; ky1[nk] = me.y1; kx2[nk] = me.x2; ky2[nk] = me.y2; kar[nk] = me.area; kan[nk] = an; }
            ++nk;
            if (nk >= a.max_det) break;
            if (alive && lane > jj && iou_gt(kb, me, a.iou)) alive = false;
            mask = __ballot(alive && lane > jj);
        }
        __syncthreads();                                            // the kept arrays are complete before the next chunk reads them
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        a.out_counts[b] = nk;
        if (a.host_counts) a.host_counts[b] = nk;       // small synchronous calls: the count goes straight to pinned host memory too
    }
    // Rows, one 32-bit word per thread step: consecutive lanes write consecutive words of a row, so the stores coalesce whether the
    // destination is HBM or -- small synchronous calls, where a copy engine hand-over costs more than the kernels -- pinned host
    // memory (out_rows then points there).  Every word is computed with the expression order of A.6 (xywh2xyxy, pad, gain, clip).
    constexpr int RW = (int)(sizeof(mi355_det) / 4);
    static_assert(sizeof(mi355_det) == 4 * (7 + MI355_MAX_KPT_FLOATS), "row words: x1 y1 x2 y2 conf cls anchor kpt[]");
    unsigned* rows_w = (unsigned*)((mi355_det*)a.out_rows + (size_t)b * a.max_det);
    const int nkf = a.nk < MI355_MAX_KPT_FLOATS ? a.nk : MI355_MAX_KPT_FLOATS;
    const int kd = a.kdim > 0 ? a.kdim : 1;
    // scale-back constants: the call's scalars, or frame b's row of a mixed batch (same expressions, per-frame values)
    float gain = a.gain, pad_x = a.pad_x, pad_y = a.pad_y, kpad_x = a.kpad_x, kpad_y = a.kpad_y, orig_w = a.orig_w, orig_h = a.orig_h;
    if (a.frame_geom) {
        const float* fg = a.frame_geom + (size_t)b * 7;
        gain = fg[0]; pad_x = fg[1]; pad_y = fg[2]; kpad_x = fg[3]; kpad_y = fg[4]; orig_w = fg[5]; orig_h = fg[6];
    }
    for (int idx = threadIdx.x; idx < nk * RW; idx += 64 * NMS_WAVES) {
        const int k = idx / RW, q = idx - k * RW;
        const int an = kan[k];
        const float* p = pred + (size_t)an * a.no;
        unsigned w = 0u;
        if (q < 4) {
            const bool isx = (q & 1) == 0;
            const float half_ext = (isx ? p[2] : p[3]) / 2.0f;
            const float c = isx ? p[0] : p[1];
            float v = q < 2 ? c - half_ext : c + half_ext;
            if (a.scale_back) {
                v -= isx ? pad_x : pad_y;
                v /= gain;
                v = fminf(fmaxf(v, 0.f), isx ? orig_w : orig_h);
            }
            w = __float_as_uint(v);
        } else if (q == 4) {
            w = __float_as_uint(best[an].x);
        } else if (q == 5) {
            w = (unsigned)(int)best[an].y;
        } else if (q == 6) {
            w = (unsigned)an;
        } else if (q - 7 < nkf) {
            const int j = q - 7;
            float v = p[4 + a.nc + j];
            if (a.scale_back && a.kdim > 0 && (j % kd) < 2) {         // kdim 0: the extra columns are no keypoints, they pass untouched
                const bool isx = (j % kd) == 0;
                v -= isx ? kpad_x : kpad_y;
                v /= gain;
                v = fminf(fmaxf(v, 0.f), isx ? orig_w : orig_h);
            }
            w = __float_as_uint(v);
        }
        rows_w[idx] = w;
    }
}

__global__ __launch_bounds__(64 * NMS_WAVES) void nms_greedy_kernel(NmsArgs a, const int* cand_counts) {
    nms_greedy_body<NMS_WAVES>(a, blockIdx.x, cand_counts[blockIdx.x]);
}

// Sort and greedy suppression of one image in ONE launch (small calls: a launch costs more than either kernel's work; the greedy
// pass then runs on the sort's 16 waves, its share loop split 16 ways).  Same code, same order of operations, same rows.
__global__ __launch_bounds__(NMS_SORT_THREADS) void nms_sort_greedy_kernel(NmsArgs a, int* cand_counts) {
    __shared__ unsigned long long skeys[NMS_LDS_KEYS];
    __shared__ int scount;
    const int b = blockIdx.x, tid = threadIdx.x;
    unsigned long long* keys = a.keys + (size_t)b * a.Apow2;
    int n = 0;
    const int n2 = nms_collect(a, b, keys, &scount, tid, &n);
    if (n2 > 1) {
        if (n2 <= NMS_LDS_KEYS) {
            for (int i = tid; i < n2; i += NMS_SORT_THREADS) skeys[i] = keys[i];
            __syncthreads();
            bitonic_sort(skeys, n2, tid, NMS_SORT_THREADS);
            for (int i = tid; i < n; i += NMS_SORT_THREADS) keys[i] = skeys[i];
        } else {
            bitonic_sort_hybrid(keys, skeys, n2, tid);
        }
    }
    const int nc = n < a.max_nms ? n : a.max_nms;
    if (tid == 0) cand_counts[b] = nc;
    __syncthreads();                                   // the block's sorted keys (global memory) are visible to all of its threads
    nms_greedy_body<NMS_SORT_THREADS / 64>(a, b, nc);
}

static bool nms_fused_on() { static const bool on = !(getenv("MI355_NMS_FUSED") && atoi(getenv("MI355_NMS_FUSED")) == 0); return on; }

const char* launch_nms(const NmsArgs& a, hipStream_t st) {
    if (a.max_det < 1 || a.max_det > NMS_MAX_DET) return "nms: max_det must be in [1, 1024]";
    // cand_counts lives in the tail of out_counts' allocation: out_counts[B .. 2B)
    int* cand_counts = a.out_counts + a.B;
    if (a.Apow2 > 4 * NMS_LDS_KEYS) {
        // big maps: the sort as a sequence of wide launches (see nms_collect_kernel); sort lengths live at out_counts[2B .. 3B)
        int* sort_len = a.out_counts + 2 * a.B;
        const int chunks = a.Apow2 / NMS_LDS_KEYS;
        hipLaunchKernelGGL(nms_collect_kernel, dim3(a.B), dim3(NMS_SORT_THREADS), 0, st, a, cand_counts, sort_len);
        hipLaunchKernelGGL(nms_chunk_sort_kernel, dim3(a.B * chunks), dim3(NMS_SORT_THREADS), 0, st, a, sort_len, chunks);
        const int bpi = a.Apow2 / 2 / NMS_SORT_THREADS;
        for (int k = 2 * NMS_LDS_KEYS; k <= a.Apow2; k <<= 1) {
            for (int j = k >> 1; j >= NMS_LDS_KEYS; j >>= 1)
                hipLaunchKernelGGL(nms_global_step_kernel, dim3(a.B * bpi), dim3(NMS_SORT_THREADS), 0, st, a, sort_len, bpi, k, j);
            hipLaunchKernelGGL(nms_lds_steps_kernel, dim3(a.B * chunks), dim3(NMS_SORT_THREADS), 0, st, a, sort_len, chunks, k);
        }
    } else if (a.B <= 16 && nms_fused_on()) {
        // small calls: sort + greedy pass in one launch (a dependent launch costs 2.9 us + the kernel's ramp: DESIGN.md 3.5)
        hipLaunchKernelGGL(nms_sort_greedy_kernel, dim3(a.B), dim3(NMS_SORT_THREADS), 0, st, a, cand_counts);
        hipError_t e1 = hipGetLastError();
        return e1 == hipSuccess ? nullptr : hipGetErrorString(e1);
    } else {
        hipLaunchKernelGGL(nms_sort_kernel, dim3(a.B), dim3(NMS_SORT_THREADS), 0, st, a, cand_counts);
    }
    hipLaunchKernelGGL(nms_greedy_kernel, dim3(a.B), dim3(64 * NMS_WAVES), 0, st, a, cand_counts);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

// ---------------------------------------------------------------------------------------------- row compaction
__global__ __launch_bounds__(1024) void scan_counts_kernel(const int* counts, int n, int* offsets) {
    __shared__ int part[1024];
    const int tid = threadIdx.x;
    const int per = (n + 1023) / 1024;
    int sum = 0;
    for (int i = tid * per; i < n && i < (tid + 1) * per; ++i) sum += counts[i];
    part[tid] = sum;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {              // Hillis-Steele inclusive scan of the 1024 partial sums
        const int v = tid >= off ? part[tid - off] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int run = tid ? part[tid - 1] : 0;
    for (int i = tid * per; i < n && i < (tid + 1) * per; ++i) { offsets[i] = run; run += counts[i]; }
    if (tid == 1023) offsets[n] = part[1023];
}

__global__ __launch_bounds__(256) void compact_rows_kernel(const unsigned* rows, const int* counts, const int* offsets, int max_det,
                                                           int row_words, unsigned* packed) {
    const int i = blockIdx.x;
    const int words = counts[i] * row_words;
    const unsigned* src = rows + (size_t)i * max_det * row_words;
    unsigned* dst = packed + (size_t)offsets[i] * row_words;
    for (int w = threadIdx.x; w < words; w += 256) dst[w] = src[w];
}

const char* launch_compact_rows(const void* rows, const int* counts, int n, int max_det, int row_words, int* offsets, void* packed,
                                hipStream_t st) {
    hipLaunchKernelGGL(scan_counts_kernel, dim3(1), dim3(1024), 0, st, counts, n, offsets);
    hipLaunchKernelGGL(compact_rows_kernel, dim3(n), dim3(256), 0, st, (const unsigned*)rows, counts, offsets, max_det, row_words,
                       (unsigned*)packed);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

// ---------------------------------------------------------------------------------------------- object features
// Ultralytics' DetectionPredictor.get_obj_feats (with_reid, model: auto) for the rows NMS kept: the Detect head's input maps read at
// the anchor each row came from.  s = min(C_l) = dim; a row on level l (g = C_l / s) gets e[j] = mean(x[a, j*g .. j*g + g - 1]),
// j = 0 .. s-1, in the canonical order acc = x[0]; acc += x[r] for ascending r; e = acc / (float)g (IEEE division; g == 1 copies
// the bits).  fp16 maps are widened to fp32 first.
// ONE WAVE PER ROW SLOT (the grid covers B * cap slots; a wave whose slot is at or beyond counts[b] leaves without a store): the
// row's anchor_idx, hence its level and pixel, are the same for all lanes and live in scalar registers; in NHWC the pixel's C_l
// channels are one contiguous run, lane j reads the g channels of outputs j, j + 64, ... in one load where g allows it (16 bytes for
// g = 4, 8 for g = 2 in fp32; half that in fp16) and the 64 lanes store 256 contiguous bytes.  A frame's offsets fit 32 bits (the
// launcher checks); the frame base is 64-bit.
typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
typedef _Float16 half4_t __attribute__((ext_vector_type(4)));

template <bool HALF, int G>
__device__ __forceinline__ float obj_feat_group(const void* frame, unsigned at, int g) {
    float x[4];
    if (HALF) {
        const _Float16* p = (const _Float16*)frame + at;
        if (G == 4) { const half4_t v = *(const half4_t*)p; x[0] = (float)v.x; x[1] = (float)v.y; x[2] = (float)v.z; x[3] = (float)v.w; }
        else if (G == 2) { const half2_t v = *(const half2_t*)p; x[0] = (float)v.x; x[1] = (float)v.y; }
        else if (G == 0) { float acc = (float)p[0]; for (int r = 1; r < g; ++r) acc += (float)p[r]; return acc / (float)g; }
        else { for (int r = 0; r < G; ++r) x[r] = (float)p[r]; }
    } else {
        const float* p = (const float*)frame + at;
        if (G == 4) { const float4 v = *(const float4*)p; x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w; }
        else if (G == 2) { const float2 v = *(const float2*)p; x[0] = v.x; x[1] = v.y; }
        else if (G == 0) { float acc = p[0]; for (int r = 1; r < g; ++r) acc += p[r]; return acc / (float)g; }
        else { for (int r = 0; r < G; ++r) x[r] = p[r]; }
    }
    if (G == 1) return x[0];
    float acc = x[0];
    for (int r = 1; r < G; ++r) acc += x[r];
    return acc / (float)G;
}

template <bool HALF>
__global__ __launch_bounds__(256) void obj_feats_kernel(ObjFeatArgs a) {
    const int slot = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));     // wave-uniform from here on
    const int lane = threadIdx.x & 63;
    if (slot >= a.B * a.cap) return;
    const int b = slot / a.cap, r = slot - b * a.cap;
    if (r >= a.counts[b]) return;
    const int anchor = __builtin_amdgcn_readfirstlane(((const int*)a.rows)[((size_t)b * a.cap + r) * a.row_words + a.anchor_word]);
    if (anchor < 0 || anchor >= a.A) return;                      // never a row NMS wrote; an index outside the maps is not followed
    ObjFeatLevel L = a.lv[0];                                    // the level the anchor lies on: scalar selects over constant indices
#pragma unroll
    for (int i = 1; i < 4; ++i) if (i < a.n_levels && anchor >= a.lv[i].anchor0) L = a.lv[i];
    const int g = L.C / a.dim;
    const void* frame = (const char*)L.base + (size_t)b * L.H * L.W * L.cs * (HALF ? 2 : 4);
    const unsigned px = (unsigned)(anchor - L.anchor0) * (unsigned)L.cs + (unsigned)L.c_off;
    float* out = a.feats + ((size_t)b * a.cap + r) * a.dim;
    for (int o = lane; o < a.dim; o += 64) {
        const unsigned at = px + (unsigned)(o * g);
        float e;
        switch (g) {
            case 1: e = obj_feat_group<HALF, 1>(frame, at, g); break;
            case 2: e = obj_feat_group<HALF, 2>(frame, at, g); break;
            case 3: e = obj_feat_group<HALF, 3>(frame, at, g); break;
            case 4: e = obj_feat_group<HALF, 4>(frame, at, g); break;
            default: e = obj_feat_group<HALF, 0>(frame, at, g); break;
        }
        out[o] = e;
    }
}

const char* launch_obj_feats(const ObjFeatArgs& a, hipStream_t st) {
    if (a.n_levels < 1 || a.n_levels > 4 || a.B < 1 || a.cap < 1 || a.dim < 1) return "obj_feats: bad shape";
    const int align = a.half ? 8 : 4;                             // elements: what the 8- and 16-byte loads need
    long anchors = 0;
    for (int l = 0; l < a.n_levels; ++l) {
        const ObjFeatLevel& L = a.lv[l];
        if (!L.base || L.C < a.dim || L.C % a.dim || L.c_off < 0 || L.c_off + L.C > L.cs || L.H < 1 || L.W < 1) return "obj_feats: bad level";
        if ((L.cs % align) || (L.c_off % align) || ((uintptr_t)L.base % 16)) return "obj_feats: a level's stride, offset or base is not aligned for vector loads";
        if ((long)L.H * L.W * L.cs >= (1l << 31)) return "obj_feats: a frame's map exceeds 32-bit offsets";
        if (L.anchor0 != (int)anchors) return "obj_feats: level starts do not follow the anchor order";
        anchors += (long)L.H * L.W;
    }
    if (anchors != a.A || (long)a.cap * a.dim >= (1l << 31) || (long)a.B * a.cap >= (1l << 31) - 4) return "obj_feats: bad anchor count or row capacity";
    const unsigned blocks = (unsigned)(((long)a.B * a.cap + 3) / 4);
    if (a.half) hipLaunchKernelGGL(obj_feats_kernel<true>, dim3(blocks), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(obj_feats_kernel<false>, dim3(blocks), dim3(256), 0, st, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

// ---------------------------------------------------------------------------------------------- tile merge
// The per-entry rows of a tiled predict call (include/mi355_yolo.h) -> one row list per source frame.  ONE BLOCK PER
// FRAME, 16 waves, the NMS kernels' structure on rows instead of anchors:
//   gather   wave w takes entries w, w + 16, ...: the entry's count, its first candidate and its origin are wave-uniform, lane r builds
//            the key (~conf bits << 32) | (e * max_det + r) of row r -- keys are unique, so the sort below is the stable order
//   sort     bitonic_sort in LDS up to 4096 keys (7 entries x 300 rows), bitonic_sort_hybrid on the frame's global key scratch beyond
//   greedy   nms_greedy_body's wave-ballot pass: chunks of 64 candidates in key order, the test against the kept rows split over the
//            waves, the pass inside the chunk run by every wave alike; a candidate dies iff an earlier kept row of the SAME class
//            overlaps it by more than thr (tile_overlap_gt: IoS or IoU on the shifted boxes)
//   rows     one 32-bit word per thread step, consecutive lanes on consecutive words of a row (plain vector stores, coalesced whether
//            out_rows is HBM or pinned host memory): box and keypoint x / y get one fp32 add of the origin, every other word its bits
// LDS: 32 KB of keys + 28 KB of kept rows (5 floats, class, slot per row; max_det <= 1024) + 1 KB of per-entry values = 61 KB of the
// 64 KB a block may declare; one block per frame, so occupancy is not a consideration.  A frame's offsets fit 32 bits: the launcher
// refuses more than MI355_TILE_MAX_CANDIDATES candidates per frame; the frame's bases are 64-bit.
constexpr int TM_WAVES = NMS_SORT_THREADS / 64;

__global__ __launch_bounds__(NMS_SORT_THREADS) void tile_merge_kernel(TileMergeArgs a) {
    __shared__ unsigned long long skeys[NMS_LDS_KEYS];
    __shared__ float kx1[NMS_MAX_DET], ky1[NMS_MAX_DET], kx2[NMS_MAX_DET], ky2[NMS_MAX_DET], kar[NMS_MAX_DET];
    __shared__ int kcl[NMS_MAX_DET], ksl[NMS_MAX_DET];
    __shared__ unsigned long long survive[2][TM_WAVES];
    __shared__ int spre[MI355_TILE_MAX_ENTRIES + 1];
    __shared__ float sox[MI355_TILE_MAX_ENTRIES], soy[MI355_TILE_MAX_ENTRIES];
    const int f = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int e0 = a.entry_off ? a.entry_off[f] : f * a.entries;
    int E = a.entry_off ? a.entry_off[f + 1] - e0 : a.entries;
    E = E < 0 ? 0 : (E > a.entries ? a.entries : E);                  // never more than the launcher sized the frame for
    const int* counts = a.counts + e0;
    const unsigned* rows = a.rows + (size_t)e0 * a.max_det * TILE_ROW_WORDS;
    if (tid == 0) {
        int at = 0;
        for (int e = 0; e < E; ++e) { spre[e] = at; const int c = counts[e]; at += c < 0 ? 0 : (c > a.max_det ? a.max_det : c); }
        spre[E] = at;
    }
    if (tid < E) { sox[tid] = (float)a.origins[2 * (e0 + tid)]; soy[tid] = (float)a.origins[2 * (e0 + tid) + 1]; }
    __syncthreads();
    const int n = spre[E];
    int n2 = 1;
    while (n2 < n) n2 <<= 1;
    const bool in_lds = n2 <= NMS_LDS_KEYS;
    // (a frame beyond the LDS form without scratch cannot get here: the launcher sizes key_stride from entries * max_det)
    unsigned long long* keys = in_lds ? skeys : a.keys + (size_t)f * a.key_stride;
    for (int e = wave; e < E; e += TM_WAVES) {                        // e, its count and its first candidate: the same in every lane
        const int first = spre[e], cnt = spre[e + 1] - first;
        const unsigned* er = rows + (size_t)e * a.max_det * TILE_ROW_WORDS;
        for (int r = lane; r < cnt; r += 64)
            keys[first + r] = ((unsigned long long)(~er[r * TILE_ROW_WORDS + 4]) << 32) | (unsigned)(e * a.max_det + r);
    }
    for (int i = n + tid; i < n2; i += NMS_SORT_THREADS) keys[i] = ~0ull;
    __syncthreads();
    if (n2 > 1) {
        if (in_lds) bitonic_sort(skeys, n2, tid, NMS_SORT_THREADS);
        else bitonic_sort_hybrid(keys, skeys, n2, tid);
    }
    __syncthreads();
    // ---- greedy suppression in key order
    int nk = 0, it = 0;
    for (int base = 0; base < n && nk < a.max_det; base += 64, ++it) {
        const int j = base + lane;
        const bool valid = j < n;
        int slot = 0, cls = 0;
        TileBox me = {0.f, 0.f, 0.f, 0.f, 0.f};
        if (valid) {
            slot = (int)(keys[j] & 0xffffffffull);
            const int e = slot / a.max_det;
            const unsigned* p = rows + (size_t)slot * TILE_ROW_WORDS;
            const float ox = sox[e], oy = soy[e];
            me.x1 = __uint_as_float(p[0]) + ox; me.y1 = __uint_as_float(p[1]) + oy;
            me.x2 = __uint_as_float(p[2]) + ox; me.y2 = __uint_as_float(p[3]) + oy;
            me.area = (me.x2 - me.x1) * (me.y2 - me.y1);
            cls = (int)p[5];
        }
        bool alive = valid;
        for (int k = wave; k < nk; k += TM_WAVES) {                   // this wave's share of the kept rows
            const TileBox kb = {kx1[k], ky1[k], kx2[k], ky2[k], kar[k]};
            if (alive && kcl[k] == cls && tile_overlap_gt(kb, me, a.metric, a.thr)) alive = false;
        }
        const unsigned long long mine = __ballot(alive);
        if (lane == 0) survive[it & 1][wave] = mine;
        __syncthreads();
        unsigned long long all = ~0ull;
#pragma unroll
        for (int w = 0; w < TM_WAVES; ++w) all &= survive[it & 1][w];
        alive = (all >> lane) & 1ull;
        unsigned long long mask = all;
        while (mask) {                                                // greedy pass inside the chunk (every wave, identically)
            const int jj = __ffsll((long long)mask) - 1;
            TileBox kb;
            kb.x1 = __shfl(me.x1, jj); kb.y1 = __shfl(me.y1, jj); kb.x2 = __shfl(me.x2, jj); kb.y2 = __shfl(me.y2, jj);
            kb.area = __shfl(me.area, jj);
            const int kc = __shfl(cls, jj);
            if (wave == 0 && lane == jj) { kx1[nk] = me.x1; ky1[nk] = me.y1; kx2[nk] = me.x2; ky2[nk] = me.y2; kar[nk] = me.area; kcl[nk] = cls; ksl[nk] = slot; }
            ++nk;
            if (nk >= a.max_det) break;
            if (alive && lane > jj && kc == cls && tile_overlap_gt(kb, me, a.metric, a.thr)) alive = false;
            mask = __ballot(alive && lane > jj);
        }
        __syncthreads();                                              // the kept arrays are complete before the next chunk reads them
    }
    __syncthreads();
    if (tid == 0) a.out_counts[f] = nk;
    unsigned* out = a.out_rows + (size_t)f * a.max_det * TILE_ROW_WORDS;
    for (int idx = tid; idx < nk * TILE_ROW_WORDS; idx += NMS_SORT_THREADS) {
        const int k = idx / TILE_ROW_WORDS, q = idx - k * TILE_ROW_WORDS;
        const int slot = ksl[k], e = slot / a.max_det;
        out[idx] = tile_shift_word(rows[(size_t)slot * TILE_ROW_WORDS + q], q, sox[e], soy[e], a.nk, a.kdim);
    }
    if (a.out_tile_idx)
        for (int k = tid; k < nk; k += NMS_SORT_THREADS) a.out_tile_idx[(size_t)f * a.max_det + k] = ksl[k] / a.max_det;
}

const char* launch_tile_merge(const TileMergeArgs& a, hipStream_t st) {
    if (a.n_frames < 1 || a.entries < 1 || a.entries > MI355_TILE_MAX_ENTRIES) return "tile_merge: entries per frame must be in [1, 64]";
    if (a.max_det < 1 || a.max_det > NMS_MAX_DET) return "tile_merge: max_det must be in [1, 1024]";
    const long cand = (long)a.entries * a.max_det;
    if (cand > MI355_TILE_MAX_CANDIDATES) return "tile_merge: more candidates per frame than the kernel's capacity";
    if (cand > NMS_LDS_KEYS) {
        long p2 = 1; while (p2 < cand) p2 <<= 1;
        if (!a.keys || a.key_stride < p2 || (a.key_stride & (a.key_stride - 1))) return "tile_merge: key scratch missing or too small";
    }
    if (a.nk < 0 || a.nk > MI355_MAX_KPT_FLOATS || !(a.kdim == 0 || a.kdim == 2 || a.kdim == 3)) return "tile_merge: bad keypoint shape";
    if (a.metric != MI355_TILE_IOS && a.metric != MI355_TILE_IOU) return "tile_merge: unknown metric";
    if (!a.rows || !a.counts || !a.origins || !a.out_rows || !a.out_counts) return "tile_merge: null argument";
    hipLaunchKernelGGL(tile_merge_kernel, dim3(a.n_frames), dim3(NMS_SORT_THREADS), 0, st, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

}  // namespace mi355
