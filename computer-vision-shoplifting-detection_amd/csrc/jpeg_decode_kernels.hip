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
// entropy = sync (jpeg_sync.h) decodes a restart segment with many lanes and puts four launches in front of idct and colour, whatever the
// number of frames: local rounds (a workgroup per sequence: round 0 and the re-walks, states in LDS), global rounds + block index (a
// workgroup per frame), write pass (a lane per subsequence; the block indices of a sequence by a scan in LDS), DC pass (a workgroup per
// frame and component).  No workgroup waits for another one and nothing is read back between the launches.
// entropy = host replaces the first launch by the twin's segment routine on the calling thread; the coefficients travel with the
// descriptors.  The rules themselves are jpeg_decode.h's, shared with the host twin (device = -1).
#include "engine_internal.h"
#include "jpeg_sync.h"

namespace mi355 {
namespace {

constexpr int kDecLanes = 256;
constexpr int kDecGroupBlocks = 24;
constexpr int kDecBlkStride = 72, kDecRowStride = 9;      // LDS layout of a staged block: with rows of 9 ints a half-wave hits 32 different banks in both passes

__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const JpegDecFrame* __restrict__ frames) {
    const JpegDecFrame& f = frames[blockIdx.y];
    const int s0 = (int)blockIdx.x * 64;
    if (f.lanes != 1 || s0 >= f.nseg) return;                              // block-uniform
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

// ---- entropy = sync (jpeg_sync.h) ----------------------------------------------------------------------------------------------------------
__device__ void jpeg_stage_huff(const JpegDecFrame& f, JpegHuff* s_h, int t) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(f.huff);
    uint32_t* dst = reinterpret_cast<uint32_t*>(s_h);
    for (int i = t; i < (int)(4 * sizeof(JpegHuff) / 4); i += kDecLanes) dst[i] = src[i];
}

// inclusive segmented sum over the 256 lanes: fl starts a segment at its lane.  Every lane of the block calls it.
__device__ uint32_t jpeg_seg_scan(uint32_t v, uint32_t fl, uint32_t* s_v, uint32_t* s_f, int t) {
    s_v[t] = v; s_f[t] = fl;
    __syncthreads();
    for (int d = 1; d < kDecLanes; d <<= 1) {
        const uint32_t pv = t >= d ? s_v[t - d] : 0u, pf = t >= d ? s_f[t - d] : 1u;
        __syncthreads();
        if (!fl) { v += pv; fl = pf; }
        s_v[t] = v; s_f[t] = fl;
        __syncthreads();
    }
    return v;
}

__global__ __launch_bounds__(256) void jpeg_sync_local_kernel(const JpegDecFrame* __restrict__ frames) {
    const JpegDecFrame& f = frames[blockIdx.y];
    if (f.lanes != 2 || blockIdx.x >= f.sy.nseq) return;                // block-uniform
    const int t = (int)threadIdx.x;
    __shared__ JpegHuff s_h[4];
    __shared__ JpegSyncState s_x[kDecLanes];
    __shared__ uint32_t s_chg[2][kDecLanes];
    jpeg_stage_huff(f, s_h, t);
    const JpegSyncSeq sq = f.sy.seqs[blockIdx.x];
    const JpegSyncSeg sg = f.sy.segs[sq.seg];
    const int S = f.sy.S, Q = f.sy.Q;
    const bool live = (uint32_t)t < sq.nsub;
    const uint32_t li = sq.lsub0 + (uint32_t)t, end = live ? jpeg_sync_end(li, S, sg.len) : 0u;
    JpegFetchWords fetch{reinterpret_cast<const uint32_t*>(f.scan)};
    JpegSyncState x{0u, 0u};
    uint32_t e = 0;
    __syncthreads();
    if (live) x = jpeg_sync_walk(f, s_h, fetch, sg.begin, sg.len, end, jpeg_sync_guess(fetch, sg.begin, li, S), e, nullptr, (JpegPosBits<JpegFetchWords>*)nullptr);
    s_x[t] = x; s_chg[0][t] = live;
    __syncthreads();
    int cur = 0, rounds = 0;
    for (int r = 1; r < Q; ++r) {                                       // at most Q rounds with round 0
        const bool redo = live && t > 0 && s_chg[cur][t - 1];
        const JpegSyncState in = redo ? s_x[t - 1] : x;
        __syncthreads();                                                // every read of the round before any write
        uint32_t c = 0;
        if (redo) {
            const JpegSyncState nx = jpeg_sync_walk(f, s_h, fetch, sg.begin, sg.len, end, in, e, nullptr, (JpegPosBits<JpegFetchWords>*)nullptr);
            c = !jpeg_sync_same(nx, x);
            x = nx; s_x[t] = x;
        }
        s_chg[cur ^ 1][t] = c;
        if (!__syncthreads_or((int)c)) break;
        rounds = r; cur ^= 1;
    }
    if (live) { f.sy.X[sq.sub0 + t] = x; f.sy.E[sq.sub0 + t] = e; }
    if (t == 0 && rounds) atomicMax(&f.sy.stats[0], (uint32_t)rounds);
}

__global__ __launch_bounds__(256) void jpeg_sync_global_kernel(const JpegDecFrame* __restrict__ frames) {
    const JpegDecFrame& f = frames[blockIdx.x];
    if (f.lanes != 2) return;                                           // block-uniform
    const int t = (int)threadIdx.x;
    __shared__ JpegHuff s_h[4];
    __shared__ uint32_t s_v[kDecLanes], s_f[kDecLanes], s_carry;
    jpeg_stage_huff(f, s_h, t);
    const uint32_t nseq = f.sy.nseq;
    const int S = f.sy.S;
    const JpegSyncSeq* seqs = f.sy.seqs;
    JpegSyncState* X = f.sy.X;
    uint32_t* E = f.sy.E;
    uint32_t* mk = f.sy.mark;
    uint32_t* nm = f.sy.mark + nseq;
    JpegFetchWords fetch{reinterpret_cast<const uint32_t*>(f.scan)};
    int some = 0;
    for (uint32_t q = (uint32_t)t; q < nseq; q += kDecLanes) {
        const uint32_t m = seqs[q].lsub0 != 0u;                          // all but a segment's first: walked from the guess so far
        mk[q] = m; nm[q] = 0u; some |= (int)m;
    }
    int any = __syncthreads_or(some);
    uint32_t rounds = 0;
    for (uint32_t r = 1; r <= nseq && any; ++r) {                       // at most as many rounds as the frame has sequences
        for (uint32_t q = (uint32_t)t; q < nseq; q += kDecLanes)
            if (mk[q]) f.sy.entry[q] = X[seqs[q].sub0 - 1];
        __syncthreads();                                                // every read of the round before any write
        int wrote = 0, next = 0;
        for (uint32_t q = (uint32_t)t; q < nseq; q += kDecLanes) {
            if (!mk[q]) continue;
            mk[q] = 0u;
            const JpegSyncSeq sq = seqs[q];
            const JpegSyncSeg sg = f.sy.segs[sq.seg];
            JpegSyncState in = f.sy.entry[q];
            for (uint32_t u = 0; u < sq.nsub; ++u) {
                const uint32_t i = sq.sub0 + u;
                uint32_t e;
                const JpegSyncState x = jpeg_sync_walk(f, s_h, fetch, sg.begin, sg.len, jpeg_sync_end(sq.lsub0 + u, S, sg.len), in, e, nullptr,
                                                       (JpegPosBits<JpegFetchWords>*)nullptr);
                E[i] = e;
                if (jpeg_sync_same(x, X[i])) break;
                X[i] = x; in = x; wrote = 1;
                if (u + 1 == sq.nsub && q + 1 < nseq && seqs[q + 1].seg == sq.seg) { nm[q + 1] = 1u; next = 1; }
            }
        }
        any = __syncthreads_or(next);
        if (__syncthreads_or(wrote)) rounds = r;
        uint32_t* sw = mk; mk = nm; nm = sw;
    }
    if (t == 0) f.sy.stats[1] = rounds;
    // the block in progress at every sequence's entry: the segment's first block + the blocks its earlier sequences completed
    if (t == 0) s_carry = 0u;
    __syncthreads();
    for (uint32_t base = 0; base < nseq; base += kDecLanes) {
        const uint32_t q = base + (uint32_t)t;
        uint32_t tot = 0, fl = 1u, blk0 = 0;
        if (q < nseq) {
            const JpegSyncSeq sq = seqs[q];
            for (uint32_t u = 0; u < sq.nsub; ++u) tot += E[sq.sub0 + u];
            fl = sq.lsub0 == 0u;
            blk0 = f.sy.segs[sq.seg].blk0;
        }
        uint32_t v = tot;
        if (t == 0 && !fl) { v += s_carry; fl = 1u; }
        const uint32_t incl = jpeg_seg_scan(v, fl, s_v, s_f, t);
        if (q < nseq) f.sy.seq_blk[q] = blk0 + incl - tot;
        if (t == kDecLanes - 1) s_carry = incl;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void jpeg_sync_write_kernel(const JpegDecFrame* __restrict__ frames) {
    const JpegDecFrame& f = frames[blockIdx.y];
    if (f.lanes != 2 || blockIdx.x >= f.sy.nseq) return;                // block-uniform
    const int t = (int)threadIdx.x;
    __shared__ JpegHuff s_h[4];
    __shared__ uint32_t s_v[kDecLanes], s_f[kDecLanes];
    jpeg_stage_huff(f, s_h, t);
    const JpegSyncSeq sq = f.sy.seqs[blockIdx.x];
    const JpegSyncSeg sg = f.sy.segs[sq.seg];
    const bool live = (uint32_t)t < sq.nsub;
    const uint32_t g = sq.sub0 + (uint32_t)t, e = live ? f.sy.E[g] : 0u;
    const uint32_t B = f.sy.seq_blk[blockIdx.x] + jpeg_seg_scan(e, t == 0, s_v, s_f, t) - e;     // the scan's barriers also publish s_h
    if (!live) return;
    f.sy.B[g] = B;
    JpegFetchWords fetch{reinterpret_cast<const uint32_t*>(f.scan)};
    const JpegSyncState in = sq.lsub0 + (uint32_t)t ? f.sy.X[g - 1] : JpegSyncState{0u, 0u};
    const uint32_t key = jpeg_sync_write_lane(f, s_h, fetch, sg, sq, (uint32_t)t, in, B);
    if (key != 0xFFFFFFFFu) atomicMin(reinterpret_cast<unsigned int*>(f.status), key);
}

constexpr int kSyncDcRun = 8;                                           // DC values per lane and chunk
__global__ __launch_bounds__(256) void jpeg_sync_dc_kernel(const JpegDecFrame* __restrict__ frames) {
    const JpegDecFrame& f = frames[blockIdx.y];
    const int c = (int)blockIdx.x;
    if (f.lanes != 2 || c >= f.ncomp) return;                           // block-uniform
    const int t = (int)threadIdx.x;
    __shared__ uint32_t s_v[kDecLanes], s_f[kDecLanes], s_carry;
    const long long ne = jpeg_sync_dc_count(f, c);
    const long long nblk = jpeg_dec_blocks(f);
    if (t == 0) s_carry = 0u;
    __syncthreads();
    for (long long base = 0; base < ne; base += (long long)kDecLanes * kSyncDcRun) {
        const long long e0 = base + (long long)t * kSyncDcRun;
        uint32_t val[kSyncDcRun], blk[kSyncDcRun];
        uint32_t run = t == 0 ? s_carry : 0u, fl = 0u;
        int head = kSyncDcRun;                                          // the values in front of the run's first segment start take the prefix
#pragma unroll
        for (int i = 0; i < kSyncDcRun; ++i) {
            val[i] = 0u; blk[i] = 0xFFFFFFFFu;
            if (e0 + i >= ne) continue;
            bool first;
            const long long b = jpeg_sync_dc_block(f, c, e0 + i, first);
            if (b >= nblk) continue;
            if (first) { run = 0u; if (!fl) head = i; fl = 1u; }
            run += (uint32_t)(int)f.coef[b * 64];
            val[i] = run; blk[i] = (uint32_t)b;
        }
        const uint32_t incl = jpeg_seg_scan(run, fl, s_v, s_f, t);
        const uint32_t prefix = t ? s_v[t - 1] : 0u;
#pragma unroll
        for (int i = 0; i < kSyncDcRun; ++i)
            if (blk[i] != 0xFFFFFFFFu) f.coef[(size_t)blk[i] * 64] = (int16_t)(uint16_t)(val[i] + (i < head ? prefix : 0u));
        __syncthreads();                                                // s_v read before the next chunk's scan writes it
        if (t == kDecLanes - 1) s_carry = incl;
        __syncthreads();
    }
}

constexpr size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

// The GPU half of one call; the streams are parsed and every argument checked (jpeg_dec_call).  lanes[i]: frame i's entropy stage runs
// on the GPU -- 1: a lane per segment, 2: sync.  outs (BGR) or coefs (the entropy stage alone, host int16) is given.
int jpeg_dec_run_gpu(JpegDecCtx* ctxp, int device, std::vector<JpegParsed>& P, const mi355_jpeg_stream* streams, int n, const int* lanes,
                     const mi355_render_out* outs, int16_t* const* coefs, int* status, void* stream, float* launch_ms, const JpegSyncOpts& so) {
    hipStream_t st = (hipStream_t)stream;
    JpegDecCtx local;
    JpegDecCtx& ctx = ctxp ? *ctxp : local;
    struct Free { JpegDecCtx* c; ~Free() { if (c) jpeg_dec_ctx_free(*c); } } free_local{ctxp ? nullptr : &local};
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return fail(MI355_EHIP, "no HIP device: the JPEG decode kernels need an MI355X (device = -1 runs their host twin)"); }
    if (device >= ndev) return fail(MI355_EINVAL, "jpeg decode: device out of range");
    HIPCHK(hipSetDevice(device));
    if (launch_ms) *launch_ms = 0.f;
    // the image, built in pinned memory and uploaded in one copy: [descriptors | Huffman tables | status | per frame: segment offsets (sync:
    // the segment and sequence tables), scan bytes (lanes, sync) or coefficients (host entropy)]; behind it on the device: [coefficients
    // of the lane and sync frames, a sync frame's round counts | a sync frame's states, counts and block indices | planes | host outputs]
    const size_t huff_off = al256((size_t)n * sizeof(JpegDecFrame)), stat_off = al256(huff_off + (size_t)n * 4 * sizeof(JpegHuff));
    size_t at = al256(stat_off + (size_t)n * 4);
    std::vector<size_t> seg_off((size_t)n), data_off((size_t)n), coef_off((size_t)n), plane_off((size_t)n * 3, 0), out_off((size_t)n, 0);
    std::vector<JpegSyncTables> T((size_t)n);
    std::vector<size_t> stats_off((size_t)n, 0), sync_off((size_t)n, 0);
    for (int i = 0; i < n; ++i) {
        const JpegDecFrame& f = P[i].f;
        if (lanes[i] == 2) jpeg_sync_tables(P[i], so.S, so.Q, T[i]);
        if (lanes[i]) {
            seg_off[i] = at; at = al256(at + (lanes[i] == 2 ? T[i].segs.size() * sizeof(JpegSyncSeg) + T[i].seqs.size() * sizeof(JpegSyncSeq) : (size_t)f.nseg * 8));
            data_off[i] = at; at = al256(at + (size_t)(P[i].scan_end - P[i].scan_begin) + 8);
        } else { coef_off[i] = at; at = al256(at + (size_t)jpeg_dec_blocks(f) * 128); }
    }
    const size_t img_bytes = at, zero_off = at;
    for (int i = 0; i < n; ++i)
        if (lanes[i]) {
            coef_off[i] = at; at = al256(at + (size_t)jpeg_dec_blocks(P[i].f) * 128);
            if (lanes[i] == 2) { stats_off[i] = at; at = al256(at + 16); }
        }
    const size_t zero_bytes = at - zero_off;
    long long most_seq = 0;
    for (int i = 0; i < n; ++i)
        if (lanes[i] == 2) {                                             // X | entry | E | B | seq_blk | mark
            const size_t ns = T[i].nsub, nq = T[i].seqs.size();
            sync_off[i] = at; at = al256(at + ns * 8 + nq * 8 + ns * 4 + ns * 4 + nq * 4 + nq * 8);
            most_seq = std::max(most_seq, (long long)nq);
        }
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
        if (lanes[i] == 1) most_seg = std::max(most_seg, (long long)f.nseg);
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
            if (lanes[i] == 2) {
                const size_t ns = T[i].nsub, nq = T[i].seqs.size(), sb = T[i].segs.size() * sizeof(JpegSyncSeg);
                f.seg = nullptr;
                std::memcpy(img + seg_off[i], T[i].segs.data(), sb);
                std::memcpy(img + seg_off[i] + sb, T[i].seqs.data(), nq * sizeof(JpegSyncSeq));
                uint8_t* w = base + sync_off[i];
                f.sy = JpegSync{so.S, so.Q, (uint32_t)ns, (uint32_t)nq, (const JpegSyncSeg*)(base + seg_off[i]), (const JpegSyncSeq*)(base + seg_off[i] + sb),
                                (JpegSyncState*)w, (uint32_t*)(w + ns * 8 + nq * 8), (uint32_t*)(w + ns * 12 + nq * 8), (uint32_t*)(w + ns * 16 + nq * 8),
                                (JpegSyncState*)(w + ns * 8), (uint32_t*)(w + ns * 16 + nq * 12), (uint32_t*)(base + stats_off[i])};
                ((uint32_t*)(img + stat_off))[i] = 0xFFFFFFFFu;          // the status key: a minimum (jpeg_sync.h)
            } else
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
    if (most_seg > 0 || most_seq > 0) HIPCHK(hipMemsetAsync(base + zero_off, 0, zero_bytes, st));
    if (most_seg > 0) {
        hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)((most_seg + 63) / 64), (unsigned)n), dim3(64), 0, st, dd);
        KCHK(launched());
    }
    if (most_seq > 0) {                                                  // entropy = sync: four launches, whatever the number of frames
        hipLaunchKernelGGL(jpeg_sync_local_kernel, dim3((unsigned)most_seq, (unsigned)n), dim3(kDecLanes), 0, st, dd);
        KCHK(launched());
        hipLaunchKernelGGL(jpeg_sync_global_kernel, dim3((unsigned)n), dim3(kDecLanes), 0, st, dd);
        KCHK(launched());
        hipLaunchKernelGGL(jpeg_sync_write_kernel, dim3((unsigned)most_seq, (unsigned)n), dim3(kDecLanes), 0, st, dd);
        KCHK(launched());
        hipLaunchKernelGGL(jpeg_sync_dc_kernel, dim3(3, (unsigned)n), dim3(kDecLanes), 0, st, dd);
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
    std::vector<JpegSyncState> hx;                                       // the hook: exit states, block indices and round counts of its one frame
    std::vector<uint32_t> hb;
    uint32_t hstats[4] = {0u, 0u, 0u, 0u};
    if ((so.states || so.stats) && n == 1 && lanes[0] == 2) {
        hx.resize(T[0].nsub); hb.resize(T[0].nsub);
        HIPCHK(hipMemcpyAsync(hx.data(), P[0].f.sy.X, hx.size() * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(hb.data(), P[0].f.sy.B, hb.size() * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(hstats, P[0].f.sy.stats, 16, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    if (!hx.empty()) {
        if (so.stats) *so.stats = mi355_jpeg_sync_stats{(int)T[0].nsub, (int)T[0].seqs.size(), (int)hstats[0], (int)hstats[1]};
        if (so.states)
            for (const JpegSyncSeg& g : T[0].segs)
                for (uint32_t u = 0; u < g.nsub; ++u) {
                    const uint32_t i = g.sub0 + u;
                    const JpegSyncState e = u ? hx[i - 1] : JpegSyncState{0u, 0u};
                    so.states[i] = mi355_jpeg_sync_state{(int)(&g - T[0].segs.data()), e.byte, (int)(e.meta & 7u), (int)((e.meta >> 3) & 7u), (int)(e.meta >> 6), hb[i]};
                }
    }
    if (launch_ms) HIPCHK(hipEventElapsedTime(launch_ms, ctx.ev0, ctx.ev1));
    for (int i = 0; i < n; ++i) {
        const int s = lanes[i] == 2 ? ((uint32_t)h_stat[i] == 0xFFFFFFFFu ? 0 : h_stat[i] & 7) : lanes[i] ? h_stat[i] : host_status[i];
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
