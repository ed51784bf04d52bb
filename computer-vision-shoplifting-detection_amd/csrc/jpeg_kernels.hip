// JPEG evidence frames: BGR frames in HBM in, baseline JFIF streams out.  Three launches per call, whatever the number
// of frames (descriptor-driven, blockIdx.y = frame):
//   transform  one block of 256 lanes per 64-pixel-wide run of MCUs (4 MCUs of 4:2:0, 8 of 4:4:4: 24 blocks of 8 x 8 either way).  The
//              pixels are converted into Y / Cb / Cr planes in LDS (edge pixels repeated), the 24 blocks gathered (chroma averaged for
//              4:2:0, level shift), 192 lanes run the row pass and then the column pass of the DCT, one 8-vector each, and every lane
//              quantises six coefficients and writes them in zigzag order: int16 [blocks][64], blocks in scan order.
//   code       one block per restart segment (= MCU row).  256 of the segment's blocks at a time are staged in LDS, one lane per block:
//              the lane forms its DC difference and walks its coefficients twice -- once to count its bits, then, after a block-wide scan
//              has given its bit offset, to OR its codes into the segment's zeroed buffer of big-endian words (atomicOr on the words it
//              shares with its neighbours, plain stores on the words it fills alone).  OR is order-free: no output bit depends on the order in
//              which lanes arrive.  The last byte is padded with 1-bits and the segment's 0xFF bytes are counted.
//   pack       one block per segment: the sizes of the segments before it give its offset behind the header; it copies its bytes there
//              with a 0x00 behind every 0xFF (a scan of the 0xFF counts places them) and RSTm in front; segment 0 copies the header, the
//              last one writes EOI and the stream's length.
// The rules themselves are jpeg_codec.h's, shared with the host twin (device = -1).
#include "engine_internal.h"
#include "jpeg_codec.h"

namespace mi355 {
namespace {

constexpr int kJpegLanes = 256;
constexpr int kJpegGroupBlocks = 24;            // 8 x 8 blocks of a transform group
constexpr int kJpegZzRow = 65;                  // int16 per staged block in the code kernel: an odd number of half-words spreads the lanes over the banks

__global__ __launch_bounds__(256) void jpeg_transform_kernel(const JpegFrame* __restrict__ frames, const JpegTables* __restrict__ tab) {
    const JpegFrame f = frames[blockIdx.y];
    const bool sub = f.bpm == 6;
    const int tm = sub ? 4 : 8;                                        // MCUs of a group
    const int groups_x = (f.mcus_x + tm - 1) / tm;
    const long long g = blockIdx.x;
    if (g >= (long long)groups_x * f.mcus_y) return;                   // block-uniform
    const int t = (int)threadIdx.x;
    const int row = (int)(g / groups_x), gx = (int)(g - (long long)row * groups_x);
    const int x0 = gx * 64, y0 = row * f.mcu;

    __shared__ uint8_t s_px[3][16][64];
    __shared__ int s_blk[kJpegGroupBlocks * 64];

    for (int i = t; i < f.mcu * 64; i += kJpegLanes) {
        const int y = i >> 6, x = i & 63;
        const uint8_t* p = f.src + (size_t)jpeg_min(y0 + y, f.H - 1) * f.pitch + (size_t)jpeg_min(x0 + x, f.W - 1) * 3;
        int yy, cb, cr;
        jpeg_ycc(p[0], p[1], p[2], yy, cb, cr);
        s_px[0][y][x] = (uint8_t)yy; s_px[1][y][x] = (uint8_t)cb; s_px[2][y][x] = (uint8_t)cr;
    }
    __syncthreads();
    for (int i = t; i < kJpegGroupBlocks * 64; i += kJpegLanes) {
        const int b = i >> 6, k = i & 63, r = k >> 3, c = k & 7;
        int s;
        if (sub) {
            const int m = b / 6, j = b - m * 6;
            if (j < 4) s = s_px[0][(j >> 1) * 8 + r][m * 16 + (j & 1) * 8 + c];
            else {
                const uint8_t* q = &s_px[j - 3][2 * r][m * 16 + 2 * c];
                s = (q[0] + q[1] + q[64] + q[65] + 2) >> 2;
            }
        } else {
            const int m = b / 3;
            s = s_px[b - m * 3][r][m * 8 + c];
        }
        s_blk[i] = s - 128;
    }
    __syncthreads();
    for (int pass = 0; pass < 2; ++pass) {
        if (t < kJpegGroupBlocks * 8) {
            const int at = (t >> 3) * 64 + (pass ? (t & 7) : (t & 7) * 8), step = pass ? 8 : 1;
            int v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = s_blk[at + k * step];
            jpeg_fdct_1d(v, pass);
#pragma unroll
            for (int k = 0; k < 8; ++k) s_blk[at + k * step] = v[k];
        }
        __syncthreads();
    }
    int16_t* out = f.coef + ((size_t)row * f.mcus_x + (size_t)gx * tm) * f.bpm * 64;
    for (int i = t; i < kJpegGroupBlocks * 64; i += kJpegLanes) {
        const int b = i >> 6, k = i & 63, m = b / f.bpm, j = b - m * f.bpm;
        if (gx * tm + m >= f.mcus_x) continue;                         // the last group of a row may hold fewer MCUs
        const int tc = sub ? (j >= 4) : (j > 0);
        out[i] = (int16_t)jpeg_quant(s_blk[b * 64 + tab->zigzag[k]], tab->q[tc][k]);
    }
}

struct JpegCount {
    unsigned bits = 0;
    __device__ void put(unsigned, int len) { bits += (unsigned)len; }
};
// ORs codes into big-endian words from bit `off` on.  A word the lane fills alone -- every one it completes after its first -- is stored;
// its first and its last word may hold its neighbours' bits and take atomicOr.
struct JpegEmit {
    uint32_t* w; unsigned long long acc = 0; int nb; bool first = true;
    __device__ JpegEmit(uint32_t* words, unsigned off) : w(words + (off >> 5)), nb((int)(off & 31u)) {}
    __device__ void put(unsigned code, int len) {
        acc |= (unsigned long long)code << (64 - nb - len);            // nb < 32 and len <= 26
        nb += len;
        if (nb >= 32) {
            const unsigned v = (unsigned)(acc >> 32);
            if (first) { atomicOr(w, v); first = false; } else *w = v;
            ++w; acc <<= 32; nb -= 32;
        }
    }
    __device__ void flush() { if (nb) atomicOr(w, (unsigned)(acc >> 32)); }
};

// exclusive scan of one value per lane over the block of 256 -> the lane's prefix; total = the block's sum (the same in every lane)
__device__ __forceinline__ unsigned jpeg_block_scan(unsigned v, unsigned* s_wave, unsigned& total) {
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    unsigned inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    __syncthreads();                                                   // the previous scan's s_wave has been read
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    unsigned before = 0; total = 0;
#pragma unroll
    for (int g = 0; g < 4; ++g) { const unsigned c = s_wave[g]; before += g < wave ? c : 0u; total += c; }
    return before + inc - v;
}

__global__ __launch_bounds__(256) void jpeg_code_kernel(const JpegFrame* __restrict__ frames, const JpegTables* __restrict__ tab) {
    const JpegFrame f = frames[blockIdx.y];
    const int seg = (int)blockIdx.x;
    if (seg >= f.mcus_y) return;                                       // block-uniform
    const int t = (int)threadIdx.x;

    __shared__ int16_t s_zz[kJpegLanes * kJpegZzRow];
    __shared__ uint16_t s_acc[2][256], s_dcc[2][12];
    __shared__ uint8_t s_acl[2][256], s_dcl[2][12];
    __shared__ unsigned s_wave[4];

    for (int i = t; i < 512; i += kJpegLanes) { s_acc[i >> 8][i & 255] = tab->ac_code[i >> 8][i & 255]; s_acl[i >> 8][i & 255] = tab->ac_len[i >> 8][i & 255]; }
    if (t < 24) { s_dcc[t / 12][t % 12] = tab->dc_code[t / 12][t % 12]; s_dcl[t / 12][t % 12] = tab->dc_len[t / 12][t % 12]; }

    const int nblk = f.mcus_x * f.bpm;
    const int16_t* coef = f.coef + (size_t)seg * nblk * 64;
    uint32_t* words = f.seg_words + (size_t)seg * f.seg_cap_words;
    unsigned base = 0;                                                 // bits of the chunks before this one; <= 24576 * 1660
    for (int c0 = 0; c0 < nblk; c0 += kJpegLanes) {
        const int nb = jpeg_min(kJpegLanes, nblk - c0);
        __syncthreads();                                               // the previous chunk's blocks have been coded (and the tables are in LDS)
        const uint32_t* src = reinterpret_cast<const uint32_t*>(coef + (size_t)c0 * 64);
        for (int i = t; i < nb * 32; i += kJpegLanes) {
            const uint32_t v = src[i];
            int16_t* d = s_zz + (i >> 5) * kJpegZzRow + (i & 31) * 2;
            d[0] = (int16_t)(v & 0xFFFFu); d[1] = (int16_t)(v >> 16);
        }
        __syncthreads();
        const bool live = t < nb;
        const int j = c0 + t, m = j / f.bpm, b = j - m * f.bpm;
        int tc, back; bool has;                                        // the component's previous block in the segment lies `back` blocks before this one
        if (f.bpm == 6) { tc = b >= 4; back = b == 0 ? 3 : b < 4 ? 1 : 6; has = m > 0 || (b >= 1 && b < 4); }
        else { tc = b > 0; back = 3; has = m > 0; }
        int pred = 0;
        if (live && has) pred = t >= back ? s_zz[(t - back) * kJpegZzRow] : coef[(size_t)(j - back) * 64];
        const int16_t* zz = s_zz + t * kJpegZzRow;
        JpegCount cnt;
        if (live) jpeg_code_block(zz, pred, s_dcc[tc], s_dcl[tc], s_acc[tc], s_acl[tc], cnt);
        unsigned total;
        const unsigned off = base + jpeg_block_scan(cnt.bits, s_wave, total);
        // zero the words this chunk begins in: the word it shares with the previous chunk already holds that chunk's bits
        for (unsigned w = ((base + 31u) >> 5) + (unsigned)t; w <= (base + total - 1u) >> 5; w += kJpegLanes) words[w] = 0u;
        __syncthreads();
        if (live) {
            JpegEmit e(words, off);
            jpeg_code_block(zz, pred, s_dcc[tc], s_dcl[tc], s_acc[tc], s_acl[tc], e);
            e.flush();
        }
        base += total;
    }
    // pad the last byte with 1-bits; then every lane's bits are in memory and the segment's 0xFF bytes can be counted
    const unsigned nbytes = (base + 7u) >> 3, npad = nbytes * 8u - base;
    if (t == 0 && npad) atomicOr(words + (base >> 5), ((1u << npad) - 1u) << (32u - (base & 31u) - npad));
    __threadfence();
    __syncthreads();
    unsigned ff = 0;
    for (unsigned w = (unsigned)t; w * 4u < nbytes; w += kJpegLanes) {
        const unsigned v = __hip_atomic_load(words + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // past this lane's L1: other lanes' atomics live in L2
        const unsigned nv = nbytes - w * 4u < 4u ? nbytes - w * 4u : 4u;
        for (unsigned k = 0; k < nv; ++k) ff += ((v >> (24u - 8u * k)) & 0xFFu) == 0xFFu;
    }
    unsigned total_ff;
    (void)jpeg_block_scan(ff, s_wave, total_ff);
    if (t == 0) { f.seg_info[2 * seg] = nbytes; f.seg_info[2 * seg + 1] = total_ff; }
}

__global__ __launch_bounds__(256) void jpeg_pack_kernel(const JpegFrame* __restrict__ frames) {
    const JpegFrame f = frames[blockIdx.y];
    const int seg = (int)blockIdx.x;
    if (seg >= f.mcus_y) return;                                       // block-uniform
    const int t = (int)threadIdx.x;
    __shared__ unsigned s_wave[4];
    __shared__ unsigned long long s_sum[kJpegLanes];

    unsigned long long mine = 0;
    for (int s = t; s < seg; s += kJpegLanes) mine += (unsigned long long)f.seg_info[2 * s] + f.seg_info[2 * s + 1];
    s_sum[t] = mine;
    __syncthreads();
    for (int d = kJpegLanes / 2; d > 0; d >>= 1) {
        if (t < d) s_sum[t] += s_sum[t + d];
        __syncthreads();
    }
    const unsigned long long start = (unsigned long long)f.hdr_len + s_sum[0] + 2ull * (unsigned)seg;
    if (seg == 0) for (int i = t; i < f.hdr_len; i += kJpegLanes) f.out[i] = f.hdr[i];
    if (seg > 0 && t == 0) { f.out[start - 2] = 0xFF; f.out[start - 1] = (uint8_t)(0xD0 + ((seg - 1) & 7)); }

    const unsigned nbytes = f.seg_info[2 * seg];
    const uint32_t* words = f.seg_words + (size_t)seg * f.seg_cap_words;
    unsigned long long ff_before = 0;
    for (unsigned w0 = 0; w0 * 4u < nbytes; w0 += kJpegLanes) {
        const unsigned w = w0 + (unsigned)t;
        const unsigned nv = w * 4u >= nbytes ? 0u : nbytes - w * 4u < 4u ? nbytes - w * 4u : 4u;
        const unsigned v = nv ? words[w] : 0u;
        unsigned ff = 0;
        for (unsigned k = 0; k < nv; ++k) ff += ((v >> (24u - 8u * k)) & 0xFFu) == 0xFFu;
        unsigned total;
        const unsigned ex = jpeg_block_scan(ff, s_wave, total);
        uint8_t* o = f.out + start + (unsigned long long)w * 4u + ff_before + ex;
        for (unsigned k = 0; k < nv; ++k) {
            const uint8_t byte = (uint8_t)(v >> (24u - 8u * k));
            *o++ = byte;
            if (byte == 0xFF) *o++ = 0;
        }
        ff_before += total;
    }
    if (seg == f.mcus_y - 1 && t == 0) {
        const unsigned long long end = start + nbytes + ff_before;
        f.out[end] = 0xFF; f.out[end + 1] = 0xD9;
        *f.len = (long long)(end + 2);
    }
}

constexpr size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

// ---- one call: checks, the work buffer's layout, staging of host frames, the launches, the copy back -----------------------------------
static int jpeg_check(const mi355_render_frame* frames, int n, int quality, int subsampling, bool host_only) {
    if (!frames) return fail(MI355_EINVAL, "jpeg: null argument");
    if (n < 1 || n > MI355_RENDER_MAX_FRAMES) return fail(MI355_EINVAL, "jpeg: n must be in [1, " + std::to_string(MI355_RENDER_MAX_FRAMES) + "]");
    if (quality < 1 || quality > 100) return fail(MI355_EINVAL, "jpeg: quality must be in [1, 100], got " + std::to_string(quality));
    if (subsampling != kJpeg420 && subsampling != kJpeg444)
        return fail(MI355_EINVAL, "jpeg: subsampling must be MI355_JPEG_420 (420) or MI355_JPEG_444 (444), got " + std::to_string(subsampling));
    for (int i = 0; i < n; ++i) {
        const mi355_render_frame& f = frames[i];
        const std::string at = "jpeg: frames[" + std::to_string(i) + "]: ";
        if (!f.data) return fail(MI355_EINVAL, at + "the frame pointer is null");
        if (f.height < 1 || f.height > kJpegMaxSide) return fail(MI355_EINVAL, at + "height must be in [1, 65535], got " + std::to_string(f.height));
        if (f.width < 1 || f.width > kJpegMaxSide) return fail(MI355_EINVAL, at + "width must be in [1, 65535], got " + std::to_string(f.width));
        if ((long long)f.row_stride < 3ll * f.width) return fail(MI355_EINVAL, at + "row_stride is smaller than a row");
        if ((long long)f.height * f.row_stride >= (1ll << 31)) return fail(MI355_EINVAL, at + "a frame must be smaller than 2 GiB");
        if (host_only && f.on_device) return fail(MI355_EINVAL, at + "the host twin (device -1) takes host memory");
    }
    return MI355_OK;
}

static JpegFrame jpeg_desc(const mi355_render_frame& f, int subsampling) {
    JpegFrame d{};
    d.src = f.data; d.H = f.height; d.W = f.width; d.pitch = f.row_stride;
    jpeg_geometry(d, subsampling);
    return d;
}

// outs != NULL: the streams; coefs != NULL: the transform stage alone, int16 [blocks][64] per frame
int jpeg_run(JpegCtx& ctx, int device, const mi355_render_frame* frames, int n, int quality, int subsampling, mi355_jpeg_out* outs,
             int16_t* const* coefs, hipStream_t st, float* launch_ms) {
    int rc = jpeg_check(frames, n, quality, subsampling, device < 0); if (rc) return rc;
    if (!outs && !coefs) return fail(MI355_EINVAL, "jpeg: null output");
    for (int i = 0; i < n; ++i) {
        const std::string at = "jpeg: outs[" + std::to_string(i) + "]: ";
        if (outs && !outs[i].data) return fail(MI355_EINVAL, at + "the data pointer is null");
        if (outs && outs[i].capacity < jpeg_bound(frames[i].height, frames[i].width, subsampling))
            return fail(MI355_EINVAL, at + "capacity " + std::to_string(outs[i].capacity) + " is below mi355_jpeg_bound = " +
                                          std::to_string(jpeg_bound(frames[i].height, frames[i].width, subsampling)) + "; nothing was written");
        if (coefs && !coefs[i]) return fail(MI355_EINVAL, at + "the coefficient pointer is null");
    }
    if (launch_ms) *launch_ms = 0.f;
    JpegTables tab;
    jpeg_make_tables(quality, tab);
    std::vector<JpegFrame> desc((size_t)n);
    for (int i = 0; i < n; ++i) desc[i] = jpeg_desc(frames[i], subsampling);
    if (device < 0) {
        for (int i = 0; i < n; ++i) {
            if (coefs) jpeg_coefficients_host(desc[i], tab, coefs[i]);
            if (outs) { desc[i].out = outs[i].data; outs[i].length = jpeg_encode_host(desc[i], tab); }
        }
        return MI355_OK;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return fail(MI355_EHIP, "no HIP device: the JPEG kernels need an MI355X (device = -1 runs their host twin)"); }
    if (device >= ndev) return fail(MI355_EINVAL, "jpeg: device out of range");
    HIPCHK(hipSetDevice(device));
    // the work buffer: [descriptors | tables | lengths | headers] (the pinned image's part) then per frame [coefficients | segment
    // words | segment sizes | stream] and the staged host frames
    const size_t tab_off = al256((size_t)n * sizeof(JpegFrame)), len_off = al256(tab_off + sizeof(JpegTables));
    const size_t hdr_off = al256(len_off + (size_t)n * 8), img_bytes = hdr_off + (size_t)n * kJpegHeaderMax;
    size_t at = al256(img_bytes);
    std::vector<size_t> coef_off((size_t)n), seg_off((size_t)n), info_off((size_t)n), out_off((size_t)n), src_off((size_t)n, 0), blocks((size_t)n);
    for (int i = 0; i < n; ++i) {
        JpegFrame& d = desc[i];
        blocks[i] = (size_t)d.mcus_x * d.mcus_y * d.bpm;
        d.seg_cap_words = ((size_t)d.mcus_x * d.bpm * kJpegBlockBits + 31) / 32 + 2;
        coef_off[i] = at; at = al256(at + blocks[i] * 128);
        if (outs) {
            seg_off[i] = at; at = al256(at + d.seg_cap_words * 4 * d.mcus_y);
            info_off[i] = at; at = al256(at + (size_t)d.mcus_y * 8);
            out_off[i] = at; at = al256(at + (size_t)jpeg_bound(d.H, d.W, subsampling));
        }
        if (!frames[i].on_device) { src_off[i] = at; at = al256(at + (size_t)(d.H - 1) * d.pitch + (size_t)d.W * 3); }
    }
    if (buf_grow(ctx.d_work, at, at + at / 4) < 0 || buf_grow(ctx.h_img, img_bytes, img_bytes + img_bytes / 4) < 0)
        return fail(MI355_EHIP, "jpeg: out of device or pinned memory (" + std::to_string(at) + " bytes of scratch)");
    uint8_t* base = ctx.d_work.p;
    int most_g = 1, most_s = 1;
    for (int i = 0; i < n; ++i) {
        JpegFrame& d = desc[i];
        d.coef = (int16_t*)(base + coef_off[i]);
        if (outs) {
            d.seg_words = (uint32_t*)(base + seg_off[i]); d.seg_info = (uint32_t*)(base + info_off[i]); d.out = base + out_off[i];
            d.len = (long long*)(base + len_off) + i; d.hdr = base + hdr_off + (size_t)i * kJpegHeaderMax;
            d.hdr_len = jpeg_write_header(tab, d, ctx.h_img.p + hdr_off + (size_t)i * kJpegHeaderMax);
        }
        if (!frames[i].on_device) {
            d.src = base + src_off[i];
            HIPCHK(hipMemcpyAsync(base + src_off[i], frames[i].data, (size_t)(d.H - 1) * d.pitch + (size_t)d.W * 3, hipMemcpyHostToDevice, st));
        }
        const int tm = d.bpm == 6 ? 4 : 8;
        const long long groups = (long long)((d.mcus_x + tm - 1) / tm) * d.mcus_y;
        if (groups > 0x7FFFFFFFll) return fail(MI355_EINVAL, "jpeg: frames[" + std::to_string(i) + "]: too many MCU groups for one launch");
        most_g = std::max(most_g, (int)groups); most_s = std::max(most_s, d.mcus_y);
    }
    std::memcpy(ctx.h_img.p, desc.data(), (size_t)n * sizeof(JpegFrame));
    std::memcpy(ctx.h_img.p + tab_off, &tab, sizeof(JpegTables));
    std::memset(ctx.h_img.p + len_off, 0, (size_t)n * 8);
    HIPCHK(hipMemcpyAsync(base, ctx.h_img.p, img_bytes, hipMemcpyHostToDevice, st));
    if (launch_ms && !ctx.ev0) { HIPCHK(hipEventCreate(&ctx.ev0)); HIPCHK(hipEventCreate(&ctx.ev1)); }
    if (launch_ms) HIPCHK(hipEventRecord(ctx.ev0, st));
    const JpegFrame* dd = (const JpegFrame*)base;
    const JpegTables* dt = (const JpegTables*)(base + tab_off);
    auto launched = [&]() -> const char* { const hipError_t e = hipGetLastError(); return e != hipSuccess ? hipGetErrorString(e) : nullptr; };
    hipLaunchKernelGGL(jpeg_transform_kernel, dim3((unsigned)most_g, (unsigned)n), dim3(kJpegLanes), 0, st, dd, dt);
    KCHK(launched());
    if (outs) {
        hipLaunchKernelGGL(jpeg_code_kernel, dim3((unsigned)most_s, (unsigned)n), dim3(kJpegLanes), 0, st, dd, dt);
        KCHK(launched());
        hipLaunchKernelGGL(jpeg_pack_kernel, dim3((unsigned)most_s, (unsigned)n), dim3(kJpegLanes), 0, st, dd);
        KCHK(launched());
    }
    if (launch_ms) HIPCHK(hipEventRecord(ctx.ev1, st));
    if (coefs) {
        for (int i = 0; i < n; ++i) HIPCHK(hipMemcpyAsync(coefs[i], desc[i].coef, blocks[i] * 128, hipMemcpyDeviceToHost, st));
    }
    if (outs) {
        // the lengths first, then only the streams' bytes, through pinned memory
        if (buf_grow(ctx.h_len, (size_t)n * 8) < 0) return fail(MI355_EHIP, "jpeg: out of pinned memory");
        HIPCHK(hipMemcpyAsync(ctx.h_len.p, base + len_off, (size_t)n * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        const long long* lens = (const long long*)ctx.h_len.p;
        std::vector<size_t> back((size_t)n);
        size_t back_bytes = 0;
        for (int i = 0; i < n; ++i) {
            if (lens[i] < desc[i].hdr_len + 2 || lens[i] > jpeg_bound(desc[i].H, desc[i].W, subsampling))
                return fail(MI355_EHIP, "jpeg: frame " + std::to_string(i) + ": the kernels reported an impossible length " + std::to_string(lens[i]));
            back[i] = back_bytes; back_bytes = al256(back_bytes + (size_t)lens[i]);
        }
        if (buf_grow(ctx.h_out, back_bytes, back_bytes + back_bytes / 4) < 0) return fail(MI355_EHIP, "jpeg: out of pinned memory");
        for (int i = 0; i < n; ++i) HIPCHK(hipMemcpyAsync(ctx.h_out.p + back[i], desc[i].out, (size_t)lens[i], hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (int i = 0; i < n; ++i) { std::memcpy(outs[i].data, ctx.h_out.p + back[i], (size_t)lens[i]); outs[i].length = lens[i]; }
    } else {
        HIPCHK(hipStreamSynchronize(st));
    }
    if (launch_ms) HIPCHK(hipEventElapsedTime(launch_ms, ctx.ev0, ctx.ev1));
    return MI355_OK;
}

void jpeg_ctx_free(JpegCtx& ctx) {
    buf_free(ctx.d_work); buf_free(ctx.h_img); buf_free(ctx.h_out); buf_free(ctx.h_len);
    if (ctx.ev0) { (void)hipEventDestroy(ctx.ev0); (void)hipEventDestroy(ctx.ev1); ctx.ev0 = ctx.ev1 = nullptr; }
}

}  // namespace mi355
