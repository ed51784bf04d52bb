// Motion gate for YOLO.track_cameras (include/mi355_yolo.h "motion gate"): a block-luma grid per camera, compared with
// the grid of the last frame that ran the detector.  ONE launch per tick for all present cameras, descriptor-driven like
// letterbox_multi_kernel and the gmc_multi kernels; the per-group routine and the changed test are motion_grid.h, which the host twin
// (device -1) runs in plain loops.  Integer arithmetic only.
//
// Work item = one wavefront = one (camera, block-row strip).  Lane (rsub, gl) = (lane >> 4, lane & 15) sums the 16-pixel groups
// g0 + gl of rows y0 + rsub, y0 + rsub + 4, ...: sixteen neighbouring lanes read 256 (Y) or 768 (BGR) consecutive bytes of a row, each
// pixel once.  A camera whose rows all start 16-byte aligned takes motion_rows_vec (every load of an iteration in flight at once).
// The four row subsets meet through two shuffles, the two groups of a 32-pixel block through one more, the strip's changed-block
// count through six: no LDS, no atomics, one uint32 per strip for the host to add.
#include "engine_internal.h"
#include "motion_grid.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace mi355 {

// The descriptor's pointers are global memory; held in these types, the loads and stores are global_* rather than flat_* instructions
// (a pointer read from memory is generic to the compiler).
#define MI355_GLOBAL __attribute__((address_space(1)))
typedef MI355_GLOBAL const uint8_t* motion_gsrc;

// A lane's R rows of one full group of a camera whose every row starts 16-byte aligned: all R * BPP 16-byte loads are issued before the
// first sum needs one (a row beyond the strip's last re-reads row y0 and adds nothing), so a wave keeps up to 12 loads per lane in flight.
template <int BPP, int R>
__device__ __forceinline__ void motion_rows_vec(motion_gsrc col, int row_stride, int y0, int y1, int rsub, unsigned& lo, unsigned& hi) {
    mi355_u32x4 v[R][BPP];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int y = y0 + rsub + 4 * r;
        MI355_GLOBAL const mi355_u32x4* q = (MI355_GLOBAL const mi355_u32x4*)(col + (unsigned)(y < y1 ? y : y0) * (unsigned)row_stride);
#pragma unroll
        for (int j = 0; j < BPP; ++j) v[r][j] = q[j];
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        unsigned l = 0, h = 0, w[4 * BPP];
#pragma unroll
        for (int j = 0; j < BPP; ++j) { w[4 * j] = v[r][j].x; w[4 * j + 1] = v[r][j].y; w[4 * j + 2] = v[r][j].z; w[4 * j + 3] = v[r][j].w; }
        motion_sums_words(w, BPP, l, h);
        const bool ok = y0 + rsub + 4 * r < y1;
        lo += ok ? l : 0u; hi += ok ? h : 0u;
    }
}

__global__ __launch_bounds__(256) void motion_grid_kernel(const MotionCam* __restrict__ cams, int n_cams, int total_strips, int block,
                                                          unsigned level_q, unsigned* __restrict__ partial) {
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * 256u + threadIdx.x) >> 6));
    if (wave >= total_strips) return;                          // wave-uniform: whole waves leave
    int ci = 0;
    while (ci + 1 < n_cams && cams[ci + 1].strip0 <= wave) ++ci;
    const MotionCam c = cams[ci];
    const motion_gsrc src = (motion_gsrc)c.src;
    MI355_GLOBAL unsigned* const cur = (MI355_GLOBAL unsigned*)c.cur;
    MI355_GLOBAL const unsigned* const ref = (MI355_GLOBAL const unsigned*)c.ref;
    MI355_GLOBAL uint8_t* const flags = (MI355_GLOBAL uint8_t*)c.flags;
    const int by = wave - c.strip0;
    const int y0 = by * block, y1 = min(c.H, y0 + block), bh = y1 - y0;
    const int ng = (c.W + kMotionGroup - 1) / kMotionGroup;
    const int rsub = lane >> 4, gl = lane & 15;
    const bool vec = (((unsigned)(uintptr_t)src | (unsigned)c.row_stride) & 15u) == 0;      // wave-uniform: every row of this camera is 16-byte aligned
    unsigned count = 0;
    auto emit = [&](int bx, unsigned s, int bw) {
        const int idx = by * c.gw + bx;
        const unsigned f = ref ? motion_block_changed(s, ref[idx], level_q, (unsigned)(bw * bh)) : 1u;
        cur[idx] = s;
        flags[idx] = (uint8_t)f;
        count += f;
    };
    for (int g0 = 0; g0 < ng; g0 += 16) {
        const int g = g0 + gl;
        unsigned lo = 0, hi = 0;
        if (g < ng) {
            const int npix = min(kMotionGroup, c.W - kMotionGroup * g);
            const motion_gsrc col = src + (unsigned)(g * kMotionGroup * c.bpp);
            if (vec && npix == kMotionGroup) {
                if (c.bpp == 1) {
                    if (block == 8) motion_rows_vec<1, 2>(col, c.row_stride, y0, y1, rsub, lo, hi);
                    else if (block == 16) motion_rows_vec<1, 4>(col, c.row_stride, y0, y1, rsub, lo, hi);
                    else {
                        motion_rows_vec<1, 4>(col, c.row_stride, y0, y1, rsub, lo, hi);
                        if (y0 + 16 < y1) motion_rows_vec<1, 4>(col, c.row_stride, y0 + 16, y1, rsub, lo, hi);
                    }
                } else {
                    if (block == 8) motion_rows_vec<3, 2>(col, c.row_stride, y0, y1, rsub, lo, hi);
                    else if (block == 16) motion_rows_vec<3, 4>(col, c.row_stride, y0, y1, rsub, lo, hi);
                    else {                                     // 32 rows: two halves of 16, half the registers
                        motion_rows_vec<3, 4>(col, c.row_stride, y0, y1, rsub, lo, hi);
                        if (y0 + 16 < y1) motion_rows_vec<3, 4>(col, c.row_stride, y0 + 16, y1, rsub, lo, hi);
                    }
                }
            } else {                                           // a partial last group, or rows that are not all aligned: row by row (motion_grid.h)
                motion_gsrc p = col + (unsigned)(y0 + rsub) * (unsigned)c.row_stride;
                for (int r = y0 + rsub; r < y1; r += 4, p += 4 * c.row_stride) motion_group_sums((const uint8_t*)p, c.bpp, npix, lo, hi);
            }
        }
        lo += __shfl_xor(lo, 16); lo += __shfl_xor(lo, 32);
        hi += __shfl_xor(hi, 16); hi += __shfl_xor(hi, 32);
        const unsigned s16 = lo + hi;
        const unsigned s32 = s16 + __shfl_xor(s16, 1);         // g0 is a multiple of 16: groups 2b and 2b + 1 sit in lanes gl, gl ^ 1
        if (rsub == 0 && g < ng) {
            if (block == 8) {
                emit(2 * g, lo, min(8, c.W - 16 * g));
                if (2 * g + 1 < c.gw) emit(2 * g + 1, hi, min(8, c.W - 16 * g - 8));
            } else if (block == 16) {
                emit(g, s16, min(16, c.W - 16 * g));
            } else if ((gl & 1) == 0) {
                emit(g >> 1, s32, min(32, c.W - 16 * g));
            }
        }
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) count += __shfl_xor(count, m);
    if (lane == 0) partial[wave] = count;
}

const char* launch_motion_grid(const MotionCam* cams_dev, int n_cams, int total_strips, int block, unsigned level_q, unsigned* partial_dev,
                               hipStream_t st) {
    if (n_cams <= 0 || total_strips <= 0) return nullptr;
    hipLaunchKernelGGL(motion_grid_kernel, dim3((unsigned)((total_strips + 3) / 4)), dim3(256), 0, st, cams_dev, n_cams, total_strips, block,
                       level_q, partial_dev);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

namespace {

// the host twin: the same group routine and the same test, strip by strip; -> the camera's changed blocks
unsigned motion_grid_host(const MotionCam& c, int block, unsigned level_q) {
    const int ng = (c.W + kMotionGroup - 1) / kMotionGroup;
    unsigned count = 0;
    for (int by = 0; by < c.gh; ++by) {
        const int y0 = by * block, y1 = std::min(c.H, y0 + block), bh = y1 - y0;
        unsigned* row = c.cur + (size_t)by * c.gw;
        std::fill(row, row + c.gw, 0u);
        for (int g = 0; g < ng; ++g) {
            unsigned lo = 0, hi = 0;
            const int npix = std::min(kMotionGroup, c.W - kMotionGroup * g);
            for (int r = y0; r < y1; ++r) motion_group_sums(c.src + (size_t)r * c.row_stride + (size_t)g * kMotionGroup * c.bpp, c.bpp, npix, lo, hi);
            if (block == 8) { row[2 * g] += lo; if (2 * g + 1 < c.gw) row[2 * g + 1] += hi; }
            else row[block == 16 ? g : g >> 1] += lo + hi;
        }
        for (int bx = 0; bx < c.gw; ++bx) {
            const int idx = by * c.gw + bx, bw = std::min(block, c.W - bx * block);
            const unsigned f = c.ref ? motion_block_changed(row[bx], c.ref[idx], level_q, (unsigned)(bw * bh)) : 1u;
            c.flags[idx] = (uint8_t)f;
            count += f;
        }
    }
    return count;
}

struct GateCam {
    int h = 0, w = 0, bpp = 0, gh = 0, gw = 0;
    bool have_ref = false, have_mask = false;
    int static_run = 0, slot = 0;                              // sums[slot] is the reference, sums[slot ^ 1] receives the current grid
    size_t cells = 0;
    Buf d;                                                     // device object: [sums 0 | sums 1 | flags], cells each
    std::vector<unsigned> hs[2]; std::vector<uint8_t> hf;      // host object
    unsigned* sums(int s, bool host) { return host ? hs[s].data() : (unsigned*)d.p + (size_t)s * cells; }
    uint8_t* flags(bool host) { return host ? hf.data() : d.p + 8 * cells; }
};

constexpr size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace
}  // namespace mi355

using namespace mi355;

struct mi355_motion_gate {
    int device = -1, n = 0, block = 16, min_blocks = 4, max_skip = 30; unsigned level_q = 32; bool host = true;
    std::vector<GateCam> cams;
    hipStream_t stream = nullptr;
    Buf d_in, h_in{true};                                      // host frames of a tick: staged with the caller's pitch, ONE upload
    Buf d_desc, h_desc{true}, d_part, h_part{true};
};

extern "C" int mi355_motion_gate_create(int device, int n_cameras, const mi355_motion_opts* opts, mi355_motion_gate** out) {
    if (!out) return fail(MI355_EINVAL, "motion gate: out is null");
    *out = nullptr;
    mi355_motion_opts o{(int)sizeof(mi355_motion_opts), 16, 2.0f, 4, 30};
    if (opts) {
        if (opts->struct_size != (int)sizeof(mi355_motion_opts)) return fail(MI355_EINVAL, "motion gate: opts.struct_size does not match this library");
        o = *opts;
    }
    if (device < -1) return fail(MI355_EINVAL, "motion gate: device must be -1 (host) or a GPU index");
    if (n_cameras < 1 || n_cameras > MI355_MOTION_MAX_CAMERAS) return fail(MI355_EINVAL, "motion gate: n_cameras must be in [1, 64]");
    if (o.block != 8 && o.block != 16 && o.block != 32) return fail(MI355_EINVAL, "motion gate: block must be 8, 16 or 32");
    if (!(o.level >= 0.f && o.level <= 255.f)) return fail(MI355_EINVAL, "motion gate: level must be in [0, 255]");
    if (o.min_blocks < 0) return fail(MI355_EINVAL, "motion gate: min_blocks must be >= 0");
    mi355_motion_gate* g = new mi355_motion_gate();
    g->device = device; g->host = device == -1; g->n = n_cameras; g->block = o.block; g->min_blocks = o.min_blocks;
    g->max_skip = o.max_skip < 0 ? -1 : o.max_skip;
    g->level_q = (unsigned)std::floor(16.0 * (double)o.level + 0.5);
    g->cams.resize((size_t)n_cameras);
    if (!g->host) {
        hipError_t e = hipSetDevice(device);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking);
        if (e != hipSuccess) { (void)hipGetLastError(); delete g; return fail(MI355_EHIP, std::string("motion gate: ") + hipGetErrorString(e)); }
    }
    *out = g;
    return MI355_OK;
}

extern "C" void mi355_motion_gate_destroy(mi355_motion_gate* g) {
    if (!g) return;
    if (!g->host) {
        (void)hipSetDevice(g->device);
        if (g->stream) { (void)hipStreamSynchronize(g->stream); (void)hipStreamDestroy(g->stream); }
        for (GateCam& c : g->cams) buf_free(c.d);
        for (Buf* b : {&g->d_in, &g->h_in, &g->d_desc, &g->h_desc, &g->d_part, &g->h_part}) buf_free(*b);
    }
    delete g;
}

extern "C" int mi355_motion_gate_reset(mi355_motion_gate* g, int camera) {
    if (!g || camera < -1 || camera >= g->n) return fail(MI355_EINVAL, "motion gate reset: camera out of range");
    for (int i = 0; i < g->n; ++i)
        if (camera < 0 || i == camera) { g->cams[i].have_ref = false; g->cams[i].static_run = 0; }
    return MI355_OK;
}

extern "C" int mi355_motion_gate_update(mi355_motion_gate* g, const mi355_motion_frame* const* frames, int frames_on_device, int* moving,
                                        int* changed) {
    if (!g || !frames || !moving || !changed) return fail(MI355_EINVAL, "motion gate update: null argument");
    if (g->host && frames_on_device) return fail(MI355_EINVAL, "motion gate update: a host gate (device -1) takes host frames");
    // every frame is checked before anything is touched
    std::vector<int> present;
    for (int i = 0; i < g->n; ++i) {
        const mi355_motion_frame* f = frames[i];
        if (!f) continue;
        if (!f->data) return fail(MI355_EINVAL, "motion gate update: data is null (an absent camera is a NULL descriptor)");
        if (f->height <= 0 || f->width <= 0) return fail(MI355_EINVAL, "motion gate update: height and width must be positive");
        if (f->bytes_per_pixel != 1 && f->bytes_per_pixel != 3) return fail(MI355_EINVAL, "motion gate update: bytes_per_pixel must be 3 (BGR) or 1 (a Y plane)");
        if ((long long)f->row_stride < (long long)f->width * f->bytes_per_pixel) return fail(MI355_EINVAL, "motion gate update: row_stride is smaller than a row");
        if ((long long)f->height * f->row_stride >= (1ll << 31)) return fail(MI355_EINVAL, "motion gate update: a frame must be smaller than 2 GiB (32-bit offsets)");
        present.push_back(i);
    }
    for (int i = 0; i < g->n; ++i) { moving[i] = 0; changed[i] = -1; }
    const int np = (int)present.size();
    if (!np) return MI355_OK;
    if (!g->host) HIPCHK(hipSetDevice(g->device));
    // geometry; a camera whose size, format (or first frame) is new loses its reference
    std::vector<MotionCam> desc((size_t)np);
    int strips = 0; size_t in_bytes = 0;
    std::vector<size_t> in_off((size_t)np, 0);
    for (int k = 0; k < np; ++k) {
        const mi355_motion_frame& f = *frames[present[k]];
        GateCam& c = g->cams[present[k]];
        if (c.h != f.height || c.w != f.width || c.bpp != f.bytes_per_pixel) {
            c.h = f.height; c.w = f.width; c.bpp = f.bytes_per_pixel; c.have_ref = false;
            c.gh = (f.height + g->block - 1) / g->block; c.gw = (f.width + g->block - 1) / g->block;
            const size_t cells = (size_t)c.gh * c.gw;
            if (g->host) { c.hs[0].assign(cells, 0u); c.hs[1].assign(cells, 0u); c.hf.assign(cells, 0); }
            else if (c.d.cap < 9 * cells) {                     // no launch is in flight: every update ends behind its stream
                if (buf_grow(c.d, 9 * cells) < 0) { c.h = c.w = c.bpp = 0; c.have_mask = false; return fail(MI355_EHIP, "motion gate: out of device memory"); }
            }
            c.cells = cells; c.have_mask = false;
        }
        MotionCam& d = desc[k];
        d.src = f.data; d.H = f.height; d.W = f.width; d.row_stride = f.row_stride; d.bpp = f.bytes_per_pixel;
        d.gh = c.gh; d.gw = c.gw; d.strip0 = strips; d.pad_ = 0;
        d.cur = c.sums(c.slot ^ 1, g->host); d.ref = c.have_ref ? c.sums(c.slot, g->host) : nullptr; d.flags = c.flags(g->host);
        strips += c.gh;
        if (!g->host && !frames_on_device) {                   // staged where the caller's address sits modulo 16: the frame takes the path it would take in place
            in_off[k] = al256(in_bytes) + ((uintptr_t)f.data & 15u);
            in_bytes = in_off[k] + (size_t)(f.height - 1) * f.row_stride + (size_t)f.width * f.bytes_per_pixel;
        }
    }
    std::vector<unsigned> counts((size_t)np, 0u);
    if (g->host) {
        for (int k = 0; k < np; ++k) counts[k] = motion_grid_host(desc[k], g->block, g->level_q);
    } else {
        if (in_bytes) {
            if (buf_grow(g->h_in, in_bytes, in_bytes + in_bytes / 4) < 0 || buf_grow(g->d_in, in_bytes, in_bytes + in_bytes / 4) < 0)
                return fail(MI355_EHIP, "motion gate: out of device or pinned memory");
            for (int k = 0; k < np; ++k) {
                const size_t bytes = (size_t)(desc[k].H - 1) * desc[k].row_stride + (size_t)desc[k].W * desc[k].bpp;
                std::memcpy(g->h_in.p + in_off[k], desc[k].src, bytes);
                desc[k].src = g->d_in.p + in_off[k];
            }
            HIPCHK(hipMemcpyAsync(g->d_in.p, g->h_in.p, in_bytes, hipMemcpyHostToDevice, g->stream));
        }
        const size_t desc_bytes = (size_t)np * sizeof(MotionCam), part_bytes = (size_t)strips * 4;
        if (buf_grow(g->h_desc, desc_bytes, (size_t)MI355_MOTION_MAX_CAMERAS * sizeof(MotionCam)) < 0 ||
            buf_grow(g->d_desc, desc_bytes, (size_t)MI355_MOTION_MAX_CAMERAS * sizeof(MotionCam)) < 0 ||
            buf_grow(g->h_part, part_bytes, 2 * part_bytes) < 0 || buf_grow(g->d_part, part_bytes, 2 * part_bytes) < 0)
            return fail(MI355_EHIP, "motion gate: out of device or pinned memory");
        std::memcpy(g->h_desc.p, desc.data(), desc_bytes);
        HIPCHK(hipMemcpyAsync(g->d_desc.p, g->h_desc.p, desc_bytes, hipMemcpyHostToDevice, g->stream));
        KCHK(launch_motion_grid((const MotionCam*)g->d_desc.p, np, strips, g->block, g->level_q, (unsigned*)g->d_part.p, g->stream));
        HIPCHK(hipMemcpyAsync(g->h_part.p, g->d_part.p, part_bytes, hipMemcpyDeviceToHost, g->stream));
        HIPCHK(hipStreamSynchronize(g->stream));
        const unsigned* part = (const unsigned*)g->h_part.p;
        for (int k = 0; k < np; ++k)
            for (int s = 0; s < desc[k].gh; ++s) counts[k] += part[desc[k].strip0 + s];
    }
    // the state rules (include/mi355_yolo.h)
    for (int k = 0; k < np; ++k) {
        const int i = present[k];
        GateCam& c = g->cams[i];
        const bool mv = !c.have_ref || (int)counts[k] >= g->min_blocks || (g->max_skip >= 0 && c.static_run >= g->max_skip);
        changed[i] = (int)counts[k]; moving[i] = mv ? 1 : 0;
        c.have_mask = true;
        if (mv) { c.slot ^= 1; c.have_ref = true; c.static_run = 0; }     // the current grid becomes the reference: a pointer swap
        else ++c.static_run;
    }
    return MI355_OK;
}

namespace {
int gate_fetch(mi355_motion_gate* g, const void* src, void* dst, size_t bytes) {
    if (g->host) { std::memcpy(dst, src, bytes); return MI355_OK; }
    HIPCHK(hipSetDevice(g->device));
    HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return MI355_OK;
}
}  // namespace

extern "C" int mi355_motion_gate_mask(mi355_motion_gate* g, int camera, uint8_t* flags_out, int cap, int* gh, int* gw) {
    if (!g || camera < 0 || camera >= g->n || !gh || !gw) return fail(MI355_EINVAL, "motion gate mask: bad argument");
    GateCam& c = g->cams[camera];
    *gh = c.have_mask ? c.gh : 0; *gw = c.have_mask ? c.gw : 0;
    if (!flags_out || !c.have_mask) return MI355_OK;
    if ((long long)cap < (long long)c.gh * c.gw) return fail(MI355_EINVAL, "motion gate mask: cap is smaller than gh * gw");
    return gate_fetch(g, c.flags(g->host), flags_out, c.cells);
}

extern "C" int mi355_op_motion_grid(int device, const mi355_motion_frame* frames, int n, int block, uint32_t* const* sums_out) {
    if (!frames || !sums_out || n < 1 || n > MI355_MOTION_MAX_CAMERAS) return fail(MI355_EINVAL, "motion grid: n must be in [1, 64]");
    for (int i = 0; i < n; ++i) if (!sums_out[i]) return fail(MI355_EINVAL, "motion grid: an output pointer is null");
    mi355_motion_opts o{(int)sizeof(mi355_motion_opts), block, 2.0f, 4, 30};
    mi355_motion_gate* g = nullptr;
    int rc = mi355_motion_gate_create(device, n, &o, &g);
    if (rc) return rc;
    std::vector<const mi355_motion_frame*> fp((size_t)n);
    for (int i = 0; i < n; ++i) fp[i] = frames + i;
    std::vector<int> mv((size_t)n), ch((size_t)n);
    rc = mi355_motion_gate_update(g, fp.data(), 0, mv.data(), ch.data());
    for (int i = 0; i < n && !rc; ++i) {                        // a first frame always moves: its grid is now the reference
        GateCam& c = g->cams[i];
        rc = gate_fetch(g, c.sums(c.slot, g->host), sums_out[i], c.cells * 4);
    }
    mi355_motion_gate_destroy(g);
    return rc;
}
