// Person crops: ONE descriptor-driven launch cuts and resamples every rectangle of every frame of a call.
//   blocks   crop k owns the blocks [blk0_k, blk0_k+1): a block finds its crop by a binary search over the descriptors' blk0 with its
//            (wave-uniform) block index, so crops of any sizes share the launch without a padded grid.
//   units    a lane's unit of work is one ALIGNED DWORD of a destination row: output rows are 3 w bytes at any pitch and mostly not
//            dword-aligned, so a row at address a (mod 4) is cut into the bytes in front of the first aligned dword, whole dwords
//            (one 32-bit store each), and the bytes behind the last.  Consecutive lanes write consecutive dwords.
//   bytes    each output byte is crop_resize.h's crop_byte: four source bytes through the host-built tap tables, integers only.  The
//            source reads of neighbouring lanes fall into the same or neighbouring cache lines; the launch is bound by its latency
//            (a few MB move per call), not by HBM.
// Nothing outside a rectangle is read, nothing outside an output's pixel bytes is written.
#include "engine_internal.h"
#include "crop_resize.h"

namespace mi355 {
namespace {

__global__ __launch_bounds__(kCropThreads) void crop_kernel(const CropDesc* __restrict__ descs, const int* __restrict__ tabs, int n_crops) {
    const int blk = (int)blockIdx.x;
    int lo = 0, hi = n_crops - 1;                                      // the last crop with blk0 <= blk that owns blocks: blk0 is non-decreasing
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (descs[mid].blk0 <= blk) lo = mid; else hi = mid - 1;
    }
    const CropDesc d = descs[lo];                                      // crops without blocks share their successor's blk0: the search ends behind them
    const int items = d.out_h * d.units;
    const int row_bytes = 3 * d.out_w;
    int item = (blk - d.blk0) * (kCropThreads * kCropItemsPerThread) + (int)threadIdx.x;
#pragma unroll 1
    for (int it = 0; it < kCropItemsPerThread; ++it, item += kCropThreads) {
        if (item >= items) return;
        const int y = item / d.units, k = item - y * d.units;
        uint8_t* row = d.dst + (uint32_t)(y * d.dst_pitch);
        const int a = (int)((uintptr_t)row & 3u);
        const int j0 = 4 * k - a;                                      // the unit's first byte within the row; row + j0 is dword-aligned
        if (j0 >= row_bytes) continue;
        if (j0 >= 0 && j0 + 4 <= row_bytes) {
            const unsigned v = crop_byte(d, tabs, y, j0) | crop_byte(d, tabs, y, j0 + 1) << 8 | crop_byte(d, tabs, y, j0 + 2) << 16 |
                               crop_byte(d, tabs, y, j0 + 3) << 24;
            *reinterpret_cast<unsigned*>(row + j0) = v;
        } else {
            const int b0 = j0 < 0 ? 0 : j0, b1 = j0 + 4 < row_bytes ? j0 + 4 : row_bytes;
            for (int j = b0; j < b1; ++j) row[j] = (uint8_t)crop_byte(d, tabs, y, j);
        }
    }
}

constexpr size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

// no allocation, no synchronisation: safe inside a stream capture
const char* launch_crops(const CropDesc* descs_dev, const int* tabs_dev, int n_crops, unsigned blocks, hipStream_t st) {
    if (!blocks) return nullptr;
    hipLaunchKernelGGL(crop_kernel, dim3(blocks), dim3(kCropThreads), 0, st, descs_dev, tabs_dev, n_crops);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? hipGetErrorString(e) : nullptr;
}

// ---- the GPU half of one call: the work buffer's layout, staging of host rows, the launch, the copy back ---------------------------------
int crops_run_gpu(void* ctx_, int device, const mi355_render_frame* frames, int n, const mi355_render_out* outs, CropPlan& P, void* stream,
                  float* launch_ms) {
    CropCtx own;
    CropCtx& ctx = ctx_ ? *(CropCtx*)ctx_ : own;
    struct Free { CropCtx* c; ~Free() { if (c) crop_ctx_free(*c); } } guard{ctx_ ? nullptr : &own};
    hipStream_t st = (hipStream_t)stream;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return fail(MI355_EHIP, "no HIP device: the crop kernel needs an MI355X (device = -1 runs its host twin)"); }
    if (device >= ndev) return fail(MI355_EINVAL, "crops: device out of range");
    HIPCHK(hipSetDevice(device));
    const size_t M = P.desc.size();
    // the work buffer: [descriptors | tap tables || staged rows of host frames | outputs bound for the host, rows packed]
    const size_t desc_bytes = al256(M * sizeof(CropDesc)), img_bytes = al256(desc_bytes + P.tabs.size() * 4);
    size_t at = img_bytes;
    std::vector<size_t> src_off((size_t)n, 0), dst_off(M, 0);
    for (int i = 0; i < n; ++i) {
        if (frames[i].on_device || P.row1[i] <= P.row0[i]) continue;
        src_off[i] = at;
        at = al256(at + (size_t)(P.row1[i] - P.row0[i] - 1) * frames[i].row_stride + (size_t)frames[i].width * 3);
    }
    const size_t back_at = at;
    for (size_t k = 0; k < M; ++k) {
        if (outs[k].on_device || !P.desc[k].out_h || !P.desc[k].out_w) continue;
        dst_off[k] = at;
        at = al256(at + (size_t)P.desc[k].out_h * P.desc[k].out_w * 3);
    }
    const size_t back_bytes = at - back_at;
    if (buf_grow(ctx.d_work, at, at + at / 4) < 0 || buf_grow(ctx.h_img, img_bytes, img_bytes + img_bytes / 4) < 0 ||
        (back_bytes && buf_grow(ctx.h_out, back_bytes, back_bytes + back_bytes / 4) < 0))
        return fail(MI355_EHIP, "crops: out of device or pinned memory");
    uint8_t* base = ctx.d_work.p;
    for (int i = 0; i < n; ++i) {
        if (frames[i].on_device || P.row1[i] <= P.row0[i]) continue;
        const size_t bytes = (size_t)(P.row1[i] - P.row0[i] - 1) * frames[i].row_stride + (size_t)frames[i].width * 3;
        HIPCHK(hipMemcpyAsync(base + src_off[i], frames[i].data + (size_t)P.row0[i] * frames[i].row_stride, bytes, hipMemcpyHostToDevice, st));
    }
    std::vector<CropDesc> dev(P.desc);
    for (size_t k = 0; k < M; ++k) {
        CropDesc& d = dev[k];
        const int i = P.frame_of[k];
        if (!frames[i].on_device && d.cw) { d.src = base + src_off[i]; d.y1 -= P.row0[i]; }
        if (!outs[k].on_device && d.out_h && d.out_w) { d.dst = base + dst_off[k]; d.dst_pitch = 3 * d.out_w; }
    }
    std::memcpy(ctx.h_img.p, dev.data(), M * sizeof(CropDesc));
    if (!P.tabs.empty()) std::memcpy(ctx.h_img.p + desc_bytes, P.tabs.data(), P.tabs.size() * 4);
    HIPCHK(hipMemcpyAsync(base, ctx.h_img.p, img_bytes, hipMemcpyHostToDevice, st));
    if (launch_ms && !ctx.ev0) { HIPCHK(hipEventCreate(&ctx.ev0)); HIPCHK(hipEventCreate(&ctx.ev1)); }
    if (launch_ms) HIPCHK(hipEventRecord(ctx.ev0, st));
    KCHK(launch_crops((const CropDesc*)base, (const int*)(base + desc_bytes), (int)M, (unsigned)P.blocks, st));
    if (launch_ms) HIPCHK(hipEventRecord(ctx.ev1, st));
    if (back_bytes) HIPCHK(hipMemcpyAsync(ctx.h_out.p, base + back_at, back_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (size_t k = 0; k < M; ++k) {
        const CropDesc& d = P.desc[k];
        if (outs[k].on_device || !d.out_h || !d.out_w) continue;
        const size_t row = (size_t)d.out_w * 3;
        const uint8_t* from = ctx.h_out.p + (dst_off[k] - back_at);
        if ((size_t)d.dst_pitch == row) std::memcpy(d.dst, from, row * d.out_h);
        else for (int y = 0; y < d.out_h; ++y) std::memcpy(d.dst + (size_t)y * d.dst_pitch, from + (size_t)y * row, row);
    }
    if (launch_ms) HIPCHK(hipEventElapsedTime(launch_ms, ctx.ev0, ctx.ev1));
    return MI355_OK;
}

void crop_ctx_free(CropCtx& ctx) {
    buf_free(ctx.d_work); buf_free(ctx.h_img); buf_free(ctx.h_out);
    if (ctx.ev0) { (void)hipEventDestroy(ctx.ev0); (void)hipEventDestroy(ctx.ev1); ctx.ev0 = ctx.ev1 = nullptr; }
}

}  // namespace mi355

using namespace mi355;

extern "C" int mi355_yolo_crops(mi355_yolo* h, const mi355_render_frame* frames, int n, const int32_t* const* rects, const int* n_rects,
                                const mi355_crop_spec* spec, const mi355_render_out* outs, float* launch_ms) {
    if (!h) return fail(MI355_EINVAL, "crops: null handle");
    std::vector<mi355_render_frame> last;
    if (!frames) {                                             // the frames of the handle's last call, where that call left them on the device
        if (h->last_frames.empty()) return fail(MI355_EINVAL, "crops: the handle has no frames of a last blocking infer call");
        if (n != (int)h->last_frames.size())
            return fail(MI355_EINVAL, "crops: n = " + std::to_string(n) + ", but the last call had " + std::to_string(h->last_frames.size()) + " frames");
        last.resize((size_t)n);
        for (int i = 0; i < n; ++i) {
            const mi355_yolo::LastFrame& f = h->last_frames[i];
            if (!f.p) return fail(MI355_EINVAL, "crops: frame " + std::to_string(i) + " of the last call is no longer on the device (a host call of more than two "
                                                "chunks keeps its last two): pass the frames again");
            last[i] = mi355_render_frame{f.p, f.h, f.w, f.pitch, 1};
        }
        frames = last.data();
    }
    HIPCHK(hipSetDevice(h->device));
    if (h->async_pending) { HIPCHK(hipStreamSynchronize(h->stream)); h->async_pending = false; }
    return crops_call(&h->crops, h->device, frames, n, rects, n_rects, spec, outs, h->stream, launch_ms);
}
