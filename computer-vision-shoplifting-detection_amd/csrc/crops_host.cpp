// Person crops: the C entry that needs no handle, the checks every call makes before any work, the descriptors and tap
// tables, and the host twin (device = -1).  No HIP in this file: with MI355_CROPS_STANDALONE defined it builds, together with
// crop_resize.h alone, into a program that has no GPU half -- which is how tools/crop_host_drive.cpp runs mi355_crops(-1, ...) under
// sanitizers.
#include "crop_resize.h"

#include <algorithm>
#include <map>
#include <utility>

namespace mi355 {
#ifdef MI355_CROPS_STANDALONE
thread_local std::string g_err;
int crops_run_gpu(void*, int, const mi355_render_frame*, int, const mi355_render_out*, CropPlan&, void*, float*) {
    g_err = "crops: built without the GPU half (device = -1 runs the host twin)";
    return MI355_EHIP;
}
#else
extern thread_local std::string g_err;          // engine_abi.hip
#endif
namespace {
int refuse(const std::string& msg) { g_err = msg; return MI355_EINVAL; }

// Python's round(): half to even.  x >= 0 and far below 2^52
int round_half_even(double x) {
    const double f = std::floor(x), r = x - f;
    const long long i = (long long)f;
    return (int)(r > 0.5 || (r == 0.5 && (i & 1)) ? i + 1 : i);
}
}  // namespace

int crops_call(void* ctx, int device, const mi355_render_frame* frames, int n, const int32_t* const* rects, const int* n_rects,
               const mi355_crop_spec* spec, const mi355_render_out* outs, void* stream, float* launch_ms) {
    if (!frames) return refuse("crops: frames is null");
    if (!rects) return refuse("crops: rects is null");
    if (!n_rects) return refuse("crops: n_rects is null");
    if (!spec) return refuse("crops: spec is null");
    if (n < 1 || n > MI355_RENDER_MAX_FRAMES) return refuse("crops: n must be in [1, " + std::to_string(MI355_RENDER_MAX_FRAMES) + "]");
    if (spec->struct_size != (int)sizeof(mi355_crop_spec)) return refuse("crops: spec.struct_size is not sizeof(mi355_crop_spec)");
    const bool native = spec->height == 0 && spec->width == 0;
    if (!native && (spec->height < 1 || spec->width < 1 || spec->height > kCropMaxSide || spec->width > kCropMaxSide))
        return refuse("crops: spec.height and spec.width must both be 0 (native) or in [1, " + std::to_string(kCropMaxSide) + "], got " +
                      std::to_string(spec->height) + " x " + std::to_string(spec->width));
    if (spec->fit != MI355_CROP_STRETCH && spec->fit != MI355_CROP_PAD)
        return refuse("crops: spec.fit must be MI355_CROP_STRETCH (0) or MI355_CROP_PAD (1), got " + std::to_string(spec->fit));
    if (spec->fill < 0 || spec->fill > 255) return refuse("crops: spec.fill must be in [0, 255], got " + std::to_string(spec->fill));
    long long total = 0;
    for (int i = 0; i < n; ++i) {
        const mi355_render_frame& f = frames[i];
        const std::string at = "crops: frames[" + std::to_string(i) + "]: ";
        if (!f.data) return refuse(at + "the data pointer is null");
        if (f.height < 1 || f.width < 1 || f.height > kCropMaxSide || f.width > kCropMaxSide)
            return refuse(at + "height and width must be in [1, " + std::to_string(kCropMaxSide) + "]");
        if ((long long)f.row_stride < 3ll * f.width) return refuse(at + "row_stride is smaller than a row");
        if ((long long)f.height * f.row_stride >= (1ll << 31)) return refuse(at + "a frame must be smaller than 2 GiB");
        if (device < 0 && f.on_device) return refuse(at + "the host twin (device -1) takes host memory");
        if (n_rects[i] < 0) return refuse("crops: n_rects[" + std::to_string(i) + "] is negative");
        if (n_rects[i] && !rects[i]) return refuse("crops: rects[" + std::to_string(i) + "] is null");
        total += n_rects[i];
        for (int k = 0; k < n_rects[i]; ++k) {
            const int32_t* r = rects[i] + (size_t)k * 4;
            if (r[0] < 0 || r[1] < 0 || r[2] < 0 || r[3] < 0 || r[0] > f.width || r[2] > f.width || r[1] > f.height || r[3] > f.height)
                return refuse("crops: rects[" + std::to_string(i) + "][" + std::to_string(k) + "] = (" + std::to_string(r[0]) + ", " + std::to_string(r[1]) + ", " +
                              std::to_string(r[2]) + ", " + std::to_string(r[3]) + ") lies outside its frame of " + std::to_string(f.height) + " x " + std::to_string(f.width));
        }
    }
    if (total > MI355_CROP_MAX_RECTS) return refuse("crops: " + std::to_string(total) + " rectangles: at most MI355_CROP_MAX_RECTS = " + std::to_string(MI355_CROP_MAX_RECTS) + " per call");
    if (total && !outs) return refuse("crops: outs is null");

    CropPlan P;
    P.desc.reserve((size_t)total); P.frame_of.reserve((size_t)total);
    P.row0.assign((size_t)n, 1 << 30); P.row1.assign((size_t)n, 0);
    std::map<std::pair<int, int>, int> tab_at;      // (destination, source) side -> first int32 of its table
    auto table = [&](int dn, int sn) {
        auto it = tab_at.find({dn, sn});
        if (it != tab_at.end()) return it->second;
        const int at = (int)P.tabs.size();
        P.tabs.resize((size_t)at + (size_t)dn * 3);
        crop_tap_table(dn, sn, P.tabs.data() + at);
        tab_at[{dn, sn}] = at;
        return at;
    };
    size_t o = 0;
    for (int i = 0; i < n; ++i) {
        for (int k = 0; k < n_rects[i]; ++k, ++o) {
            const int32_t* r = rects[i] + (size_t)k * 4;
            const bool empty = r[2] <= r[0] || r[3] <= r[1];
            CropDesc d{};
            d.src = frames[i].data; d.src_pitch = frames[i].row_stride;
            d.dst = outs[o].data; d.dst_pitch = outs[o].row_stride;
            d.x1 = r[0]; d.y1 = r[1]; d.cw = empty ? 0 : r[2] - r[0]; d.ch = empty ? 0 : r[3] - r[1];
            d.fill = spec->fill; d.xtab = d.ytab = -1;
            if (native) { d.out_w = d.in_w = d.cw; d.out_h = d.in_h = d.ch; }
            else {
                d.out_w = spec->width; d.out_h = spec->height;
                if (empty) d.in_w = d.in_h = 0;
                else if (spec->fit == MI355_CROP_STRETCH) { d.in_w = d.out_w; d.in_h = d.out_h; }
                else {      // LetterBox(auto=False): the scale, the rounded inner size (at least 1), the pad split
                    const double rr = std::min((double)d.out_h / d.ch, (double)d.out_w / d.cw);
                    d.in_w = std::min(std::max(round_half_even(d.cw * rr), 1), d.out_w);
                    d.in_h = std::min(std::max(round_half_even(d.ch * rr), 1), d.out_h);
                    d.off_x = round_half_even((d.out_w - d.in_w) / 2.0 - 0.1 + 1.0) - 1;     // round(dw / 2 - 0.1), dw / 2 - 0.1 >= -0.1
                    d.off_y = round_half_even((d.out_h - d.in_h) / 2.0 - 0.1 + 1.0) - 1;
                }
                if (!empty && (d.in_w != d.cw || d.in_h != d.ch)) { d.xtab = table(d.in_w, d.cw); d.ytab = table(d.in_h, d.ch); }
            }
            const std::string at = "crops: outs[" + std::to_string(o) + "]: ";
            if (d.out_w > 0 && d.out_h > 0) {
                if (!d.dst) return refuse(at + "the data pointer is null");
                if ((long long)d.dst_pitch < 3ll * d.out_w) return refuse(at + "row_stride is smaller than a row of " + std::to_string(d.out_w) + " pixels");
                if ((long long)d.out_h * d.dst_pitch >= (1ll << 31)) return refuse(at + "an output must be smaller than 2 GiB");
                if (device < 0 && outs[o].on_device) return refuse(at + "the host twin (device -1) takes host memory");
            }
            d.units = crop_row_units(d.out_w);
            d.blk0 = (int)P.blocks;
            const long long items = (long long)d.out_h * d.units, per = (long long)kCropThreads * kCropItemsPerThread;
            P.blocks += (items + per - 1) / per;
            if (!empty) { P.row0[i] = std::min(P.row0[i], d.y1); P.row1[i] = std::max(P.row1[i], d.y1 + d.ch); }
            P.desc.push_back(d); P.frame_of.push_back(i);
        }
    }
    if (P.blocks >= (1ll << 31)) return refuse("crops: the call's outputs are too large for one launch");
    if (launch_ms) *launch_ms = 0.f;
    if (device < 0) {
        for (const CropDesc& d : P.desc) crop_host(d, P.tabs.data());
        return MI355_OK;
    }
    if (!total) return MI355_OK;
    return crops_run_gpu(ctx, device, frames, n, outs, P, stream, launch_ms);
}

}  // namespace mi355

extern "C" int mi355_crops(int device, const mi355_render_frame* frames, int n, const int32_t* const* rects, const int* n_rects,
                           const mi355_crop_spec* spec, const mi355_render_out* outs, void* stream, float* launch_ms) {
    return mi355::crops_call(nullptr, device, frames, n, rects, n_rects, spec, outs, stream, launch_ms);
}
