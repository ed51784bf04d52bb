// JPEG ingest: the C entries that need no handle, the checks every call makes before any work, and the host twin
// (device = -1).  No HIP in this file: with MI355_JPEG_DECODE_STANDALONE defined it builds, together with jpeg_decode.h alone, into a
// program that has no GPU half -- which is how tools/jpeg_decode_host_drive.cpp runs mi355_jpeg_decode(-1, ...) under sanitizers.
#include "jpeg_decode.h"

namespace mi355 {
#ifdef MI355_JPEG_DECODE_STANDALONE
thread_local std::string g_err;
int jpeg_dec_run_gpu(JpegDecCtx*, int, std::vector<JpegParsed>&, const mi355_jpeg_stream*, int, const int*, const mi355_render_out*, int16_t* const*,
                     int*, void*, float*) {
    g_err = "jpeg decode: built without the GPU half (device = -1 runs the host twin)";
    return MI355_EHIP;
}
#else
extern thread_local std::string g_err;          // engine_abi.hip
#endif
namespace {
int refuse(const std::string& msg) { g_err = msg; return MI355_EINVAL; }
}  // namespace

int jpeg_dec_call(JpegDecCtx* ctx, int device, mi355_jpeg_stream* streams, int n, int entropy, const mi355_render_out* outs,
                  int16_t* const* coefs, int* status, void* stream, float* launch_ms) {
    if (!streams) return refuse("jpeg decode: null argument");
    if (!outs && !coefs) return refuse("jpeg decode: null output");
    if (n < 1 || n > MI355_RENDER_MAX_FRAMES) return refuse("jpeg decode: n must be in [1, " + std::to_string(MI355_RENDER_MAX_FRAMES) + "]");
    if (entropy != MI355_JPEG_ENTROPY_AUTO && entropy != MI355_JPEG_ENTROPY_GPU && entropy != MI355_JPEG_ENTROPY_HOST)
        return refuse("jpeg decode: entropy must be MI355_JPEG_ENTROPY_AUTO (0), _GPU (1) or _HOST (2), got " + std::to_string(entropy));
    std::vector<JpegParsed> P((size_t)n);
    std::vector<int> lanes((size_t)n, 0);
    for (int i = 0; i < n; ++i) {
        const std::string at = "jpeg decode: streams[" + std::to_string(i) + "]: ";
        if (!streams[i].data) return refuse(at + "the data pointer is null");
        std::string why;
        if (!jpeg_dec_parse(streams[i].data, streams[i].length, P[i], why)) return refuse(at + why);
        const JpegDecFrame& f = P[i].f;
        if (outs) {
            if (!outs[i].data) return refuse("jpeg decode: outs[" + std::to_string(i) + "]: the data pointer is null");
            if ((long long)outs[i].row_stride < 3ll * f.W) return refuse("jpeg decode: outs[" + std::to_string(i) + "]: row_stride is smaller than a row of " + std::to_string(f.W) + " pixels");
            if ((long long)f.H * outs[i].row_stride >= (1ll << 31)) return refuse("jpeg decode: outs[" + std::to_string(i) + "]: a frame must be smaller than 2 GiB");
            if (device < 0 && outs[i].on_device) return refuse("jpeg decode: outs[" + std::to_string(i) + "]: the host twin (device -1) takes host memory");
        }
        if (coefs && !coefs[i]) return refuse("jpeg decode: coefs[" + std::to_string(i) + "]: the coefficient pointer is null");
        lanes[i] = device >= 0 && (entropy == MI355_JPEG_ENTROPY_GPU || (entropy == MI355_JPEG_ENTROPY_AUTO && f.ri > 0));
    }
    for (int i = 0; i < n; ++i) streams[i].entropy_used = lanes[i] ? MI355_JPEG_ENTROPY_GPU : MI355_JPEG_ENTROPY_HOST;
    if (launch_ms) *launch_ms = 0.f;
    std::vector<int> st((size_t)n, 0);
    if (device < 0) {
        std::vector<int16_t> scratch;
        for (int i = 0; i < n; ++i) {
            int16_t* c = coefs ? coefs[i] : nullptr;
            if (!c) { scratch.resize((size_t)jpeg_dec_blocks(P[i].f) * 64); c = scratch.data(); }
            st[i] = jpeg_dec_coefficients_host(P[i], streams[i].data, c);
            if (outs && !st[i]) jpeg_dec_pixels_host(P[i], c, outs[i].data, outs[i].row_stride);
        }
    } else {
        const int rc = jpeg_dec_run_gpu(ctx, device, P, streams, n, lanes.data(), outs, coefs, st.data(), stream, launch_ms);
        if (rc) return rc;
    }
    int bad = -1;
    for (int i = n - 1; i >= 0; --i) { if (status) status[i] = st[i]; if (st[i]) bad = i; }
    if (bad >= 0) return refuse("jpeg decode: streams[" + std::to_string(bad) + "]: corrupt entropy-coded data: " + jpeg_dec_status_name(st[bad]));
    return MI355_OK;
}
}  // namespace mi355

using namespace mi355;

extern "C" {

#ifdef MI355_JPEG_DECODE_STANDALONE
const char* mi355_last_error(void) { return g_err.c_str(); }
#endif

int mi355_jpeg_info(const uint8_t* data, int64_t length, mi355_jpeg_stream_info* info) {
    if (!data || !info) return refuse("jpeg info: null argument");
    JpegParsed P;
    std::string why;
    if (!jpeg_dec_parse(data, length, P, why)) return refuse("jpeg info: " + why);
    const JpegDecFrame& f = P.f;
    info->height = f.H; info->width = f.W; info->components = f.ncomp;
    info->subsampling = f.ncomp == 1 ? 400 : f.hs == 1 ? 444 : f.vs == 1 ? 422 : 420;
    info->restart_interval = f.ri; info->segments = f.nseg; info->blocks = jpeg_dec_blocks(f);
    return MI355_OK;
}

int mi355_jpeg_decode(int device, mi355_jpeg_stream* streams, int n, int entropy, const mi355_render_out* outs, int* status, void* stream,
                      float* launch_ms) {
    if (!outs) return refuse("jpeg decode: null output");
    return jpeg_dec_call(nullptr, device, streams, n, entropy, outs, nullptr, status, stream, launch_ms);
}

int mi355_op_jpeg_decode_coefficients(int device, mi355_jpeg_stream* streams, int n, int entropy, int16_t* const* coefs, int* status) {
    if (!coefs) return refuse("jpeg decode: null output");
    return jpeg_dec_call(nullptr, device, streams, n, entropy, nullptr, coefs, status, nullptr, nullptr);
}

}  // extern "C"
