// JPEG ingest: the C entries that need no handle, the checks every call makes before any work, and the host twin
// (device = -1).  No HIP in this file: with MI355_JPEG_DECODE_STANDALONE defined it builds, together with jpeg_decode.h and jpeg_sync.h
// alone, into a program that has no GPU half -- which is how tools/jpeg_decode_host_drive.cpp and tools/jpeg_sync_host_drive.cpp run
// mi355_jpeg_decode(-1, ...) and mi355_op_jpeg_sync(-1, ...) under sanitizers.
#include "jpeg_sync.h"

#include <cstdlib>

namespace mi355 {
#ifdef MI355_JPEG_DECODE_STANDALONE
thread_local std::string g_err;
int jpeg_dec_run_gpu(JpegDecCtx*, int, std::vector<JpegParsed>&, const mi355_jpeg_stream*, int, const int*, const mi355_render_out*, int16_t* const*,
                     int*, void*, float*, const JpegSyncOpts&) {
    g_err = "jpeg decode: built without the GPU half (device = -1 runs the host twin)";
    return MI355_EHIP;
}
#else
extern thread_local std::string g_err;          // engine_abi.hip
#endif
namespace {
int refuse(const std::string& msg) { g_err = msg; return MI355_EINVAL; }
// S of product calls: kJpegSyncSubBytes, or MI355_JPEG_SYNC_SUB_BYTES (a power of two, 8 .. 4096) -- a tuning knob, read at every
// call, with which tools/jpeg_decode_bench.py compares subsequence lengths in one run
int sync_sub_bytes() {
    const char* e = std::getenv("MI355_JPEG_SYNC_SUB_BYTES");
    const long v = e ? std::strtol(e, nullptr, 10) : 0;
    return v >= 8 && v <= 4096 && !(v & (v - 1)) ? (int)v : kJpegSyncSubBytes;
}
}  // namespace

int jpeg_dec_call(JpegDecCtx* ctx, int device, mi355_jpeg_stream* streams, int n, int entropy, const mi355_render_out* outs,
                  int16_t* const* coefs, int* status, void* stream, float* launch_ms, const JpegSyncOpts* sync) {
    JpegSyncOpts so = sync ? *sync : JpegSyncOpts{};
    if (!sync) so.S = sync_sub_bytes();
    if (!streams) return refuse("jpeg decode: null argument");
    if (!outs && !coefs) return refuse("jpeg decode: null output");
    if (n < 1 || n > MI355_RENDER_MAX_FRAMES) return refuse("jpeg decode: n must be in [1, " + std::to_string(MI355_RENDER_MAX_FRAMES) + "]");
    if (entropy < MI355_JPEG_ENTROPY_AUTO || entropy > MI355_JPEG_ENTROPY_SYNC)
        return refuse("jpeg decode: entropy must be MI355_JPEG_ENTROPY_AUTO (0), _GPU (1), _HOST (2) or _SYNC (3), got " + std::to_string(entropy));
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
        const int req = streams[i].entropy ? streams[i].entropy : entropy;      // the stream's own request goes first
        if (req < MI355_JPEG_ENTROPY_AUTO || req > MI355_JPEG_ENTROPY_SYNC) return refuse(at + "entropy must be 0 or an MI355_JPEG_ENTROPY_* value, got " + std::to_string(req));
        lanes[i] = req == MI355_JPEG_ENTROPY_SYNC ? 2 : device >= 0 && (req == MI355_JPEG_ENTROPY_GPU || (req == MI355_JPEG_ENTROPY_AUTO && f.ri > 0));
    }
    for (int i = 0; i < n; ++i) streams[i].entropy_used = lanes[i] == 2 ? MI355_JPEG_ENTROPY_SYNC : lanes[i] ? MI355_JPEG_ENTROPY_GPU : MI355_JPEG_ENTROPY_HOST;
    if (launch_ms) *launch_ms = 0.f;
    std::vector<int> st((size_t)n, 0);
    if (device < 0) {
        std::vector<int16_t> scratch;
        for (int i = 0; i < n; ++i) {
            int16_t* c = coefs ? coefs[i] : nullptr;
            if (!c) { scratch.resize((size_t)jpeg_dec_blocks(P[i].f) * 64); c = scratch.data(); }
            st[i] = lanes[i] == 2 ? jpeg_sync_coefficients_host(P[i], streams[i].data, so.S, so.Q, c, so.states, so.stats)
                                  : jpeg_dec_coefficients_host(P[i], streams[i].data, c);
            if (outs && !st[i]) jpeg_dec_pixels_host(P[i], c, outs[i].data, outs[i].row_stride);
        }
    } else {
        const int rc = jpeg_dec_run_gpu(ctx, device, P, streams, n, lanes.data(), outs, coefs, st.data(), stream, launch_ms, so);
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

int mi355_op_jpeg_sync(int device, mi355_jpeg_stream* stream, int sub_bytes, int seq_subs, int16_t* coef, int* status, mi355_jpeg_sync_state* states,
                       int max_states, mi355_jpeg_sync_stats* stats) {
    if (!stream || !stats) return refuse("jpeg sync: null argument");
    if (sub_bytes < 8 || sub_bytes > (1 << 20) || (sub_bytes & (sub_bytes - 1))) return refuse("jpeg sync: sub_bytes must be a power of two, at least 8");
    if (seq_subs < 2 || seq_subs > kJpegSyncSeqSubs) return refuse("jpeg sync: seq_subs must be in [2, " + std::to_string(kJpegSyncSeqSubs) + "]");
    if (!stream->data) return refuse("jpeg sync: the data pointer is null");
    JpegParsed P;
    std::string why;
    if (!jpeg_dec_parse(stream->data, stream->length, P, why)) return refuse("jpeg sync: " + why);
    JpegSyncTables T;
    jpeg_sync_tables(P, sub_bytes, seq_subs, T);
    *stats = mi355_jpeg_sync_stats{(int)T.nsub, (int)T.seqs.size(), 0, 0};
    if (!coef) return MI355_OK;
    if (states && (long long)max_states < (long long)T.nsub) return refuse("jpeg sync: states holds fewer than nsub entries");
    JpegSyncOpts so;
    so.S = sub_bytes; so.Q = seq_subs; so.states = states; so.stats = stats;
    mi355_jpeg_stream s = *stream;
    s.entropy = MI355_JPEG_ENTROPY_SYNC;
    int st = 0;
    int16_t* cp = coef;
    int rc = jpeg_dec_call(nullptr, device, &s, 1, MI355_JPEG_ENTROPY_SYNC, nullptr, &cp, &st, nullptr, nullptr, &so);
    stream->entropy_used = s.entropy_used;
    if (status) *status = st;
    if (rc == MI355_EINVAL && st) rc = MI355_OK;                          // corrupt entropy-coded data is this hook's result, not its failure
    return rc;
}

}  // extern "C"
