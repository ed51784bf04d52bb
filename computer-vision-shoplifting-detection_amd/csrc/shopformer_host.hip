// Shopformer score path, host side: parse the weight image (cvsd_amd/shopformer.py:build_image), upload it, plan LDS, and the C ABI
// mi355_shopformer_* of include/mi355_yolo.h.  One kernel launch per call whatever the number of windows for variant 1, two for variant 2
// (version-2 images): tokenizer, then the transformer over row groups of up to 16 windows (shopformer_kernels.hip).
// Version-3 images hold either variant plus the GCAE decoder: one more launch (shopformer_decoder.hip), only when asked.
// mi355_shopformer_score_poses takes poses and window starts instead of windows: one launch more, pose_windows.hip.
//
// Every step is stated once.  Loading is a chain of named steps (parse_image, check_envelope, the three LDS plans, check_adjacency,
// bind_tensors on the host copy and again on the uploaded one, upload, count_macs); every refusal of an image fires before the first HIP
// call.  Every score entry point is its argument checks (check_outputs) plus ONE shared launch sequence (enqueue); the blocking ones
// stage through run_blocking; the 6- and 7-argument forms are wrappers that build the outputs struct.  Device memory is the grow-only
// Buf of dev_buf.h: a call grows the buffers it uses, to what it needs.
#include "engine_internal.h"
#include "shopformer.h"
#include "pose_windows.h"
#include "dev_buf.h"

#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <map>

using namespace mi355;

struct mi355_shopformer {
    int device = 0;
    SfParams p{};
    SfParams* d_params = nullptr;       // the kernel reads its parameters from device memory
    float* d_weights = nullptr;
    long long launches = 0;             // kernel launches enqueued through this handle
    // staging of the blocking calls, used on `stream` only: the windows, one buffer per output, the poses and starts of score_poses
    Buf win, score, tsc, tok, rec, pose, perr, pose_in, starts;
    // Two token buffers, on purpose.  `tok` above belongs to the blocking calls and is used on `stream`; `tok_scratch` is where a
    // device / async call without a tokens output leaves its tokens, on the CALLER's stream.  Such a call may still be running when a
    // blocking call starts on the same handle, so one buffer for both would be a race.
    Buf tok_scratch;
    int lds_tf = 0;                     // variant 2: LDS of the transformer launch
    hipStream_t stream = nullptr;
    long long n_params = 0, macs = 0;
    int lds_bytes = 0;
    // the GCAE decoder (version-3 images)
    bool has_dec = false;
    SfDecParams dp{};
    SfDecParams* d_dec = nullptr;
    int lds_dec = 0;
    long long macs_dec = 0;
    ~mi355_shopformer() {
        if (d_weights) (void)hipFree(d_weights);
        if (d_params) (void)hipFree(d_params);
        if (d_dec) (void)hipFree(d_dec);
        for (Buf* b : {&win, &score, &tsc, &tok, &rec, &pose, &perr, &pose_in, &starts, &tok_scratch}) buf_free(*b);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace {

struct Entry { uint32_t kind, d[3]; uint64_t off, count; };
constexpr int kNCfg = 18;              // V, T, H, L, heads, layers, ff, D, ntok, nnz, s0..s3, T1..T4
constexpr int kNCfg2 = 24;             // version 2: + variant, Din, in_proj, out_proj, norm_kind, act_kind
constexpr int kNCfg3 = 30;             // version 3: + the decoder's four factors, the frames its layers emit, the interpolation flag
const char* kNoDecoder = "this Shopformer weight image was built without the decoder (build it with decoder=True)";

int pad_stride(int k) { int c = (k + 3) / 4 * 4; if (((c / 4) & 1) == 0) c += 4; return c; }   // 4 * odd

// ---- loading: each step of mi355_shopformer_create once, in the order its refusals fire -----------------------------------------------
// the header and the tensor table of a weight image; `data` points into the caller's bytes
struct Image {
    uint32_t ver = 0, ncfg = 0;
    int cfg[kNCfg3] = {0};
    bool v2 = false, dec = false;      // the shopformer_2 variant; the GCAE decoder's fields and tensors are there
    std::map<std::string, Entry> tab;
    const float* data = nullptr; size_t nfloats = 0;
};

int parse_image(const uint8_t* blob, size_t nbytes, Image& im) {
    if (nbytes < 24 || std::memcmp(blob, "MI355SF1", 8) != 0) return fail(MI355_EFORMAT, "not a Shopformer weight image (bad magic)");
    std::memcpy(&im.ver, blob + 8, 4); std::memcpy(&im.ncfg, blob + 12, 4);
    if (!((im.ver == 1 && im.ncfg == kNCfg) || (im.ver == 2 && im.ncfg == kNCfg2) || (im.ver == 3 && im.ncfg == kNCfg3)))
        return fail(MI355_EFORMAT, "unsupported Shopformer weight image version");
    size_t pos = 16;
    if (nbytes < pos + 4 * im.ncfg + 4) return fail(MI355_EFORMAT, "truncated Shopformer weight image");
    std::memcpy(im.cfg, blob + pos, 4 * im.ncfg); pos += 4 * im.ncfg;
    im.v2 = im.ver == 2 || (im.ver == 3 && im.cfg[18] == 2);
    im.dec = im.ver == 3;
    uint32_t nent; std::memcpy(&nent, blob + pos, 4); pos += 4;
    const size_t rec = 32 + 4 + 12 + 16;
    if (nent > 4096 || nbytes < pos + nent * rec) return fail(MI355_EFORMAT, "truncated Shopformer weight image");
    for (uint32_t i = 0; i < nent; ++i) {
        const uint8_t* r = blob + pos + i * rec;
        char name[33] = {0}; std::memcpy(name, r, 32);
        Entry e; std::memcpy(&e.kind, r + 32, 4); std::memcpy(e.d, r + 36, 12); std::memcpy(&e.off, r + 48, 8); std::memcpy(&e.count, r + 56, 8);
        im.tab[name] = e;
    }
    pos += nent * rec; pos += (16 - pos % 16) % 16;
    if (nbytes < pos) return fail(MI355_EFORMAT, "truncated Shopformer weight image");      // cut inside the padding: no wrapped float count
    im.data = (const float*)(blob + pos); im.nfloats = (nbytes - pos) / 4;
    for (auto& kv : im.tab)
        if (kv.second.off > im.nfloats || kv.second.count > im.nfloats - kv.second.off || kv.second.off % 4)       // no wrap; float4 reads
            return fail(MI355_EFORMAT, "Shopformer weight image: tensor '" + kv.first + "' lies outside the file");
    return MI355_OK;
}

int in_set(int v, std::initializer_list<int> s) { for (int x : s) if (x == v) return 1; return 0; }
int bad(const char* f, int v) { return fail(MI355_EFORMAT, std::string("Shopformer weight image: unsupported ") + f + " = " + std::to_string(v)); }

// the score kernels' envelope (the Python loader refuses the same fields by name before an image is ever built) -> p's geometry
int check_envelope(const Image& im, SfParams& p) {
    const int* cfg = im.cfg;
    const bool v2 = im.v2;
    p.V = cfg[0]; p.T = cfg[1]; p.H = cfg[2]; p.L = cfg[3]; p.heads = cfg[4]; p.layers = cfg[5]; p.ff = cfg[6]; p.D = cfg[7]; p.ntok = cfg[8]; p.nnz = cfg[9];
    for (int i = 0; i < 4; ++i) { p.s[i] = cfg[10 + i]; p.Tn[i + 1] = cfg[14 + i]; }
    p.Tn[0] = p.T;
    if (!in_set(p.V, {17, 18})) return bad("num_keypoints", p.V);
    if (!in_set(p.T, {12, 24})) return bad("seq_len", p.T);
    if (!in_set(p.H, {32, 64})) return bad("hidden_channels", p.H);
    if (!in_set(p.L, {4, 8})) return bad("latent_channels", p.L);
    if (im.dec && cfg[18] != 1 && cfg[18] != 2) return bad("variant", cfg[18]);
    if (im.dec && !v2 && (cfg[19] != p.D || cfg[20] || cfg[21] || cfg[22] != 0 || cfg[23] != 0)) return bad("variant-1 field in a version-3 image", cfg[19]);
    p.variant = v2 ? cfg[18] : 1; p.Din = v2 ? cfg[19] : p.D; p.in_proj = v2 ? cfg[20] : 0; p.out_proj = v2 ? cfg[21] : 0;
    if (v2) {
        if (p.variant != 2) return bad("variant", p.variant);
        if (p.Din != p.L * p.V) return bad("transformer.input_dim", p.Din);
        if (p.D < 4 || p.D % 4 || p.D > 144) return bad("transformer.d_model", p.D);
        if (p.heads < 1 || p.D % p.heads) return bad("transformer.num_heads", p.heads);
        if (p.ff <= 0 || p.ff % 4 || p.ff > 512) return bad("transformer.dim_feedforward", p.ff);
        if ((p.in_proj != 0 && p.in_proj != 1) || p.in_proj != (p.Din != p.D)) return bad("input projection flag", p.in_proj);
        if (p.out_proj != p.in_proj) return bad("output projection flag", p.out_proj);
        if (cfg[22] != 1) return bad("norm kind", cfg[22]);
        if (cfg[23] != 1) return bad("activation kind", cfg[23]);
    } else {
        if (!in_set(p.heads, {1, 2, 4}) || p.D != p.L * p.V || p.D % p.heads) return bad("transformer_heads", p.heads);
        if (p.ff <= 0 || p.ff % 4 || p.ff > 64) return bad("transformer_ff_dim", p.ff);
    }
    if (p.layers < 1 || p.layers > SF_MAX_LAYERS) return bad(v2 ? "transformer.num_layers" : "transformer_layers", p.layers);
    if (p.nnz < 1 || p.nnz > p.V) return bad("adjacency row length", p.nnz);
    for (int i = 0; i < 4; ++i) {
        const bool ok = v2 ? in_set(p.s[i], {1, 2, 3}) : in_set(p.s[i], {1, 2});
        if (!ok || p.Tn[i + 1] != (p.Tn[i] - 1) / p.s[i] + 1) return bad("block stride", p.s[i]);
    }
    if (p.ntok != p.Tn[4] || p.ntok < 1 || p.ntok > 8 || (v2 && p.ntok != 2)) return bad("token count", p.ntok);
    p.att_scale = 1.0f / std::sqrt((float)(p.D / p.heads));
    p.csH = pad_stride(p.H); p.csD = pad_stride(std::max(p.D, p.Din)); p.csQ = pad_stride(3 * p.D); p.csF = pad_stride(p.ff);
    return MI355_OK;
}

// LDS of the first launch for G windows per workgroup (floats; every region a multiple of 4); variant 2's transformer is its own launch
int lds_tokenizer(const SfParams& p, int G, int* offs) {
    const int in = (G * p.T * p.V * 2 + 3) / 4 * 4;
    const int rows = G * p.ntok;
    const int tf = p.variant == 2 ? 0 : rows * (5 * p.csD + p.csQ + p.csF) + (G * p.heads * p.ntok * p.ntok + 3) / 4 * 4;
    const int P = std::max(G * p.Tn[1] * p.V * p.csH, tf);
    const int Q = G * std::max(p.Tn[2], p.Tn[4]) * p.V * p.csH;
    offs[0] = 0; offs[1] = in; offs[2] = 2 * in; offs[3] = 2 * in + P;
    return (2 * in + P + Q) * 4;
}
// the largest group of windows that fits
int plan_tokenizer(SfParams& p, int* lds_bytes) {
    int offs[4], G = 0;
    for (int g = 8; g >= 1; --g) if (lds_tokenizer(p, g, offs) <= SF_LDS_BYTES) { G = g; break; }
    if (!G) return fail(MI355_EFORMAT, "Shopformer weight image: one window does not fit the 160 KiB of LDS");
    *lds_bytes = lds_tokenizer(p, G, offs);
    p.G = G; p.offXin = offs[0]; p.offAx = offs[1]; p.offP = offs[2]; p.offQ = offs[3];
    return MI355_OK;
}

// variant 2's transformer launch: state of the decoder, state of the encoder / memory, the normed copy, and one region that is
// q|k|v + attention output during attention and the feed-forward hidden layer after it; up to 16 windows = 32 rows
int lds_transformer(const SfParams& p, int GT, int* o) {
    const int rows = GT * p.ntok, u = std::max(p.csQ + p.csD, p.csF);
    o[0] = 0; o[1] = rows * p.csD; o[2] = 2 * rows * p.csD; o[3] = 3 * rows * p.csD; o[4] = o[3] + rows * u;
    return (o[4] + (GT * p.heads * p.ntok * p.ntok + 3) / 4 * 4) * 4;
}
int plan_transformer(SfParams& p, int* lds_bytes) {
    int o[5], GT = 0;
    for (int g : {16, 8, 4, 2, 1}) if (lds_transformer(p, g, o) <= SF_LDS_BYTES) { GT = g; break; }
    if (!GT) return fail(MI355_EFORMAT, "Shopformer weight image: one window's tokens do not fit the 160 KiB of LDS");
    if (const char* e = std::getenv("MI355_SF2_ROW_GROUP")) {      // kernel experiments (row-group A/B of DESIGN.md 3.9); the product never sets it
        const int g = std::atoi(e);
        if (g >= 1 && g <= GT) GT = g;
    }
    *lds_bytes = lds_transformer(p, GT, o);
    p.GT = GT; p.offTgt = o[0]; p.offX = o[1]; p.offNb = o[2]; p.offU = o[3]; p.offSc = o[4];
    return MI355_OK;
}

// the decoder's envelope: factors 1 or 2, a 1x1 last layer, the frame count they imply, at most the window's length
int check_decoder_envelope(const Image& im, const SfParams& p, SfDecParams& d) {
    d.V = p.V; d.T = p.T; d.H = p.H; d.L = p.L; d.ntok = p.ntok; d.Din = p.L * p.V;
    int frames = p.ntok;
    for (int i = 0; i < 4; ++i) {
        d.f[i] = im.cfg[24 + i];
        if (!in_set(d.f[i], {1, 2}) || (i == 3 && d.f[i] != 1)) return bad("decoder upsample factor", d.f[i]);
        frames *= d.f[i];
    }
    d.Td = im.cfg[28]; d.interp = im.cfg[29];
    if (d.Td != frames || d.Td > p.T) return bad("decoder frame count", d.Td);
    if (d.interp != (d.Td != p.T ? 1 : 0)) return bad("decoder interpolation flag", d.interp);
    if ((p.V * p.H) % 32) return bad("decoder initial_proj width", p.V * p.H);
    d.scale = (float)d.Td / (float)p.T;
    d.csT = pad_stride(d.Din); d.csH = pad_stride(p.H);
    return MI355_OK;
}

// row group: G windows = G * ntok rows of initial_proj.  4 windows (8 or 12 rows of the 16-row tile) measured fastest: two
// workgroups fit a CU's LDS, which gains more than the full tile of 5 or 8 windows
int lds_decoder(const SfParams& p, SfDecParams& d, int G) {
    d.offTok = 0; d.offX = G * p.ntok * d.csT; d.offOut = d.offX + G * p.ntok * p.V * d.csH;
    return (d.offOut + (G * 2 * d.Td * p.V + 3) / 4 * 4) * 4;
}
int plan_decoder(const SfParams& p, SfDecParams& d, int* lds_bytes) {
    int G = 4;
    if (const char* e = std::getenv("MI355_SFD_ROW_GROUP")) {      // kernel experiments (row-group A/B of DESIGN.md 3.11); the product never sets it
        const int g = std::atoi(e);
        if (g >= 1 && g <= 32) G = g;
    }
    while (G > 1 && lds_decoder(p, d, G) > SF_LDS_BYTES) --G;
    if (lds_decoder(p, d, G) > SF_LDS_BYTES) return fail(MI355_EFORMAT, "Shopformer weight image: one window's decoder rows do not fit the 160 KiB of LDS");
    d.G = G; *lds_bytes = lds_decoder(p, d, G);
    return MI355_OK;
}

// adjacency columns must stay inside a pose (they index LDS rows); a table that is absent is bind_tensors' refusal
int check_adjacency(const Image& im, const SfParams& p) {
    const auto it = im.tab.find("adj_col");
    if (it == im.tab.end()) return MI355_OK;
    const Entry& e = it->second;
    if (e.count < (uint64_t)p.V * p.nnz) return fail(MI355_EFORMAT, "Shopformer weight image: adjacency table too short");
    for (int i = 0; i < p.V * p.nnz; ++i) {
        const float c = im.data[e.off + i];
        if (!(c >= 0.f && c <= (float)(p.V - 1)) || c != std::floor(c)) return fail(MI355_EFORMAT, "Shopformer weight image: adjacency column outside the pose");
    }
    return MI355_OK;
}

// one pass over the tensor table against `base` (the image's floats on the host, then their uploaded copy): names and shapes are
// checked, pointers handed out, logical parameters counted; `miss` keeps the last tensor that was missing or misshapen
struct Binder {
    const Image& im; const float* base; const SfParams& p;
    long long n_params = 0; std::string miss;
    const Entry* find(const std::string& n) { auto it = im.tab.find(n); if (it == im.tab.end()) { miss = n; return nullptr; } return &it->second; }
    // packed: [tiles of 16 out][taps][blocks of 16 in][256]; plain: at least `need` floats
    const float* packed(const std::string& n, int co, int taps, int ci) {
        const Entry* e = find(n); if (!e) return nullptr;
        const uint64_t want = (uint64_t)((co + 15) / 16) * taps * ((ci + 15) / 16) * 256;
        if (e->kind != 1 || (int)e->d[0] != co || (int)e->d[1] != taps || (int)e->d[2] != ci || e->count != want) { miss = n + " (shape)"; return nullptr; }
        n_params += (long long)co * taps * ci;
        return base + e->off;
    }
    const float* plain(const std::string& n, int need) {
        const Entry* e = find(n); if (!e) return nullptr;
        if (e->kind != 0 || e->count < (uint64_t)((need + 15) / 16 * 16)) { miss = n + " (shape)"; return nullptr; }
        n_params += need;
        return base + e->off;
    }
    SfLin lin(const std::string& n, int o, int i) { SfLin l; l.w = packed(n + ".w", o, 1, i); l.b = plain(n + ".b", o); return l; }
    SfNorm norm(const std::string& n) { SfNorm l; l.g = plain(n + ".g", p.D); l.b = plain(n + ".b", p.D); return l; }
    SfAttn attn(const std::string& n) { SfAttn a; a.q = lin(n + ".q", p.D, p.D); a.kv = lin(n + ".kv", 2 * p.D, p.D); a.out = lin(n + ".out", p.D, p.D); return a; }
};

int bind_tensors(const Image& im, const float* base, mi355_shopformer* h) {
    SfParams& p = h->p;
    Binder b{im, base, p};
    const int ch[5] = {2, p.H, p.H, p.H, p.L};
    p.in_scale = b.plain("in_scale", 2 * p.V); p.in_shift = b.plain("in_shift", 2 * p.V);
    p.adj_col = b.plain("adj_col", p.V * p.nnz); p.adj_val = b.plain("adj_val", p.V * p.nnz);
    p.pe_in = b.plain("pe_in", p.ntok * p.D); p.pe_score = im.v2 ? nullptr : b.plain("pe_score", p.ntok * p.D);
    for (int i = 0; i < 4; ++i) {
        const std::string n = "b" + std::to_string(i);
        const bool conv_res = ch[i] != ch[i + 1] || p.s[i] != 1;
        SfBlock& k = p.blk[i];
        k.gw = i == 0 ? b.plain(n + ".gw", 2 * p.H) : b.packed(n + ".gw", ch[i + 1], 1, ch[i]);
        k.gb = b.plain(n + ".gb", ch[i + 1]);
        k.tw = b.packed(n + ".tw", ch[i + 1], 9, ch[i + 1]); k.tb = b.plain(n + ".tb", ch[i + 1]);
        k.rw = !conv_res ? nullptr : i == 0 ? b.plain(n + ".rw", 2 * p.H) : b.packed(n + ".rw", ch[i + 1], 1, ch[i]);
        k.rb = conv_res ? b.plain(n + ".rb", ch[i + 1]) : nullptr;
    }
    for (int e = 0; e < p.layers; ++e) {
        const std::string a = "e" + std::to_string(e), d = "d" + std::to_string(e);
        p.enc[e] = SfEnc{b.attn(a + ".sa"), b.norm(a + ".n1"), b.lin(a + ".f1", p.ff, p.D), b.lin(a + ".f2", p.D, p.ff), b.norm(a + ".n2")};
        p.dec[e] = SfDec{b.attn(d + ".sa"), b.norm(d + ".n1"), b.attn(d + ".ca"), b.norm(d + ".n2"), b.lin(d + ".f1", p.ff, p.D), b.lin(d + ".f2", p.D, p.ff), b.norm(d + ".n3")};
    }
    if (im.v2) {
        p.en = b.norm("en"); p.dn = b.norm("dn");
        if (p.in_proj) p.inp = b.lin("inp", p.D, p.Din);
        if (p.out_proj) p.outp = b.lin("outp", p.Din, p.D);
    } else {
        p.proj = b.lin("proj", p.D, p.D);
    }
    if (im.dec) {
        SfDecParams& d = h->dp;
        d.ipw = b.packed("dec.ip.w", p.V * p.H, 1, d.Din); d.ipb = b.plain("dec.ip.b", p.V * p.H);
        for (int i = 0; i < 4; ++i) {
            const std::string n = "dec.l" + std::to_string(i);
            d.w[i] = b.packed(n + ".w", i == 3 ? 2 : p.H, d.f[i], p.H); d.b[i] = b.plain(n + ".b", i == 3 ? 2 : p.H);
        }
    }
    h->n_params = b.n_params;
    if (!b.miss.empty()) return fail(MI355_EFORMAT, "Shopformer weight image: tensor '" + b.miss + "' is missing or has the wrong shape");
    return MI355_OK;
}

// the first HIP calls of a create: the device, the kernels' LDS attribute, the image's floats, the handle's stream
int upload(const Image& im, int device, mi355_shopformer* h) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(MI355_EHIP, "no HIP device: the Shopformer kernel needs an MI355X (there is no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(MI355_EINVAL, "device index out of range");
    h->device = device;
    HIPCHK(hipSetDevice(device));
    KCHK(prepare_shopformer_device());
    if (im.dec) KCHK(prepare_shopformer_decoder_device());
    HIPCHK(hipMalloc(&h->d_weights, std::max<size_t>(im.nfloats, 4) * 4));
    HIPCHK(hipMemcpy(h->d_weights, im.data, im.nfloats * 4, hipMemcpyHostToDevice));
    HIPCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    return MI355_OK;
}
// ... and the last: the parameter blocks, their pointers bound to the uploaded copy
int upload_params(mi355_shopformer* h) {
    HIPCHK(hipMalloc(&h->d_params, sizeof(SfParams)));
    HIPCHK(hipMemcpy(h->d_params, &h->p, sizeof(SfParams), hipMemcpyHostToDevice));
    if (h->has_dec) {
        HIPCHK(hipMalloc(&h->d_dec, sizeof(SfDecParams)));
        HIPCHK(hipMemcpy(h->d_dec, &h->dp, sizeof(SfDecParams), hipMemcpyHostToDevice));
    }
    return MI355_OK;
}

// multiply-accumulates per window, zero-padding taps not counted
long long count_macs(const SfParams& p) {
    const int ch[5] = {2, p.H, p.H, p.H, p.L};
    long long macs = 0;
    for (int b = 0; b < 4; ++b) {
        long long taps = 0;
        for (int to = 0; to < p.Tn[b + 1]; ++to) for (int k = 0; k < 9; ++k) { const int ti = to * p.s[b] + k - 4; taps += ti >= 0 && ti < p.Tn[b]; }
        macs += (long long)p.V * (taps * ch[b + 1] * ch[b + 1] + (long long)p.Tn[b] * ch[b] * ch[b + 1] + (p.blk[b].rw ? (long long)p.Tn[b + 1] * ch[b] * ch[b + 1] : 0));
    }
    const long long at = 4LL * p.D * p.D, ffm = 2LL * p.D * p.ff;
    return macs + (long long)p.ntok * (p.layers * (at + ffm) + p.layers * (2 * at + ffm) +
                                       (p.variant == 2 ? (long long)(p.in_proj + p.out_proj) * p.D * p.Din : (long long)p.D * p.D));
}
long long count_macs_decoder(const SfParams& p, const SfDecParams& d) {
    long long rows = p.ntok, m = (long long)p.ntok * d.Din * p.H * p.V;
    for (int i = 0; i < 4; ++i) { rows *= d.f[i]; m += rows * p.V * p.H * (i == 3 ? 2 : p.H); }
    return m;
}

int create_impl_sf(const uint8_t* blob, size_t nbytes, int device, mi355_shopformer** out) {
    if (!blob || !out) return fail(MI355_EINVAL, "null argument");
    Image im;
    int rc = parse_image(blob, nbytes, im); if (rc) return rc;
    std::unique_ptr<mi355_shopformer> h(new mi355_shopformer);
    SfParams& p = h->p;
    if ((rc = check_envelope(im, p)) || (rc = plan_tokenizer(p, &h->lds_bytes)) || (im.v2 && (rc = plan_transformer(p, &h->lds_tf)))) return rc;
    if (im.dec) {
        if ((rc = check_decoder_envelope(im, p, h->dp)) || (rc = plan_decoder(p, h->dp, &h->lds_dec))) return rc;
        h->has_dec = true;
        h->macs_dec = count_macs_decoder(p, h->dp);
    }
    // the tensor table is bound twice: against the host copy first, so that a missing or misshapen tensor is refused before the device
    // is touched, then against the uploaded copy
    if ((rc = check_adjacency(im, p)) || (rc = bind_tensors(im, im.data, h.get())) || (rc = upload(im, device, h.get())) ||
        (rc = bind_tensors(im, h->d_weights, h.get())))
        return rc;
    h->macs = count_macs(p);
    if ((rc = upload_params(h.get()))) return rc;
    *out = h.release();
    return MI355_OK;
}

// ---- scoring: the argument checks, the one launch sequence, the blocking calls' staging --------------------------------------------------
constexpr int kOutputsOld = (int)offsetof(mi355_shopformer_outputs_t, poses);      // the struct before the decoder's two pointers

struct Dst { float *scores, *token_scores, *tokens, *recon, *poses, *pose_error; };       // where a call's outputs go; each may be null

// GMC's return codes (dev_buf.h) as this unit's; a failed allocation leaves the buffer empty and the handle usable
int grow(Buf& b, size_t bytes) { return buf_grow(b, bytes) < 0 ? fail(MI355_EHIP, "hipMalloc: out of device memory for a Shopformer buffer") : MI355_OK; }
float* f32(const Buf& b) { return (float*)b.p; }

// every refusal the _ex entry points share, once, in the order they fire: the caller's struct (copied into the current layout: a caller
// compiled against the older, shorter struct has no decoder outputs), score_poses' own arguments, and what n > 0 windows need
struct PoseArgs { const void* poses; int dtype, P, V_src; const int* starts; int neck; };
int check_outputs(const mi355_shopformer* h, const mi355_shopformer_outputs_t* in, int n, Dst* d, const PoseArgs* pa = nullptr) {
    if (!in || (in->struct_size != (int)sizeof(mi355_shopformer_outputs_t) && in->struct_size != kOutputsOld))
        return fail(MI355_EINVAL, "mi355_shopformer_outputs_t: null or struct_size is not sizeof");
    mi355_shopformer_outputs_t o;
    std::memset(&o, 0, sizeof(o));
    std::memcpy(&o, in, (size_t)in->struct_size);
    if (!o.scores && !o.token_scores && !o.tokens && !o.recon && !o.poses && !o.pose_error) return fail(MI355_EINVAL, "mi355_shopformer_outputs_t: every output pointer is null");
    if (o.token_scores && h->p.variant != 2) return fail(MI355_EINVAL, "token_scores exist only for the shopformer_2 variant (version-2 images)");
    if ((o.poses || o.pose_error) && !h->has_dec) return fail(MI355_EINVAL, kNoDecoder);
    if (o.pose_error && !o.poses) return fail(MI355_EINVAL, "pose_error is written beside poses: set the poses output too");
    if (pa) { const int rc = pose_windows_validate(pa->poses, pa->dtype, pa->P, pa->V_src, pa->starts, n, h->p.T, h->p.V, pa->neck); if (rc) return rc; }
    if (n > 0 && h->p.variant != 2 && !o.scores) return fail(MI355_EINVAL, "the shopformer/ variant needs the scores output");
    *d = Dst{o.scores, o.token_scores, o.tokens, o.recon, o.poses, o.pose_error};
    return MI355_OK;
}

// THE launch sequence, for n > 0 windows and device pointers on `st`: the token destination (the caller's, else the handle's scratch,
// grown here; variant 1 needs one only for a tokens or poses output), the variant's launch(es), the decoder's when poses are asked for
int enqueue(mi355_shopformer* h, const float* win, int n, const Dst& d, hipStream_t st) {
    const SfParams& p = h->p;
    float* tok = d.tokens;
    if (!tok && (p.variant == 2 || d.poses)) {
        const int rc = grow(h->tok_scratch, (size_t)n * p.ntok * p.Din * 4); if (rc) return rc;
        tok = f32(h->tok_scratch);
    }
    if (p.variant == 2) KCHK(launch_shopformer2(h->d_params, p.G, p.GT, h->lds_bytes, h->lds_tf, win, n, tok, d.scores, d.token_scores, d.recon, st, &h->launches));
    else KCHK(launch_shopformer(h->d_params, p.G, win, n, d.scores, tok, d.recon, st, &h->launches));
    if (d.poses) KCHK(launch_shopformer_decoder(h->d_dec, h->dp.G, h->lds_dec, tok, n, d.poses, d.pose_error, win, st, &h->launches));
    return MI355_OK;
}

// n > 0 windows wait in h->win (enqueued on h->stream): a staging buffer for every output `out` (host pointers) asks for, grown here,
// plus what the launches need anyway (variant 1 always writes scores; the tokens whenever a launch reads them: this path never uses
// the device calls' scratch), the launch sequence, the downloads, and the wait for them
int run_blocking(mi355_shopformer* h, int n, const Dst& out) {
    const SfParams& p = h->p;
    const size_t tokb = (size_t)n * p.ntok * p.Din * 4, poseb = (size_t)n * 2 * p.T * p.V * 4;
    const struct { float* Dst::*m; Buf* buf; size_t bytes; bool internal; } parts[] = {
        {&Dst::scores, &h->score, (size_t)n * 4, p.variant != 2},
        {&Dst::token_scores, &h->tsc, (size_t)n * p.ntok * 4, false},
        {&Dst::tokens, &h->tok, tokb, p.variant == 2 || out.poses != nullptr},
        {&Dst::recon, &h->rec, tokb, false},
        {&Dst::poses, &h->pose, poseb, false},
        {&Dst::pose_error, &h->perr, poseb / 2, false},
    };
    Dst dev{};
    for (const auto& s : parts)
        if (out.*s.m || s.internal) { const int rc = grow(*s.buf, s.bytes); if (rc) return rc; dev.*s.m = f32(*s.buf); }
    const int rc = enqueue(h, f32(h->win), n, dev, h->stream); if (rc) return rc;
    for (const auto& s : parts)
        if (out.*s.m) HIPCHK(hipMemcpyAsync(out.*s.m, dev.*s.m, s.bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return MI355_OK;
}

}  // namespace

extern "C" {

int mi355_shopformer_create(const void* image, size_t nbytes, int device_id, mi355_shopformer** out) {
    return create_impl_sf((const uint8_t*)image, nbytes, device_id, out);
}

void mi355_shopformer_destroy(mi355_shopformer* h) { delete h; }

int mi355_shopformer_info(const mi355_shopformer* h, mi355_shopformer_info_t* info) {
    if (!h || !info) return fail(MI355_EINVAL, "null argument");
    std::memset(info, 0, sizeof(*info));
    const SfParams& p = h->p;
    info->num_keypoints = p.V; info->seq_len = p.T; info->hidden_channels = p.H; info->latent_channels = p.L; info->heads = p.heads;
    info->layers = p.layers; info->n_tokens = p.ntok; info->d_model = p.D; info->group = p.G; info->lds_bytes = h->lds_bytes;
    info->launches = h->launches; info->n_params = h->n_params; info->macs_per_window = h->macs;
    info->variant = p.variant; info->group_transformer = p.variant == 2 ? p.GT : p.G;
    return MI355_OK;
}

int mi355_shopformer_score_ex_device_async(mi355_shopformer* h, const float* windows_dev, int n, const mi355_shopformer_outputs_t* out,
                                           void* stream) {
    if (!h || n < 0 || (n > 0 && !windows_dev)) return fail(MI355_EINVAL, "null argument or negative count");
    Dst d;
    const int rc = check_outputs(h, out, n, &d); if (rc) return rc;
    if (n == 0) return MI355_OK;
    HIPCHK(hipSetDevice(h->device));
    return enqueue(h, windows_dev, n, d, (hipStream_t)stream);
}

int mi355_shopformer_score_ex(mi355_shopformer* h, const float* windows, int n, const mi355_shopformer_outputs_t* out) {
    if (!h || n < 0 || (n > 0 && !windows)) return fail(MI355_EINVAL, "null argument or negative count");
    Dst d;
    int rc = check_outputs(h, out, n, &d); if (rc) return rc;
    if (n == 0) return MI355_OK;
    HIPCHK(hipSetDevice(h->device));
    const size_t bytes = (size_t)n * 2 * h->p.T * h->p.V * 4;
    rc = grow(h->win, bytes); if (rc) return rc;
    HIPCHK(hipMemcpyAsync(h->win.p, windows, bytes, hipMemcpyHostToDevice, h->stream));
    return run_blocking(h, n, d);
}

// the forms from before the outputs struct: their own null check, then the _ex form
int mi355_shopformer_score_device_async(mi355_shopformer* h, const float* windows_dev, int n, float* scores_dev, float* tokens_dev,
                                        float* recon_dev, void* stream) {
    if (!h || n < 0 || (n > 0 && (!windows_dev || !scores_dev))) return fail(MI355_EINVAL, "null argument or negative count");
    if (n == 0) return MI355_OK;
    mi355_shopformer_outputs_t o{};
    o.struct_size = (int)sizeof(o); o.scores = scores_dev; o.tokens = tokens_dev; o.recon = recon_dev;
    return mi355_shopformer_score_ex_device_async(h, windows_dev, n, &o, stream);
}

int mi355_shopformer_score(mi355_shopformer* h, const float* windows, int n, float* scores, float* tokens, float* recon) {
    if (!h || n < 0 || (n > 0 && (!windows || !scores))) return fail(MI355_EINVAL, "null argument or negative count");
    if (n == 0) return MI355_OK;
    mi355_shopformer_outputs_t o{};
    o.struct_size = (int)sizeof(o); o.scores = scores; o.tokens = tokens; o.recon = recon;
    return mi355_shopformer_score_ex(h, windows, n, &o);
}

int mi355_shopformer_score_poses(mi355_shopformer* h, const void* poses, int dtype, int P, int V_src, const int* starts, int n, int neck,
                                 const mi355_shopformer_outputs_t* out) {
    if (!h) return fail(MI355_EINVAL, "null argument");
    Dst d;
    const PoseArgs pa{poses, dtype, P, V_src, starts, neck};
    int rc = check_outputs(h, out, n, &d, &pa); if (rc) return rc;
    if (n == 0) return MI355_OK;
    const SfParams& p = h->p;
    HIPCHK(hipSetDevice(h->device));
    const size_t pose_bytes = (size_t)P * V_src * 2 * (dtype == MI355_POSE_F64 ? 8 : 4);
    if ((rc = grow(h->win, (size_t)n * 2 * p.T * p.V * 4)) || (rc = grow(h->pose_in, pose_bytes)) || (rc = grow(h->starts, (size_t)n * 4))) return rc;
    HIPCHK(hipMemcpyAsync(h->pose_in.p, poses, pose_bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->starts.p, starts, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    KCHK(launch_pose_windows(h->pose_in.p, dtype, V_src, (const int*)h->starts.p, n, p.T, p.V, neck, f32(h->win), h->stream, &h->launches));
    return run_blocking(h, n, d);
}

int mi355_shopformer_decode_device_async(mi355_shopformer* h, const float* tokens_dev, int n, float* poses_dev, void* stream) {
    if (!h || n < 0 || (n > 0 && (!tokens_dev || !poses_dev))) return fail(MI355_EINVAL, "null argument or negative count");
    if (!h->has_dec) return fail(MI355_EINVAL, kNoDecoder);
    if (n == 0) return MI355_OK;
    HIPCHK(hipSetDevice(h->device));
    KCHK(launch_shopformer_decoder(h->d_dec, h->dp.G, h->lds_dec, tokens_dev, n, poses_dev, nullptr, nullptr, (hipStream_t)stream, &h->launches));
    return MI355_OK;
}

int mi355_shopformer_decode(mi355_shopformer* h, const float* tokens, int n, float* poses) {
    if (!h || n < 0 || (n > 0 && (!tokens || !poses))) return fail(MI355_EINVAL, "null argument or negative count");
    if (!h->has_dec) return fail(MI355_EINVAL, kNoDecoder);
    if (n == 0) return MI355_OK;
    HIPCHK(hipSetDevice(h->device));
    const SfParams& p = h->p;
    const size_t tokb = (size_t)n * p.ntok * p.Din * 4, poseb = (size_t)n * 2 * p.T * p.V * 4;
    int rc;
    if ((rc = grow(h->tok, tokb)) || (rc = grow(h->pose, poseb))) return rc;
    HIPCHK(hipMemcpyAsync(h->tok.p, tokens, tokb, hipMemcpyHostToDevice, h->stream));
    if ((rc = mi355_shopformer_decode_device_async(h, f32(h->tok), n, f32(h->pose), h->stream))) return rc;
    HIPCHK(hipMemcpyAsync(poses, h->pose.p, poseb, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return MI355_OK;
}

int mi355_shopformer_decoder_info(const mi355_shopformer* h, mi355_shopformer_decoder_info_t* info) {
    if (!h || !info) return fail(MI355_EINVAL, "null argument");
    if (!h->has_dec) return fail(MI355_EINVAL, kNoDecoder);
    std::memset(info, 0, sizeof(*info));
    for (int i = 0; i < 4; ++i) info->factors[i] = h->dp.f[i];
    info->frames = h->dp.Td; info->interpolate = h->dp.interp; info->group = h->dp.G; info->lds_bytes = h->lds_dec;
    info->macs_per_window = h->macs_dec;
    return MI355_OK;
}

}  // extern "C"
