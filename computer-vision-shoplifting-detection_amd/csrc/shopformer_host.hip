// Shopformer score path, host side: parse the weight image (cvsd_amd/shopformer.py:build_image), upload it, plan LDS, and the C ABI
// mi355_shopformer_* of include/mi355_yolo.h.  One kernel launch per call whatever the number of windows for variant 1, two for variant 2
// (version-2 images): tokenizer, then the transformer over row groups of up to 16 windows (shopformer_kernels.hip).
// Version-3 images hold either variant plus the GCAE decoder: one more launch (shopformer_decoder.hip), only when asked.
// mi355_shopformer_score_poses takes poses and window starts instead of windows: one launch more, pose_windows.hip.
#include "engine_internal.h"
#include "shopformer.h"
#include "pose_windows.h"

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
    float *d_win = nullptr, *d_score = nullptr, *d_tok = nullptr, *d_rec = nullptr, *d_tsc = nullptr;
    size_t cap = 0;                     // windows the staging buffers hold
    float* d_tok_scratch = nullptr;     // variant 2, device / async calls without a tokens output: where launch 1 leaves the tokens
    size_t scratch_cap = 0;
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
    float *d_pose = nullptr, *d_perr = nullptr;
    size_t cap_dec = 0;                 // windows d_pose / d_perr hold
    // mi355_shopformer_score_poses: the uploaded poses and window starts
    void* d_pose_in = nullptr;
    int* d_starts = nullptr;
    size_t cap_pose_in = 0, cap_starts = 0;     // bytes / entries
    ~mi355_shopformer() {
        if (d_weights) (void)hipFree(d_weights);
        if (d_params) (void)hipFree(d_params);
        if (d_dec) (void)hipFree(d_dec);
        for (float* q : {d_win, d_score, d_tok, d_rec, d_tsc, d_tok_scratch, d_pose, d_perr}) if (q) (void)hipFree(q);
        if (d_pose_in) (void)hipFree(d_pose_in);
        if (d_starts) (void)hipFree(d_starts);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace {

struct Entry { uint32_t kind, d[3]; uint64_t off, count; };
const char* kCfg[] = {"V", "T", "H", "L", "heads", "layers", "ff", "D", "ntok", "nnz", "s0", "s1", "s2", "s3", "T1", "T2", "T3", "T4"};
constexpr int kNCfg = 18;
constexpr int kNCfg2 = 24;             // version 2: + variant, Din, in_proj, out_proj, norm_kind, act_kind
constexpr int kNCfg3 = 30;             // version 3: + the decoder's four factors, the frames its layers emit, the interpolation flag
const char* kNoDecoder = "this Shopformer weight image was built without the decoder (build it with decoder=True)";

int pad_stride(int k) { int c = (k + 3) / 4 * 4; if (((c / 4) & 1) == 0) c += 4; return c; }   // 4 * odd

int in_set(int v, std::initializer_list<int> s) { for (int x : s) if (x == v) return 1; return 0; }

int create_impl_sf(const uint8_t* blob, size_t nbytes, int device, mi355_shopformer** out) {
    if (!blob || !out) return fail(MI355_EINVAL, "null argument");
    if (nbytes < 24 || std::memcmp(blob, "MI355SF1", 8) != 0) return fail(MI355_EFORMAT, "not a Shopformer weight image (bad magic)");
    uint32_t ver, ncfg;
    std::memcpy(&ver, blob + 8, 4); std::memcpy(&ncfg, blob + 12, 4);
    if (!((ver == 1 && ncfg == kNCfg) || (ver == 2 && ncfg == kNCfg2) || (ver == 3 && ncfg == kNCfg3))) return fail(MI355_EFORMAT, "unsupported Shopformer weight image version");
    size_t pos = 16;
    int cfg[kNCfg3] = {0};
    if (nbytes < pos + 4 * ncfg + 4) return fail(MI355_EFORMAT, "truncated Shopformer weight image");
    std::memcpy(cfg, blob + pos, 4 * ncfg); pos += 4 * ncfg;
    const bool v2 = ver == 2 || (ver == 3 && cfg[18] == 2);
    const bool dec = ver == 3;
    uint32_t nent; std::memcpy(&nent, blob + pos, 4); pos += 4;
    const size_t rec = 32 + 4 + 12 + 16;
    if (nent > 4096 || nbytes < pos + nent * rec) return fail(MI355_EFORMAT, "truncated Shopformer weight image");
    std::map<std::string, Entry> tab;
    for (uint32_t i = 0; i < nent; ++i) {
        const uint8_t* r = blob + pos + i * rec;
        char name[33] = {0}; std::memcpy(name, r, 32);
        Entry e; std::memcpy(&e.kind, r + 32, 4); std::memcpy(e.d, r + 36, 12); std::memcpy(&e.off, r + 48, 8); std::memcpy(&e.count, r + 56, 8);
        tab[name] = e;
    }
    pos += nent * rec; pos += (16 - pos % 16) % 16;
    const size_t nfloats = (nbytes - pos) / 4;
    for (auto& kv : tab)
        if (kv.second.off > nfloats || kv.second.count > nfloats - kv.second.off || kv.second.off % 4)       // no wrap; float4 reads
            return fail(MI355_EFORMAT, "Shopformer weight image: tensor '" + kv.first + "' lies outside the file");

    std::unique_ptr<mi355_shopformer> h(new mi355_shopformer);
    SfParams& p = h->p;
    p.V = cfg[0]; p.T = cfg[1]; p.H = cfg[2]; p.L = cfg[3]; p.heads = cfg[4]; p.layers = cfg[5]; p.ff = cfg[6]; p.D = cfg[7]; p.ntok = cfg[8]; p.nnz = cfg[9];
    for (int i = 0; i < 4; ++i) { p.s[i] = cfg[10 + i]; p.Tn[i + 1] = cfg[14 + i]; }
    p.Tn[0] = p.T;
    // the kernel's envelope (the Python loader refuses the same fields by name before an image is ever built)
    auto bad = [&](const char* f, int v) { return fail(MI355_EFORMAT, std::string("Shopformer weight image: unsupported ") + f + " = " + std::to_string(v)); };
    if (!in_set(p.V, {17, 18})) return bad("num_keypoints", p.V);
    if (!in_set(p.T, {12, 24})) return bad("seq_len", p.T);
    if (!in_set(p.H, {32, 64})) return bad("hidden_channels", p.H);
    if (!in_set(p.L, {4, 8})) return bad("latent_channels", p.L);
    if (dec && cfg[18] != 1 && cfg[18] != 2) return bad("variant", cfg[18]);
    if (dec && !v2 && (cfg[19] != p.D || cfg[20] || cfg[21] || cfg[22] != 0 || cfg[23] != 0)) return bad("variant-1 field in a version-3 image", cfg[19]);
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

    // LDS plan: the largest group of windows that fits (floats; every region a multiple of 4)
    auto plan = [&](int G, int* offs) {
        const int in = (G * p.T * p.V * 2 + 3) / 4 * 4;
        const int rows = G * p.ntok;
        const int tf = v2 ? 0 : rows * (5 * p.csD + p.csQ + p.csF) + (G * p.heads * p.ntok * p.ntok + 3) / 4 * 4;   // variant 2: its own launch
        const int P = std::max(G * p.Tn[1] * p.V * p.csH, tf);
        const int Q = G * std::max(p.Tn[2], p.Tn[4]) * p.V * p.csH;
        offs[0] = 0; offs[1] = in; offs[2] = 2 * in; offs[3] = 2 * in + P;
        return (2 * in + P + Q) * 4;
    };
    int offs[4], G = 0;
    for (int g = 8; g >= 1; --g) if (plan(g, offs) <= SF_LDS_BYTES) { G = g; break; }
    if (!G) return fail(MI355_EFORMAT, "Shopformer weight image: one window does not fit the 160 KiB of LDS");
    h->lds_bytes = plan(G, offs);
    p.G = G; p.offXin = offs[0]; p.offAx = offs[1]; p.offP = offs[2]; p.offQ = offs[3];
    if (v2) {
        // the transformer launch: state of the decoder, state of the encoder / memory, the normed copy, and one region that is
        // q|k|v + attention output during attention and the feed-forward hidden layer after it; up to 16 windows = 32 rows
        auto plan_tf = [&](int GT, int* o) {
            const int rows = GT * p.ntok, u = std::max(p.csQ + p.csD, p.csF);
            o[0] = 0; o[1] = rows * p.csD; o[2] = 2 * rows * p.csD; o[3] = 3 * rows * p.csD; o[4] = o[3] + rows * u;
            return (o[4] + (GT * p.heads * p.ntok * p.ntok + 3) / 4 * 4) * 4;
        };
        int o[5], GT = 0;
        for (int g : {16, 8, 4, 2, 1}) if (plan_tf(g, o) <= SF_LDS_BYTES) { GT = g; break; }
        if (!GT) return fail(MI355_EFORMAT, "Shopformer weight image: one window's tokens do not fit the 160 KiB of LDS");
        if (const char* e = std::getenv("MI355_SF2_ROW_GROUP")) {      // kernel experiments (row-group A/B of DESIGN.md 3.9); the product never sets it
            const int g = std::atoi(e);
            if (g >= 1 && g <= GT) GT = g;
        }
        h->lds_tf = plan_tf(GT, o);
        p.GT = GT; p.offTgt = o[0]; p.offX = o[1]; p.offNb = o[2]; p.offU = o[3]; p.offSc = o[4];
    }

    if (dec) {
        // the decoder's envelope: factors 1 or 2, a 1x1 last layer, the frame count they imply, at most the window's length
        SfDecParams& d = h->dp;
        d.V = p.V; d.T = p.T; d.H = p.H; d.L = p.L; d.ntok = p.ntok; d.Din = p.L * p.V;
        int frames = p.ntok;
        for (int i = 0; i < 4; ++i) {
            d.f[i] = cfg[24 + i];
            if (!in_set(d.f[i], {1, 2}) || (i == 3 && d.f[i] != 1)) return bad("decoder upsample factor", d.f[i]);
            frames *= d.f[i];
        }
        d.Td = cfg[28]; d.interp = cfg[29];
        if (d.Td != frames || d.Td > p.T) return bad("decoder frame count", d.Td);
        if (d.interp != (d.Td != p.T ? 1 : 0)) return bad("decoder interpolation flag", d.interp);
        if ((p.V * p.H) % 32) return bad("decoder initial_proj width", p.V * p.H);
        d.scale = (float)d.Td / (float)p.T;
        d.csT = pad_stride(d.Din); d.csH = pad_stride(p.H);
        // row group: G windows = G * ntok rows of initial_proj.  4 windows (8 or 12 rows of the 16-row tile) measured fastest: two
        // workgroups fit a CU's LDS, which gains more than the full tile of 5 or 8 windows
        auto plan_dec = [&](int G) {
            d.offTok = 0; d.offX = G * p.ntok * d.csT; d.offOut = d.offX + G * p.ntok * p.V * d.csH;
            return (d.offOut + (G * 2 * d.Td * p.V + 3) / 4 * 4) * 4;
        };
        int G = 4;
        if (const char* e = std::getenv("MI355_SFD_ROW_GROUP")) {      // kernel experiments (row-group A/B of DESIGN.md 3.11); the product never sets it
            const int g = std::atoi(e);
            if (g >= 1 && g <= 32) G = g;
        }
        while (G > 1 && plan_dec(G) > SF_LDS_BYTES) --G;
        if (plan_dec(G) > SF_LDS_BYTES) return fail(MI355_EFORMAT, "Shopformer weight image: one window's decoder rows do not fit the 160 KiB of LDS");
        d.G = G; h->lds_dec = plan_dec(G); h->has_dec = true;
        long long rows = p.ntok, m = (long long)p.ntok * d.Din * p.H * p.V;
        for (int i = 0; i < 4; ++i) { rows *= d.f[i]; m += rows * p.V * p.H * (i == 3 ? 2 : p.H); }
        h->macs_dec = m;
    }

    // adjacency columns must stay inside a pose (they index LDS rows)
    const float* data = (const float*)(blob + pos);
    bool missing = false; std::string miss;
    auto host = [&](const std::string& n) -> const Entry* { auto it = tab.find(n); if (it == tab.end()) { missing = true; miss = n; return nullptr; } return &it->second; };
    if (const Entry* e = host("adj_col")) {
        if (e->count < (uint64_t)p.V * p.nnz) return fail(MI355_EFORMAT, "Shopformer weight image: adjacency table too short");
        for (int i = 0; i < p.V * p.nnz; ++i) { const float c = data[e->off + i]; if (!(c >= 0.f && c <= (float)(p.V - 1)) || c != std::floor(c)) return fail(MI355_EFORMAT, "Shopformer weight image: adjacency column outside the pose"); }
    }
    // the tensor table is bound twice: against the host copy first, so that a missing or misshapen tensor is refused before the device
    // is touched, then against the uploaded copy
    const float* base = data;
    // packed: [tiles of 16 out][taps][blocks of 16 in][256]; plain: at least `need` floats
    auto packed = [&](const std::string& n, int co, int taps, int ci) -> const float* {
        const Entry* e = host(n); if (!e) return nullptr;
        const uint64_t want = (uint64_t)((co + 15) / 16) * taps * ((ci + 15) / 16) * 256;
        if (e->kind != 1 || (int)e->d[0] != co || (int)e->d[1] != taps || (int)e->d[2] != ci || e->count != want) { missing = true; miss = n + " (shape)"; return nullptr; }
        h->n_params += (long long)co * taps * ci;
        return base + e->off;
    };
    auto plain = [&](const std::string& n, int need) -> const float* {
        const Entry* e = host(n); if (!e) return nullptr;
        if (e->kind != 0 || e->count < (uint64_t)((need + 15) / 16 * 16)) { missing = true; miss = n + " (shape)"; return nullptr; }
        h->n_params += need;
        return base + e->off;
    };
    auto lin = [&](const std::string& n, int o, int i) { SfLin l; l.w = packed(n + ".w", o, 1, i); l.b = plain(n + ".b", o); return l; };
    auto norm = [&](const std::string& n) { SfNorm l; l.g = plain(n + ".g", p.D); l.b = plain(n + ".b", p.D); return l; };
    auto attn = [&](const std::string& n) { SfAttn a; a.q = lin(n + ".q", p.D, p.D); a.kv = lin(n + ".kv", 2 * p.D, p.D); a.out = lin(n + ".out", p.D, p.D); return a; };
    const int ch[5] = {2, p.H, p.H, p.H, p.L};
    auto bind = [&]() {
    h->n_params = 0;
    p.in_scale = plain("in_scale", 2 * p.V); p.in_shift = plain("in_shift", 2 * p.V);
    p.adj_col = plain("adj_col", p.V * p.nnz); p.adj_val = plain("adj_val", p.V * p.nnz);
    p.pe_in = plain("pe_in", p.ntok * p.D); p.pe_score = v2 ? nullptr : plain("pe_score", p.ntok * p.D);
    for (int b = 0; b < 4; ++b) {
        const std::string n = "b" + std::to_string(b);
        const bool conv_res = ch[b] != ch[b + 1] || p.s[b] != 1;
        SfBlock& k = p.blk[b];
        k.gw = b == 0 ? plain(n + ".gw", 2 * p.H) : packed(n + ".gw", ch[b + 1], 1, ch[b]);
        k.gb = plain(n + ".gb", ch[b + 1]);
        k.tw = packed(n + ".tw", ch[b + 1], 9, ch[b + 1]); k.tb = plain(n + ".tb", ch[b + 1]);
        k.rw = !conv_res ? nullptr : b == 0 ? plain(n + ".rw", 2 * p.H) : packed(n + ".rw", ch[b + 1], 1, ch[b]);
        k.rb = conv_res ? plain(n + ".rb", ch[b + 1]) : nullptr;
    }
    for (int e = 0; e < p.layers; ++e) {
        const std::string a = "e" + std::to_string(e), d = "d" + std::to_string(e);
        p.enc[e] = SfEnc{attn(a + ".sa"), norm(a + ".n1"), lin(a + ".f1", p.ff, p.D), lin(a + ".f2", p.D, p.ff), norm(a + ".n2")};
        p.dec[e] = SfDec{attn(d + ".sa"), norm(d + ".n1"), attn(d + ".ca"), norm(d + ".n2"), lin(d + ".f1", p.ff, p.D), lin(d + ".f2", p.D, p.ff), norm(d + ".n3")};
    }
    if (v2) {
        p.en = norm("en"); p.dn = norm("dn");
        if (p.in_proj) p.inp = lin("inp", p.D, p.Din);
        if (p.out_proj) p.outp = lin("outp", p.Din, p.D);
    } else {
        p.proj = lin("proj", p.D, p.D);
    }
    if (dec) {
        SfDecParams& d = h->dp;
        d.ipw = packed("dec.ip.w", p.V * p.H, 1, d.Din); d.ipb = plain("dec.ip.b", p.V * p.H);
        for (int i = 0; i < 4; ++i) {
            const std::string n = "dec.l" + std::to_string(i);
            d.w[i] = packed(n + ".w", i == 3 ? 2 : p.H, d.f[i], p.H); d.b[i] = plain(n + ".b", i == 3 ? 2 : p.H);
        }
    }
    };
    bind();
    if (missing) return fail(MI355_EFORMAT, "Shopformer weight image: tensor '" + miss + "' is missing or has the wrong shape");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(MI355_EHIP, "no HIP device: the Shopformer kernel needs an MI355X (there is no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(MI355_EINVAL, "device index out of range");
    h->device = device;
    HIPCHK(hipSetDevice(device));
    KCHK(prepare_shopformer_device());
    if (dec) KCHK(prepare_shopformer_decoder_device());
    HIPCHK(hipMalloc(&h->d_weights, std::max<size_t>(nfloats, 4) * 4));
    HIPCHK(hipMemcpy(h->d_weights, data, nfloats * 4, hipMemcpyHostToDevice));
    HIPCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    base = h->d_weights;
    bind();
    // multiply-accumulates per window, zero-padding taps not counted
    long long macs = 0;
    for (int b = 0; b < 4; ++b) {
        long long taps = 0;
        for (int to = 0; to < p.Tn[b + 1]; ++to) for (int k = 0; k < 9; ++k) { const int ti = to * p.s[b] + k - 4; taps += ti >= 0 && ti < p.Tn[b]; }
        macs += (long long)p.V * (taps * ch[b + 1] * ch[b + 1] + (long long)p.Tn[b] * ch[b] * ch[b + 1] + (p.blk[b].rw ? (long long)p.Tn[b + 1] * ch[b] * ch[b + 1] : 0));
    }
    const long long at = 4LL * p.D * p.D, ffm = 2LL * p.D * p.ff;
    macs += (long long)p.ntok * (p.layers * (at + ffm) + p.layers * (2 * at + ffm) + (v2 ? (long long)(p.in_proj + p.out_proj) * p.D * p.Din : (long long)p.D * p.D));
    h->macs = macs;
    HIPCHK(hipMalloc(&h->d_params, sizeof(SfParams)));
    HIPCHK(hipMemcpy(h->d_params, &p, sizeof(SfParams), hipMemcpyHostToDevice));
    if (dec) {
        HIPCHK(hipMalloc(&h->d_dec, sizeof(SfDecParams)));
        HIPCHK(hipMemcpy(h->d_dec, &h->dp, sizeof(SfDecParams), hipMemcpyHostToDevice));
    }
    *out = h.release();
    return MI355_OK;
}

int ensure_cap(mi355_shopformer* h, size_t n) {
    if (n <= h->cap) return MI355_OK;
    for (float** q : {&h->d_win, &h->d_score, &h->d_tok, &h->d_rec, &h->d_tsc}) { if (*q) (void)hipFree(*q); *q = nullptr; }
    h->cap = 0;
    const SfParams& p = h->p;
    HIPCHK(hipMalloc(&h->d_win, n * 2 * p.T * p.V * 4));
    HIPCHK(hipMalloc(&h->d_score, n * 4));
    HIPCHK(hipMalloc(&h->d_tok, n * p.ntok * p.Din * 4));
    HIPCHK(hipMalloc(&h->d_rec, n * p.ntok * p.Din * 4));
    HIPCHK(hipMalloc(&h->d_tsc, n * p.ntok * 4));
    h->cap = n;
    return MI355_OK;
}

int ensure_cap_dec(mi355_shopformer* h, size_t n) {
    if (n <= h->cap_dec) return MI355_OK;
    for (float** q : {&h->d_pose, &h->d_perr}) { if (*q) (void)hipFree(*q); *q = nullptr; }
    h->cap_dec = 0;
    const SfParams& p = h->p;
    HIPCHK(hipMalloc(&h->d_pose, n * 2 * p.T * p.V * 4));
    HIPCHK(hipMalloc(&h->d_perr, n * p.T * p.V * 4));
    h->cap_dec = n;
    return MI355_OK;
}

// device / async calls without a tokens output: the handle's scratch, grown here
int ensure_scratch(mi355_shopformer* h, size_t n) {
    if (n <= h->scratch_cap) return MI355_OK;
    if (h->d_tok_scratch) { (void)hipFree(h->d_tok_scratch); h->d_tok_scratch = nullptr; h->scratch_cap = 0; }
    HIPCHK(hipMalloc(&h->d_tok_scratch, n * h->p.ntok * h->p.Din * 4));
    h->scratch_cap = n;
    return MI355_OK;
}

int ensure_pose_in(mi355_shopformer* h, size_t bytes, size_t n) {
    if (bytes > h->cap_pose_in) {
        if (h->d_pose_in) { (void)hipFree(h->d_pose_in); h->d_pose_in = nullptr; h->cap_pose_in = 0; }
        HIPCHK(hipMalloc(&h->d_pose_in, bytes));
        h->cap_pose_in = bytes;
    }
    if (n > h->cap_starts) {
        if (h->d_starts) { (void)hipFree(h->d_starts); h->d_starts = nullptr; h->cap_starts = 0; }
        HIPCHK(hipMalloc(&h->d_starts, n * 4));
        h->cap_starts = n;
    }
    return MI355_OK;
}

constexpr int kOutputsOld = (int)offsetof(mi355_shopformer_outputs_t, poses);      // the struct before the decoder's two pointers

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

// checks the caller's struct and copies it into the current layout: a caller compiled against the older, shorter struct has no
// decoder outputs
static int outputs_ok(const mi355_shopformer* h, const mi355_shopformer_outputs_t* in, mi355_shopformer_outputs_t* o) {
    if (!in || (in->struct_size != (int)sizeof(mi355_shopformer_outputs_t) && in->struct_size != kOutputsOld))
        return fail(MI355_EINVAL, "mi355_shopformer_outputs_t: null or struct_size is not sizeof");
    std::memset(o, 0, sizeof(*o));
    std::memcpy(o, in, (size_t)in->struct_size);
    if (!o->scores && !o->token_scores && !o->tokens && !o->recon && !o->poses && !o->pose_error) return fail(MI355_EINVAL, "mi355_shopformer_outputs_t: every output pointer is null");
    if (o->token_scores && h->p.variant != 2) return fail(MI355_EINVAL, "token_scores exist only for the shopformer_2 variant (version-2 images)");
    if ((o->poses || o->pose_error) && !h->has_dec) return fail(MI355_EINVAL, kNoDecoder);
    if (o->pose_error && !o->poses) return fail(MI355_EINVAL, "pose_error is written beside poses: set the poses output too");
    return MI355_OK;
}

// variant 2 on device pointers: launch 1 leaves the tokens in the caller's buffer or, without one, in the handle's scratch (grown here)
static int run2_device(mi355_shopformer* h, const float* win, int n, float* scores, float* tsc, float* tok, float* rec, hipStream_t st) {
    const SfParams& p = h->p;
    if (!tok) {
        const int rc = ensure_scratch(h, (size_t)n); if (rc) return rc;
        tok = h->d_tok_scratch;
    }
    KCHK(launch_shopformer2(h->d_params, p.G, p.GT, h->lds_bytes, h->lds_tf, win, n, tok, scores, tsc, rec, st, &h->launches));
    return MI355_OK;
}

// n windows wait in h->d_win (enqueued on h->stream, the staging buffers large enough): the score launch(es), the decoder's when
// `out` asks for poses, the downloads into `out`'s host pointers, and the wait for them
static int score_staged(mi355_shopformer* h, int n, const mi355_shopformer_outputs_t* out) {
    const SfParams& p = h->p;
    const size_t per = (size_t)p.ntok * p.Din * 4;
    if (p.variant == 2) {
        const int rc = run2_device(h, h->d_win, n, out->scores ? h->d_score : nullptr, out->token_scores ? h->d_tsc : nullptr, h->d_tok,
                                   out->recon ? h->d_rec : nullptr, h->stream);
        if (rc) return rc;
    } else {
        KCHK(launch_shopformer(h->d_params, p.G, h->d_win, n, h->d_score, out->tokens || out->poses ? h->d_tok : nullptr,
                               out->recon ? h->d_rec : nullptr, h->stream, &h->launches));
    }
    if (out->poses) {
        KCHK(launch_shopformer_decoder(h->d_dec, h->dp.G, h->lds_dec, h->d_tok, n, h->d_pose, out->pose_error ? h->d_perr : nullptr, h->d_win,
                                       h->stream, &h->launches));
        HIPCHK(hipMemcpyAsync(out->poses, h->d_pose, (size_t)n * 2 * p.T * p.V * 4, hipMemcpyDeviceToHost, h->stream));
        if (out->pose_error) HIPCHK(hipMemcpyAsync(out->pose_error, h->d_perr, (size_t)n * p.T * p.V * 4, hipMemcpyDeviceToHost, h->stream));
    }
    if (out->scores) HIPCHK(hipMemcpyAsync(out->scores, h->d_score, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    if (out->token_scores) HIPCHK(hipMemcpyAsync(out->token_scores, h->d_tsc, (size_t)n * p.ntok * 4, hipMemcpyDeviceToHost, h->stream));
    if (out->tokens) HIPCHK(hipMemcpyAsync(out->tokens, h->d_tok, n * per, hipMemcpyDeviceToHost, h->stream));
    if (out->recon) HIPCHK(hipMemcpyAsync(out->recon, h->d_rec, n * per, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return MI355_OK;
}

int mi355_shopformer_score_ex_device_async(mi355_shopformer* h, const float* windows_dev, int n, const mi355_shopformer_outputs_t* out,
                                           void* stream) {
    if (!h || n < 0 || (n > 0 && !windows_dev)) return fail(MI355_EINVAL, "null argument or negative count");
    mi355_shopformer_outputs_t o;
    int rc = outputs_ok(h, out, &o); if (rc) return rc;
    if (n == 0) return MI355_OK;
    if (h->p.variant != 2 && !o.scores) return fail(MI355_EINVAL, "the shopformer/ variant needs the scores output");
    if (o.poses) {                      // the score path into a tokens buffer, then the decoder's one launch on it
        HIPCHK(hipSetDevice(h->device));
        float* tok = o.tokens;
        if (!tok) { rc = ensure_scratch(h, (size_t)n); if (rc) return rc; tok = h->d_tok_scratch; }
        if (h->p.variant == 2) { rc = run2_device(h, windows_dev, n, o.scores, o.token_scores, tok, o.recon, (hipStream_t)stream); if (rc) return rc; }
        else KCHK(launch_shopformer(h->d_params, h->p.G, windows_dev, n, o.scores, tok, o.recon, (hipStream_t)stream, &h->launches));
        KCHK(launch_shopformer_decoder(h->d_dec, h->dp.G, h->lds_dec, tok, n, o.poses, o.pose_error, windows_dev, (hipStream_t)stream, &h->launches));
        return MI355_OK;
    }
    if (h->p.variant != 2) return mi355_shopformer_score_device_async(h, windows_dev, n, o.scores, o.tokens, o.recon, stream);
    HIPCHK(hipSetDevice(h->device));
    return run2_device(h, windows_dev, n, o.scores, o.token_scores, o.tokens, o.recon, (hipStream_t)stream);
}

int mi355_shopformer_score_ex(mi355_shopformer* h, const float* windows, int n, const mi355_shopformer_outputs_t* out) {
    if (!h || n < 0 || (n > 0 && !windows)) return fail(MI355_EINVAL, "null argument or negative count");
    mi355_shopformer_outputs_t full;
    int rc = outputs_ok(h, out, &full); if (rc) return rc;
    out = &full;
    if (n == 0) return MI355_OK;
    if (h->p.variant != 2 && !out->scores) return fail(MI355_EINVAL, "the shopformer/ variant needs the scores output");
    if (h->p.variant != 2 && !out->poses) return mi355_shopformer_score(h, windows, n, out->scores, out->tokens, out->recon);
    HIPCHK(hipSetDevice(h->device));
    rc = ensure_cap(h, (size_t)n); if (rc) return rc;
    if (out->poses) { rc = ensure_cap_dec(h, (size_t)n); if (rc) return rc; }
    HIPCHK(hipMemcpyAsync(h->d_win, windows, (size_t)n * 2 * h->p.T * h->p.V * 4, hipMemcpyHostToDevice, h->stream));
    return score_staged(h, n, out);
}

int mi355_shopformer_score_device_async(mi355_shopformer* h, const float* windows_dev, int n, float* scores_dev, float* tokens_dev,
                                        float* recon_dev, void* stream) {
    if (!h || n < 0 || (n > 0 && (!windows_dev || !scores_dev))) return fail(MI355_EINVAL, "null argument or negative count");
    if (n == 0) return MI355_OK;
    HIPCHK(hipSetDevice(h->device));
    if (h->p.variant == 2) return run2_device(h, windows_dev, n, scores_dev, nullptr, tokens_dev, recon_dev, (hipStream_t)stream);
    KCHK(launch_shopformer(h->d_params, h->p.G, windows_dev, n, scores_dev, tokens_dev, recon_dev, (hipStream_t)stream, &h->launches));
    return MI355_OK;
}

int mi355_shopformer_score(mi355_shopformer* h, const float* windows, int n, float* scores, float* tokens, float* recon) {
    if (!h || n < 0 || (n > 0 && (!windows || !scores))) return fail(MI355_EINVAL, "null argument or negative count");
    if (n == 0) return MI355_OK;
    HIPCHK(hipSetDevice(h->device));
    if (h->p.variant == 2) {
        mi355_shopformer_outputs_t o{};
        o.struct_size = (int)sizeof(o); o.scores = scores; o.tokens = tokens; o.recon = recon;
        return mi355_shopformer_score_ex(h, windows, n, &o);
    }
    const int rc = ensure_cap(h, (size_t)n); if (rc) return rc;
    const SfParams& p = h->p;
    const size_t per = (size_t)p.ntok * p.D * 4;
    HIPCHK(hipMemcpyAsync(h->d_win, windows, (size_t)n * 2 * p.T * p.V * 4, hipMemcpyHostToDevice, h->stream));
    KCHK(launch_shopformer(h->d_params, p.G, h->d_win, n, h->d_score, tokens ? h->d_tok : nullptr, recon ? h->d_rec : nullptr, h->stream, &h->launches));
    HIPCHK(hipMemcpyAsync(scores, h->d_score, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    if (tokens) HIPCHK(hipMemcpyAsync(tokens, h->d_tok, n * per, hipMemcpyDeviceToHost, h->stream));
    if (recon) HIPCHK(hipMemcpyAsync(recon, h->d_rec, n * per, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return MI355_OK;
}

int mi355_shopformer_score_poses(mi355_shopformer* h, const void* poses, int dtype, int P, int V_src, const int* starts, int n, int neck,
                                 const mi355_shopformer_outputs_t* out) {
    if (!h) return fail(MI355_EINVAL, "null argument");
    mi355_shopformer_outputs_t full;
    int rc = outputs_ok(h, out, &full); if (rc) return rc;
    const SfParams& p = h->p;
    rc = pose_windows_validate(poses, dtype, P, V_src, starts, n, p.T, p.V, neck); if (rc) return rc;
    if (n == 0) return MI355_OK;
    if (p.variant != 2 && !full.scores) return fail(MI355_EINVAL, "the shopformer/ variant needs the scores output");
    HIPCHK(hipSetDevice(h->device));
    rc = ensure_cap(h, (size_t)n); if (rc) return rc;
    if (full.poses) { rc = ensure_cap_dec(h, (size_t)n); if (rc) return rc; }
    const size_t pose_bytes = (size_t)P * V_src * 2 * (dtype == MI355_POSE_F64 ? 8 : 4);
    rc = ensure_pose_in(h, pose_bytes, (size_t)n); if (rc) return rc;
    HIPCHK(hipMemcpyAsync(h->d_pose_in, poses, pose_bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_starts, starts, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    KCHK(launch_pose_windows(h->d_pose_in, dtype, V_src, h->d_starts, n, p.T, p.V, neck, h->d_win, h->stream, &h->launches));
    return score_staged(h, n, &full);
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
    int rc = ensure_cap(h, (size_t)n); if (rc) return rc;
    rc = ensure_cap_dec(h, (size_t)n); if (rc) return rc;
    const SfParams& p = h->p;
    HIPCHK(hipMemcpyAsync(h->d_tok, tokens, (size_t)n * p.ntok * p.Din * 4, hipMemcpyHostToDevice, h->stream));
    KCHK(launch_shopformer_decoder(h->d_dec, h->dp.G, h->lds_dec, h->d_tok, n, h->d_pose, nullptr, nullptr, h->stream, &h->launches));
    HIPCHK(hipMemcpyAsync(poses, h->d_pose, (size_t)n * 2 * p.T * p.V * 4, hipMemcpyDeviceToHost, h->stream));
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
