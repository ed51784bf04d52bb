// Shopformer score path: what the host unit (shopformer_host.hip) hands to the kernels (shopformer_kernels.hip).
// Variant 1 (shopformer/) is one kernel; variant 2 (shopformer_2/) is two: the tokenizer, then the transformer over larger row groups.
#pragma once
#include <hip/hip_runtime.h>

namespace mi355 {

constexpr int SF_MAX_LAYERS = 4;
constexpr int SF_MAX_V = 18;          // joints per pose the register-resident A.X step is unrolled for
constexpr int SF_THREADS = 512;       // 8 waves, 2 per SIMD
constexpr int SF_LDS_BYTES = 160 * 1024;

struct SfLin  { const float* w; const float* b; };      // w: packed A-operand fragments (shopformer.py:pack_mfma), b: bias padded to 16
struct SfNorm { const float* g; const float* b; };
struct SfAttn { SfLin q, kv, out; };
struct SfEnc  { SfAttn sa; SfNorm n1; SfLin f1, f2; SfNorm n2; };
struct SfDec  { SfAttn sa; SfNorm n1; SfAttn ca; SfNorm n2; SfLin f1, f2; SfNorm n3; };
struct SfBlock { const float *gw, *gb, *tw, *tb, *rw, *rb; };     // rw == nullptr: identity residual; block 0: gw / rw plain [H][2]

struct SfParams {
    int V, T, H, L, heads, layers, ff, D, ntok, nnz;
    int s[4], Tn[5];
    int G;                                 // windows per workgroup
    int csH, csD, csQ, csF;                // LDS row strides (floats), each 4 * odd: 16 rows of float4 reads hit 64 distinct banks
    int offXin, offAx, offP, offQ;         // LDS regions (floats): normalised input, A.X of it, ping, pong
    float att_scale;                       // 1 / sqrt(head_dim)
    const float *in_scale, *in_shift, *adj_col, *adj_val, *pe_in, *pe_score;
    SfBlock blk[4];
    SfEnc enc[SF_MAX_LAYERS];
    SfDec dec[SF_MAX_LAYERS];
    SfLin proj;
    // ---- variant 2 only (version-2 images).  D is d_model there, Din = L * V the token width; csD covers max(D, Din)
    int variant, Din, in_proj, out_proj;
    int GT;                                // windows per workgroup of the transformer launch (16 = two 16-row MFMA tiles of 2 tokens)
    int offTgt, offX, offNb, offU, offSc;  // LDS regions of the transformer launch (floats)
    SfLin inp, outp;                       // input / output projection (in_proj / out_proj)
    SfNorm en, dn;                         // final norms of the encoder and the decoder
};

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) for the CURRENT device (the attribute is per device): once per handle, at create
const char* prepare_shopformer_device();
// one launch for n windows, parameters in device memory; *launches is incremented per kernel launch; nullptr or the HIP error string
const char* launch_shopformer(const SfParams* p_dev, int group, const float* windows, int n, float* scores, float* tokens, float* recon,
                              hipStream_t stream, long long* launches);

// variant 2: launch 1 writes tokens [n][ntok][Din] to HBM (the caller's buffer or the handle's scratch), launch 2 reads them back in
// groups of GT windows and writes scores [n], token_scores [n][ntok] and recon [n][ntok][Din] (each may be nullptr); 2 launches
const char* launch_shopformer2(const SfParams* p_dev, int group, int group_tf, int lds_tok, int lds_tf, const float* windows, int n,
                               float* tokens, float* scores, float* token_scores, float* recon, hipStream_t stream, long long* launches);

// ---- the GCAE decoder (version-3 images): its own parameter block and its own launch (shopformer_decoder.hip)
struct SfDecParams {
    int V, T, H, L, ntok, Din;
    int f[4];                              // upsample factor of each layer (1 = 1x1 convolution, 2 = (2,1)/(2,1) transposed convolution)
    int Td, interp;                        // frames the layers emit = ntok * f0 * f1 * f2 * f3; Td != T: linear interpolation along time
    float scale;                           // (float)Td / (float)T, the source-index scale of align_corners=False
    int G;                                 // windows per workgroup: G * ntok rows of initial_proj
    int csT, csH;                          // LDS row strides (floats), each 4 * odd
    int offTok, offX, offOut;              // LDS regions (floats): tokens, initial_proj's output, the layers' output frames
    const float *ipw, *ipb;                // initial_proj, output features permuted to (joint, channel) order; packed / padded to 16
    const float *w[4], *b[4];              // layer matrices [out][parity][in] packed, folded BatchNorm in them and in the bias
};

const char* prepare_shopformer_decoder_device();
// one launch: tokens [n][ntok][Din] -> poses [n][2][T][V]; pose_error [n][T][V] when both it and `windows` [n][2][T][V] are given
const char* launch_shopformer_decoder(const SfDecParams* p_dev, int group, int lds_bytes, const float* tokens, int n, float* poses,
                                      float* pose_error, const float* windows, hipStream_t stream, long long* launches);

}  // namespace mi355
