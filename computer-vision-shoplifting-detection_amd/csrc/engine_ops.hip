// Single-operator entry points of include/mi355_yolo.h (host pointers in and out; the parity tests isolate a kernel with them).
#include <limits>
#include "engine_internal.h"

using namespace mi355;

extern "C" {

int mi355_op_letterbox(int device_id, const uint8_t* bgr, int n, int height, int width, int imgsz, uint8_t* out) {
    if (!bgr || !out || n <= 0 || height <= 0 || width <= 0 || imgsz <= 0) return fail(MI355_EINVAL, "bad argument");
    HIPCHK(hipSetDevice(device_id));
    const Geometry g = make_geometry(height, width, imgsz);
    DevMem dm; uint8_t *d_src, *d_dst; int *d_x, *d_y;
    std::vector<int> xt, yt;
    resize_table(g.Wr, g.w0, xt); resize_table(g.Hr, g.h0, yt);
    const size_t sb = (size_t)n * height * width * 3, db = (size_t)n * g.Hl * g.Wl * 3;
    HIPCHK(dm.alloc(&d_src, sb)); HIPCHK(dm.alloc(&d_dst, db)); HIPCHK(dm.alloc(&d_x, xt.size() * 4)); HIPCHK(dm.alloc(&d_y, yt.size() * 4));
    HIPCHK(hipMemcpy(d_src, bgr, sb, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_x, xt.data(), xt.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_y, yt.data(), yt.size() * 4, hipMemcpyHostToDevice));
    LetterboxArgs la{};
    la.src = d_src; la.H = height; la.W = width; la.frame_stride = (long long)height * width * 3; la.row_stride = width * 3;
    la.dst = d_dst; la.Hd = g.Hl; la.Wd = g.Wl; la.top = g.top; la.left = g.left; la.Hr = g.Hr; la.Wr = g.Wr;
    la.xtab = d_x; la.ytab = d_y; la.resize = g.resize ? 1 : 0; la.B = n;
    KCHK(launch_letterbox(la, nullptr));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, d_dst, db, hipMemcpyDeviceToHost));
    return MI355_OK;
}

static int op_conv2d_impl(int device_id, const float* x, int n, int h, int w, int cin, const float* w_oihw, const float* bias,
                          int cout, int k, int stride, int silu, const float* residual, float* y, int plan_index, int* n_plans,
                          bool half, bool out_f32, int sub_t0 = 0, int* sub_tile = nullptr) {
    // sub_t0 > 0 (fp32 3x3, stride 1): the launch runs over the cout tiles [sub_t0, last] alone, as the engine launches a merged head
    // conv's class couts in a sparse pass; y comes in holding what the other couts must still hold afterwards
    if (!x || !w_oihw || !bias || !y || n <= 0 || h <= 0 || w <= 0 || cin <= 0 || cout <= 0) return fail(MI355_EINVAL, "bad argument");
    if (!((k == 1 && stride == 1) || (k == 3 && (stride == 1 || stride == 2)))) return fail(MI355_EINVAL, "k/stride not supported");
    if ((h % stride) || (w % stride)) return fail(MI355_EINVAL, "h and w must be multiples of the stride");
    HIPCHK(hipSetDevice(device_id));
    const int ho = h / stride, wo = w / stride;
    const int es_in = half ? 2 : 4, es_out = (half && !out_f32) ? 2 : 4;
    const int cs_in = round_up(cin, 16 / es_in), cs_out = round_up(cout, 16 / es_out);
    const size_t npi = (size_t)n * h * w, npo = (size_t)n * ho * wo;
    // host images of the padded NHWC tensors, in the device dtype (fp32 -> fp16 is round-to-nearest-even)
    std::vector<float> xin(npi * cs_in, 0.f), yout(npo * cs_out, 0.f), rs;
    for (size_t p = 0; p < npi; ++p) std::memcpy(&xin[p * cs_in], x + p * cin, (size_t)cin * 4);
    auto upload = [&](float** dptr, DevMem& dm, const std::vector<float>& v, int es) -> int {
        HIPCHK(dm.alloc(dptr, v.size() * es));
        if (es == 4) { HIPCHK(hipMemcpy(*dptr, v.data(), v.size() * 4, hipMemcpyHostToDevice)); return MI355_OK; }
        std::vector<uint16_t> hb(v.size());
        floats_to_halfs(v.data(), hb.data(), v.size());
        HIPCHK(hipMemcpy(*dptr, hb.data(), hb.size() * 2, hipMemcpyHostToDevice));
        return MI355_OK;
    };
    DevMem dm; float *d_x, *d_y, *d_r = nullptr, *d_w, *d_b, *d_z;
    HIPCHK(dm.alloc(&d_z, 256)); HIPCHK(hipMemset(d_z, 0, 256));
    int rc = upload(&d_x, dm, xin, es_in); if (rc) return rc;
    HIPCHK(dm.alloc(&d_y, yout.size() * es_out));
    HIPCHK(hipMemset(d_y, 0, yout.size() * es_out));
    if (sub_t0 > 0) {
        for (size_t p = 0; p < npo; ++p) std::memcpy(&yout[p * cs_out], y + p * cout, (size_t)cout * 4);
        HIPCHK(hipMemcpy(d_y, yout.data(), yout.size() * 4, hipMemcpyHostToDevice));
    }
    if (residual) {
        rs.assign(npo * cs_out, 0.f);
        for (size_t p = 0; p < npo; ++p) std::memcpy(&rs[p * cs_out], residual + p * cout, (size_t)cout * 4);
        rc = upload(&d_r, dm, rs, es_out); if (rc) return rc;
    }
    std::vector<float> bp(round_up(cout, 16), 0.f);
    std::memcpy(bp.data(), bias, (size_t)cout * 4);
    HIPCHK(dm.alloc(&d_b, bp.size() * 4));
    HIPCHK(hipMemcpy(d_b, bp.data(), bp.size() * 4, hipMemcpyHostToDevice));
    if (half) {
        std::vector<uint16_t> pk(packed_weight_halfs(cout, cin, k));
        pack_conv_weights_f16(w_oihw, cout, cin, k, pk.data());
        HIPCHK(dm.alloc(&d_w, pk.size() * 2));
        HIPCHK(hipMemcpy(d_w, pk.data(), pk.size() * 2, hipMemcpyHostToDevice));
    } else {
        std::vector<float> pk(packed_weight_floats(cout, cin, k));
        pack_conv_weights(w_oihw, cout, cin, k, pk.data());
        HIPCHK(dm.alloc(&d_w, pk.size() * 4));
        HIPCHK(hipMemcpy(d_w, pk.data(), pk.size() * 4, hipMemcpyHostToDevice));
    }
    ConvArgs a{};
    a.src = d_x; a.src_cs = cs_in; a.dst = d_y; a.dst_cs = cs_out; a.res = d_r; a.res_cs = cs_out; a.wpk = d_w; a.bias = d_b;
    a.B = n; a.Hin = h; a.Win = w; a.Hout = ho; a.Wout = wo; a.Cin = cin; a.Cout = cout; a.k = k; a.stride = stride; a.pad = k / 2; a.act = silu ? 1 : 0;
    a.zeros = d_z; a.dtype = half ? 1 : 0; a.out_f32 = (half && out_f32) ? 1 : 0;
    const int nt = (cout + 15) / 16;
    if (sub_t0 > 0) a.sub_ctiles = nt - sub_t0;
    std::vector<ConvLaunch> cands;
    KCHK(plan_conv_candidates(a, &cands));
    // plan_index: which candidate launch plan to run (tests sweep it to cover every kernel variant and wave shape)
    ConvLaunch l = cands[(size_t)(plan_index < 0 ? 0 : plan_index) % cands.size()];
    if (n_plans) *n_plans = (int)cands.size();
    if (sub_t0 > 0) {
        if (l.version != 1 && l.version != 6) return fail(MI355_EINVAL, "sub-range launches exist for the 3x3 kernels only");
        l = cout_subrange(l, sub_t0, nt - sub_t0);
    }
    if (sub_tile) {
        const int f[MI355_PLAN_TILE_FIELDS] = {l.version, l.PT, l.CT, l.WP, l.a.TW, l.a.TH, l.a.cgroups, (int)l.grid_x, (int)l.grid_y};
        std::copy(f, f + MI355_PLAN_TILE_FIELDS, sub_tile);
    }
    KCHK(run_conv(l, nullptr));
    HIPCHK(hipDeviceSynchronize());
    if (es_out == 4) {
        HIPCHK(hipMemcpy(yout.data(), d_y, yout.size() * 4, hipMemcpyDeviceToHost));
    } else {
        std::vector<uint16_t> hb(yout.size());
        HIPCHK(hipMemcpy(hb.data(), d_y, hb.size() * 2, hipMemcpyDeviceToHost));
        halfs_to_floats(hb.data(), yout.data(), hb.size());
    }
    for (size_t p = 0; p < npo; ++p) std::memcpy(y + p * cout, &yout[p * cs_out], (size_t)cout * 4);
    return MI355_OK;
}

int mi355_op_dwconv2d(int device_id, const float* x, int n, int h, int w, int x_cs, int x_off, int c, const float* w_c1kk,
                      const float* bias, int k, int silu, const float* residual, int res_cs, int res_off, float* y, int y_cs, int y_off) {
    if (!x || !w_c1kk || !bias || !y || n <= 0 || h <= 0 || w <= 0 || c <= 0 || k != 3) return fail(MI355_EINVAL, "bad argument");
    auto view_ok = [&](int cs, int off) { return cs > 0 && off >= 0 && !(cs & 3) && !(off & 3) && off + round_up(c, 4) <= cs; };
    if (!view_ok(x_cs, x_off) || !view_ok(y_cs, y_off) || (residual && !view_ok(res_cs, res_off)))
        return fail(MI355_EINVAL, "views: strides / offsets must be multiples of 4 and the view (rounded up to 4 channels) inside the tensor");
    HIPCHK(hipSetDevice(device_id));
    const size_t np = (size_t)n * h * w;
    const int cp = round_up(c, 4), kk = k * k;
    std::vector<float> wt((size_t)kk * cp, 0.f), bp(cp, 0.f);
    for (int ch = 0; ch < c; ++ch)
        for (int t = 0; t < kk; ++t) wt[(size_t)t * cp + ch] = w_c1kk[(size_t)ch * kk + t];
    std::memcpy(bp.data(), bias, (size_t)c * 4);
    DevMem dm; float *d_x, *d_y, *d_r = nullptr, *d_w, *d_b;
    HIPCHK(dm.alloc(&d_x, np * x_cs * 4)); HIPCHK(hipMemcpy(d_x, x, np * x_cs * 4, hipMemcpyHostToDevice));
    HIPCHK(dm.alloc(&d_y, np * y_cs * 4)); HIPCHK(hipMemcpy(d_y, y, np * y_cs * 4, hipMemcpyHostToDevice));
    if (residual) { HIPCHK(dm.alloc(&d_r, np * res_cs * 4)); HIPCHK(hipMemcpy(d_r, residual, np * res_cs * 4, hipMemcpyHostToDevice)); }
    HIPCHK(dm.alloc(&d_w, wt.size() * 4)); HIPCHK(hipMemcpy(d_w, wt.data(), wt.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(dm.alloc(&d_b, bp.size() * 4)); HIPCHK(hipMemcpy(d_b, bp.data(), bp.size() * 4, hipMemcpyHostToDevice));
    DwConvArgs a{};
    a.src = d_x + x_off; a.src_cs = x_cs; a.dst = d_y + y_off; a.dst_cs = y_cs;
    if (residual) { a.res = d_r + res_off; a.res_cs = res_cs; }
    a.w = d_w; a.bias = d_b; a.B = n; a.H = h; a.W = w; a.C = c; a.k = k; a.act = silu ? 1 : 0; a.c_pad = cp;
    KCHK(launch_dwconv(a, nullptr));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(y, d_y, np * y_cs * 4, hipMemcpyDeviceToHost));
    return MI355_OK;
}

int mi355_op_decode(int device_id, const float* const* bufs, const int* geom, int n_levels, int n, int nc, int nkpt, int kdim,
                    int mode, int gate, float* pred, float* best, int* fallback_count) {
    if (!bufs || !geom || !pred || !best || n <= 0 || nc <= 0 || nkpt < 0) return fail(MI355_EINVAL, "bad argument");
    if (n_levels < 1 || n_levels > 4) return fail(MI355_EINVAL, "decode takes 1 to 4 levels");
    if (mode < 0 || mode > 2) return fail(MI355_EINVAL, "mode must be 0 (full), 1 (nms) or 2 (split)");
    if (nkpt ? (kdim != 2 && kdim != 3) : kdim != 0) return fail(MI355_EINVAL, "kdim must be 2 or 3 with keypoints and 0 without");
    const int nk = nkpt * kdim, no = 4 + nc + nk;
    DecodeArgs d{};
    long anchors = 0;
    for (int l = 0; l < n_levels; ++l) {
        const int* g = geom + 7 * l;           // cs, box_off, cls_off, kpt_off, h, w, stride
        if (!bufs[l] || g[0] <= 0 || g[4] <= 0 || g[5] <= 0 || g[6] <= 0) return fail(MI355_EINVAL, "bad level");
        if (g[1] < 0 || g[1] + 64 > g[0] || g[2] < 0 || g[2] + nc > g[0] || (nk && (g[3] < 0 || g[3] + nk > g[0])))
            return fail(MI355_EINVAL, "a level's box / class / keypoint slice lies outside its cs channels");
        d.lv[l].cs = g[0]; d.lv[l].box_off = g[1]; d.lv[l].cls_off = g[2]; d.lv[l].kpt_off = g[3];
        d.lv[l].H = g[4]; d.lv[l].W = g[5]; d.lv[l].stride = g[6]; d.lv[l].anchor0 = (int)anchors;
        anchors += (long)g[4] * g[5];
    }
    if (anchors * n * (long)no > (1l << 28)) return fail(MI355_EINVAL, "too many anchors");
    HIPCHK(hipSetDevice(device_id));
    DevMem dm; float *d_pred, *d_best; int* d_words;
    for (int l = 0; l < n_levels; ++l) {
        float* d_buf;
        const size_t bytes = (size_t)n * d.lv[l].H * d.lv[l].W * d.lv[l].cs * 4;
        HIPCHK(dm.alloc(&d_buf, bytes)); HIPCHK(hipMemcpy(d_buf, bufs[l], bytes, hipMemcpyHostToDevice));
        d.lv[l].buf = d_buf;
    }
    const size_t pn = (size_t)n * anchors * no, bn = (size_t)n * anchors * 2;
    HIPCHK(dm.alloc(&d_pred, pn * 4)); HIPCHK(hipMemcpy(d_pred, pred, pn * 4, hipMemcpyHostToDevice));
    HIPCHK(dm.alloc(&d_best, bn * 4)); HIPCHK(hipMemcpy(d_best, best, bn * 4, hipMemcpyHostToDevice));
    const int words[2] = {gate, 0};            // the gate word, the box stage's counter
    HIPCHK(dm.alloc(&d_words, sizeof(words))); HIPCHK(hipMemcpy(d_words, words, sizeof(words), hipMemcpyHostToDevice));
    d.n_levels = n_levels; d.B = n; d.A = (int)anchors; d.nc = nc; d.nkpt = nkpt; d.kdim = kdim;
    d.pred = d_pred; d.best = (float2*)d_best;
    if (mode == 2) {
        KCHK(launch_decode(d, false, nullptr, 1));
        d.gate = d_words; d.fallback_count = d_words + 1;
        KCHK(launch_decode(d, false, nullptr, 2));
    } else {
        KCHK(launch_decode(d, mode == 0, nullptr));
    }
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(pred, d_pred, pn * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(best, d_best, bn * 4, hipMemcpyDeviceToHost));
    if (fallback_count) HIPCHK(hipMemcpy(fallback_count, d_words + 1, sizeof(int), hipMemcpyDeviceToHost));
    return MI355_OK;
}

// The object-feature gather as a chunk enqueues it behind NMS (engine_run.hip:run_chunks), on rows that hold the caller's anchor_idx.
int mi355_op_obj_feats(int device_id, const void* const* bufs, const int* geom, int n_levels, int n, int half, const int* anchor_idx,
                       const int* counts, int cap, int dim, float* feats) {
    if (!bufs || !geom || !anchor_idx || !counts || !feats || n <= 0 || cap <= 0 || dim <= 0) return fail(MI355_EINVAL, "bad argument");
    if (n_levels < 1 || n_levels > 4) return fail(MI355_EINVAL, "obj_feats takes 1 to 4 levels");
    const int es = half ? 2 : 4, align = half ? 8 : 4;
    ObjFeatArgs a{};
    long anchors = 0; int cmin = 1 << 30;
    for (int l = 0; l < n_levels; ++l) {
        const int* g = geom + 5 * l;           // cs, c_off, C, h, w
        if (!bufs[l] || g[0] <= 0 || g[1] < 0 || g[2] <= 0 || g[1] + g[2] > g[0] || g[3] <= 0 || g[4] <= 0) return fail(MI355_EINVAL, "bad level");
        if ((g[0] % align) || (g[1] % align)) return fail(MI355_EINVAL, "a level's cs and c_off must be multiples of 4 (fp32) or 8 (fp16)");
        if (g[2] % dim) return fail(MI355_EINVAL, "dim must divide every level's channel count");
        if ((long)g[3] * g[4] * g[0] >= (1l << 31)) return fail(MI355_EINVAL, "a frame's map exceeds 32-bit offsets");
        a.lv[l] = ObjFeatLevel{nullptr, g[0], g[1], g[2], g[3], g[4], (int)anchors};
        anchors += (long)g[3] * g[4]; cmin = std::min(cmin, g[2]);
    }
    if (cmin != dim) return fail(MI355_EINVAL, "dim must be the smallest level's channel count");
    if (anchors >= (1l << 31) || (long)n * cap >= (1l << 28) || (long)cap * dim >= (1l << 31)) return fail(MI355_EINVAL, "too many anchors or rows");
    for (int i = 0; i < n; ++i) {
        if (counts[i] < 0 || counts[i] > cap) return fail(MI355_EINVAL, "counts must lie in 0 .. cap");
        for (int r = 0; r < counts[i]; ++r)
            if (anchor_idx[(size_t)i * cap + r] < 0 || anchor_idx[(size_t)i * cap + r] >= anchors) return fail(MI355_EINVAL, "anchor_idx outside 0 .. A-1");
    }
    HIPCHK(hipSetDevice(device_id));
    DevMem dm;
    for (int l = 0; l < n_levels; ++l) {
        char* d_buf;
        const size_t bytes = (size_t)n * a.lv[l].H * a.lv[l].W * a.lv[l].cs * es;
        HIPCHK(dm.alloc(&d_buf, bytes)); HIPCHK(hipMemcpy(d_buf, bufs[l], bytes, hipMemcpyHostToDevice));
        a.lv[l].base = d_buf;
    }
    std::vector<mi355_det> rows((size_t)n * cap);
    std::memset(rows.data(), 0, rows.size() * sizeof(mi355_det));
    for (size_t i = 0; i < rows.size(); ++i) rows[i].anchor_idx = anchor_idx[i];
    mi355_det* d_rows; int* d_counts; float* d_feats;
    const size_t fn = (size_t)n * cap * dim;
    HIPCHK(dm.alloc(&d_rows, rows.size() * sizeof(mi355_det))); HIPCHK(hipMemcpy(d_rows, rows.data(), rows.size() * sizeof(mi355_det), hipMemcpyHostToDevice));
    HIPCHK(dm.alloc(&d_counts, (size_t)n * 4)); HIPCHK(hipMemcpy(d_counts, counts, (size_t)n * 4, hipMemcpyHostToDevice));
    HIPCHK(dm.alloc(&d_feats, fn * 4)); HIPCHK(hipMemcpy(d_feats, feats, fn * 4, hipMemcpyHostToDevice));
    a.n_levels = n_levels; a.half = half ? 1 : 0; a.B = n; a.cap = cap; a.A = (int)anchors; a.dim = dim;
    a.rows = d_rows; a.row_words = (int)(sizeof(mi355_det) / 4); a.anchor_word = (int)(offsetof(mi355_det, anchor_idx) / 4);
    a.counts = d_counts; a.feats = d_feats;
    KCHK(launch_obj_feats(a, nullptr));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(feats, d_feats, fn * 4, hipMemcpyDeviceToHost));
    return MI355_OK;
}

// The sparse tail of a pass without its dense launches (engine_run.hip:launch_net): state zeroed, launch_sparse_lists,
// launch_sparse_box.  ptrs: 10 per level, geom: 11 per level (include/mi355_yolo.h).
int mi355_op_sparse_box(int device_id, void* const* ptrs, const int* geom, int n_levels, int n, const float* best, float conf,
                        const int* classes, int n_classes, int nc, int no, int act, float* pred, int* state) {
    if (!ptrs || !geom || !best || !pred || !state || n <= 0 || nc <= 0) return fail(MI355_EINVAL, "bad argument");
    if (n_levels < 1 || n_levels > 3) return fail(MI355_EINVAL, "sparse_box takes 1 to 3 levels");
    if (no < 4 + nc) return fail(MI355_EINVAL, "no must be at least 4 + nc");
    if (act < 0 || act > 2) return fail(MI355_EINVAL, "act must be 0 (none), 1 (SiLU) or 2 (fast SiLU)");
    SparseArgs sa{};
    struct Lv { int src_cs, src_off, cin, cout_a, mid_cs, mid_off; float* d_mid; size_t mid_floats; };
    Lv lv[3];
    long anchors = 0;
    for (int l = 0; l < n_levels; ++l) {
        const int* g = geom + 11 * l;          // h, w, src_cs, src_off, cin, cout_a, stride, mid_cs, mid_off, cap_dil, cap_cand
        void* const* p = ptrs + 10 * l;        // src, wA, bA, wB, bB, wC, bC, mid, dil, cand
        for (int i = 0; i < 10; ++i) if (!p[i]) return fail(MI355_EINVAL, "bad level: null pointer");
        const int h = g[0], w = g[1], stride = g[6];
        lv[l] = Lv{g[2], g[3], g[4], g[5], g[7], g[8], nullptr, 0};
        if (h <= 0 || w <= 0 || stride <= 0) return fail(MI355_EINVAL, "bad level");
        if (lv[l].cin <= 0 || (lv[l].cin & 15)) return fail(MI355_EINVAL, "cin must be a positive multiple of 16");
        if (lv[l].cout_a < 64) return fail(MI355_EINVAL, "cv2.i.0 needs at least 64 couts");
        auto view_ok = [](int cs, int off, int c) { return cs > 0 && off >= 0 && !(cs & 3) && !(off & 3) && off + c <= cs; };
        if (!view_ok(lv[l].src_cs, lv[l].src_off, lv[l].cin) || !view_ok(lv[l].mid_cs, lv[l].mid_off, 64))
            return fail(MI355_EINVAL, "views: strides / offsets must be multiples of 4 and the views (cin of src, 64 of mid) inside the tensors");
        const long pos = (long)n * h * w;
        if (pos > (1l << 24)) return fail(MI355_EINVAL, "too many positions");
        if (g[9] < 1 || g[10] < 1 || g[9] > pos || g[10] > pos) return fail(MI355_EINVAL, "list capacities must lie in 1 .. n*h*w");
        SparseLevel& L = sa.lv[l];
        L.src_cs = lv[l].src_cs; L.cib = lv[l].cin / 16; L.mid_cs = lv[l].mid_cs;
        L.H = h; L.W = w; L.stride = stride; L.anchor0 = (int)anchors; L.cap_dil = g[9]; L.cap_cand = g[10];
        anchors += (long)h * w;
    }
    if (anchors * n * (long)no > (1l << 28)) return fail(MI355_EINVAL, "too many anchors");
    std::vector<unsigned> mask;
    if (n_classes > 0 && classes) {
        mask.assign((nc + 31) / 32, 0u);
        for (int i = 0; i < n_classes; ++i) if (classes[i] >= 0 && classes[i] < nc) mask[classes[i] >> 5] |= 1u << (classes[i] & 31);
        // the lists kernel indexes the mask with best[]'s class: it must name a class
        for (long i = 0; i < anchors * n; ++i)
            if (!(best[2 * i + 1] >= 0.f && best[2 * i + 1] < (float)nc)) return fail(MI355_EINVAL, "best[] holds a class outside 0 .. nc-1");
    }
    HIPCHK(hipSetDevice(device_id));
    DevMem dm; float *d_pred, *d_best; int* d_state; unsigned* d_mask = nullptr;
    auto upload_conv = [&](const float* wt, const float* b, int co, int ci, int k, const float** dw, const float** db) -> int {
        std::vector<float> pk(packed_weight_floats(co, ci, k)), bp(round_up(co, 16), 0.f);
        pack_conv_weights(wt, co, ci, k, pk.data());
        std::memcpy(bp.data(), b, (size_t)co * 4);
        float *w_, *b_;
        HIPCHK(dm.alloc(&w_, pk.size() * 4)); HIPCHK(hipMemcpy(w_, pk.data(), pk.size() * 4, hipMemcpyHostToDevice));
        HIPCHK(dm.alloc(&b_, bp.size() * 4)); HIPCHK(hipMemcpy(b_, bp.data(), bp.size() * 4, hipMemcpyHostToDevice));
        *dw = w_; *db = b_;
        return MI355_OK;
    };
    for (int l = 0; l < n_levels; ++l) {
        void* const* p = ptrs + 10 * l;
        SparseLevel& L = sa.lv[l];
        const size_t np = (size_t)n * L.H * L.W;
        float* d_src;
        HIPCHK(dm.alloc(&d_src, np * L.src_cs * 4)); HIPCHK(hipMemcpy(d_src, p[0], np * L.src_cs * 4, hipMemcpyHostToDevice));
        lv[l].mid_floats = np * L.mid_cs;
        HIPCHK(dm.alloc(&lv[l].d_mid, lv[l].mid_floats * 4)); HIPCHK(hipMemcpy(lv[l].d_mid, p[7], lv[l].mid_floats * 4, hipMemcpyHostToDevice));
        L.src = d_src + lv[l].src_off; L.mid = lv[l].d_mid + lv[l].mid_off;
        // the whole (possibly merged cv2.i.0 | cv3.i.0) weight is packed; the kernel reads its first four cout tiles
        int rc = upload_conv((const float*)p[1], (const float*)p[2], lv[l].cout_a, lv[l].cin, 3, &L.wA, &L.biasA); if (rc) return rc;
        rc = upload_conv((const float*)p[3], (const float*)p[4], 64, 64, 3, &L.wB, &L.biasB); if (rc) return rc;
        rc = upload_conv((const float*)p[5], (const float*)p[6], 64, 64, 1, &L.wC, &L.biasC); if (rc) return rc;
        HIPCHK(dm.alloc(&L.dil, (size_t)L.cap_dil * 4)); HIPCHK(hipMemset(L.dil, 0xFF, (size_t)L.cap_dil * 4));
        HIPCHK(dm.alloc(&L.cand, (size_t)L.cap_cand * 4)); HIPCHK(hipMemset(L.cand, 0xFF, (size_t)L.cap_cand * 4));
    }
    const size_t pn = (size_t)n * anchors * no, bn = (size_t)n * anchors * 2;
    HIPCHK(dm.alloc(&d_pred, pn * 4)); HIPCHK(hipMemcpy(d_pred, pred, pn * 4, hipMemcpyHostToDevice));
    HIPCHK(dm.alloc(&d_best, bn * 4)); HIPCHK(hipMemcpy(d_best, best, bn * 4, hipMemcpyHostToDevice));
    HIPCHK(dm.alloc(&d_state, 16 * sizeof(int))); HIPCHK(hipMemset(d_state, 0xFF, 16 * sizeof(int)));     // whatever an earlier pass left
    if (!mask.empty()) { HIPCHK(dm.alloc(&d_mask, mask.size() * 4)); HIPCHK(hipMemcpy(d_mask, mask.data(), mask.size() * 4, hipMemcpyHostToDevice)); }
    sa.n_levels = n_levels; sa.B = n; sa.A = (int)anchors; sa.no = no; sa.act = act; sa.pred = d_pred; sa.best = (const float2*)d_best;
    sa.conf = conf; sa.class_mask = d_mask; sa.state = d_state;
    HIPCHK(hipMemsetAsync(d_state, 0, 12 * sizeof(int), nullptr));
    KCHK(launch_sparse_lists(sa, nullptr));
    KCHK(launch_sparse_box(sa, nullptr));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(state, d_state, 12 * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(pred, d_pred, pn * 4, hipMemcpyDeviceToHost));
    for (int l = 0; l < n_levels; ++l) {
        void* const* p = ptrs + 10 * l;
        const SparseLevel& L = sa.lv[l];
        HIPCHK(hipMemcpy(p[7], lv[l].d_mid, lv[l].mid_floats * 4, hipMemcpyDeviceToHost));
        const int nd = std::max(0, std::min(state[l], L.cap_dil)), ncd = std::max(0, std::min(state[4 + l], L.cap_cand));
        if (nd) HIPCHK(hipMemcpy(p[8], L.dil, (size_t)nd * 4, hipMemcpyDeviceToHost));
        if (ncd) HIPCHK(hipMemcpy(p[9], L.cand, (size_t)ncd * 4, hipMemcpyDeviceToHost));
    }
    return MI355_OK;
}

int mi355_op_sppf_pools(int device_id, const void* x, int n, int h, int w, int x_cs, int x_off, int c, void* y, int y_cs, int y_off,
                        int half) {
    if (!x || !y || n <= 0 || h <= 0 || w <= 0 || c <= 0) return fail(MI355_EINVAL, "bad argument");
    const int es = half ? 2 : 4, al = 16 / es;
    auto view_ok = [&](int cs, int off, int cv) { return cs > 0 && off >= 0 && !(cs % al) && !(off % al) && off + cv <= cs; };
    if ((c % al) || !view_ok(x_cs, x_off, c) || !view_ok(y_cs, y_off, 3 * c))
        return fail(MI355_EINVAL, "views: c, strides and offsets must be multiples of 16 bytes and the views (c in, 3c out) inside the tensors");
    HIPCHK(hipSetDevice(device_id));
    const size_t np = (size_t)n * h * w;
    DevMem dm; char *d_x, *d_y;
    HIPCHK(dm.alloc(&d_x, np * x_cs * es)); HIPCHK(hipMemcpy(d_x, x, np * x_cs * es, hipMemcpyHostToDevice));
    HIPCHK(dm.alloc(&d_y, np * y_cs * es)); HIPCHK(hipMemcpy(d_y, y, np * y_cs * es, hipMemcpyHostToDevice));
    if (half) KCHK(launch_sppf_pools_f16(d_x + (size_t)x_off * es, x_cs, d_y + (size_t)y_off * es, y_cs, n, h, w, c, nullptr));
    else KCHK(launch_sppf_pools((const float*)d_x + x_off, x_cs, (float*)d_y + y_off, y_cs, n, h, w, c, nullptr));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(y, d_y, np * y_cs * es, hipMemcpyDeviceToHost));
    return MI355_OK;
}

int mi355_op_upsample2x(int device_id, const uint32_t* x, int n, int h, int w, int x_cs, int x_off, int c, uint32_t* y, int y_cs,
                        int y_off) {
    if (!x || !y || n <= 0 || h <= 0 || w <= 0 || c <= 0) return fail(MI355_EINVAL, "bad argument");
    auto view_ok = [&](int cs, int off) { return cs > 0 && off >= 0 && !(cs & 3) && !(off & 3) && off + c <= cs; };
    if (!view_ok(x_cs, x_off) || !view_ok(y_cs, y_off))
        return fail(MI355_EINVAL, "views: strides / offsets must be multiples of 4 and the view inside the tensor");
    HIPCHK(hipSetDevice(device_id));
    const size_t np = (size_t)n * h * w;
    DevMem dm; float *d_x, *d_y;
    HIPCHK(dm.alloc(&d_x, np * x_cs * 4)); HIPCHK(hipMemcpy(d_x, x, np * x_cs * 4, hipMemcpyHostToDevice));
    HIPCHK(dm.alloc(&d_y, 4 * np * y_cs * 4)); HIPCHK(hipMemcpy(d_y, y, 4 * np * y_cs * 4, hipMemcpyHostToDevice));
    KCHK(launch_upsample2x(d_x + x_off, x_cs, d_y + y_off, y_cs, n, h, w, c, nullptr));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(y, d_y, 4 * np * y_cs * 4, hipMemcpyDeviceToHost));
    return MI355_OK;
}

int mi355_op_psa_attention(int device_id, const float* qkv, int n, int hw, int heads, int key_dim, int head_dim, float* y) {
    if (!qkv || !y || n <= 0 || hw <= 0 || heads <= 0) return fail(MI355_EINVAL, "bad argument");
    if (key_dim != 32 || head_dim != 64) return fail(MI355_EINVAL, "key_dim must be 32 and head_dim 64");
    HIPCHK(hipSetDevice(device_id));
    const size_t np = (size_t)n * hw;
    const int cin = heads * (2 * key_dim + head_dim), cout = heads * head_dim;
    DevMem dm; float *d_x, *d_y;
    HIPCHK(dm.alloc(&d_x, np * cin * 4)); HIPCHK(hipMemcpy(d_x, qkv, np * cin * 4, hipMemcpyHostToDevice));
    HIPCHK(dm.alloc(&d_y, np * cout * 4)); HIPCHK(hipMemset(d_y, 0, np * cout * 4));
    PsaAttnArgs a{};
    a.qkv = d_x; a.qkv_cs = cin; a.dst = d_y; a.dst_cs = cout;
    a.B = n; a.N = hw; a.heads = heads; a.key_dim = key_dim; a.head_dim = head_dim;
    a.scale = (float)(1.0 / std::sqrt((double)key_dim));
    KCHK(launch_psa_attention(a, nullptr));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(y, d_y, np * cout * 4, hipMemcpyDeviceToHost));
    return MI355_OK;
}

int mi355_op_conv2d(int device_id, const float* x, int n, int h, int w, int cin, const float* w_oihw, const float* bias,
                    int cout, int k, int stride, int silu, const float* residual, float* y, int plan_index, int* n_plans) {
    return op_conv2d_impl(device_id, x, n, h, w, cin, w_oihw, bias, cout, k, stride, silu, residual, y, plan_index, n_plans, false, false);
}

int mi355_op_conv2d_subrange(int device_id, const float* x, int n, int h, int w, int cin, const float* w_oihw, const float* bias,
                             int cout, int silu, int t0, float* y, int plan_index, int* n_plans, int* tile) {
    if (t0 <= 0 || t0 >= (cout + 15) / 16) return fail(MI355_EINVAL, "t0 must name a cout tile behind the first and inside the conv");
    return op_conv2d_impl(device_id, x, n, h, w, cin, w_oihw, bias, cout, 3, 1, silu, nullptr, y, plan_index, n_plans, false, false, t0, tile);
}

int mi355_op_conv2d_f16(int device_id, const float* x, int n, int h, int w, int cin, const float* w_oihw, const float* bias,
                        int cout, int k, int stride, int silu, const float* residual, float* y, int out_f32, int plan_index,
                        int* n_plans) {
    return op_conv2d_impl(device_id, x, n, h, w, cin, w_oihw, bias, cout, k, stride, silu, residual, y, plan_index, n_plans, true,
                          out_f32 != 0);
}

// Pointwise conv over cat(upsample2x(x_half), x_skip) with the upsample fused into the conv's read side (fp32): the parity hook of the
// neck's Upsample -> Concat -> C2f.cv1 chain as the engine runs it (the up channels of the concat buffer are never written: they
// are poisoned here, so a plan that reads them shows).
static int op_conv1x1_upcat_impl(int device_id, const float* x_half, const float* x_skip, int n, int h, int w, int up_c, int skip_c,
                                 const float* w_oihw, const float* bias, int cout, int silu, float* y, int plan_index, int* n_plans, bool half) {
    if (!x_half || !x_skip || !w_oihw || !bias || !y || n <= 0 || h <= 0 || w <= 0 || up_c <= 0 || skip_c <= 0 || cout <= 0) return fail(MI355_EINVAL, "bad argument");
    if ((h & 1) || (w & 1) || (up_c & 15)) return fail(MI355_EINVAL, "h and w must be even and up_c a multiple of 16");
    HIPCHK(hipSetDevice(device_id));
    const int es = half ? 2 : 4, al = 16 / es;
    const int cin = up_c + skip_c, cs_in = round_up(cin, al), cs_h = round_up(up_c, al), cs_out = round_up(cout, al);
    const size_t np = (size_t)n * h * w, nph = np / 4;
    std::vector<float> xin(np * cs_in, 0.f), xh(nph * cs_h, 0.f), yout(np * cs_out, 0.f);
    const float poison = std::numeric_limits<float>::quiet_NaN();
    for (size_t p = 0; p < np; ++p) {
        for (int c = 0; c < up_c; ++c) xin[p * cs_in + c] = poison;
        std::memcpy(&xin[p * cs_in + up_c], x_skip + p * skip_c, (size_t)skip_c * 4);
    }
    for (size_t p = 0; p < nph; ++p) std::memcpy(&xh[p * cs_h], x_half + p * up_c, (size_t)up_c * 4);
    DevMem dm; float *d_x, *d_h, *d_y, *d_w, *d_b, *d_z;
    HIPCHK(dm.alloc(&d_z, 256)); HIPCHK(hipMemset(d_z, 0, 256));
    auto upload = [&](float** dptr, const std::vector<float>& v) -> int {
        HIPCHK(dm.alloc(dptr, v.size() * es));
        if (!half) { HIPCHK(hipMemcpy(*dptr, v.data(), v.size() * 4, hipMemcpyHostToDevice)); return MI355_OK; }
        std::vector<uint16_t> hb(v.size());
        floats_to_halfs(v.data(), hb.data(), v.size());
        HIPCHK(hipMemcpy(*dptr, hb.data(), hb.size() * 2, hipMemcpyHostToDevice));
        return MI355_OK;
    };
    int rc = upload(&d_x, xin); if (rc) return rc;
    rc = upload(&d_h, xh); if (rc) return rc;
    HIPCHK(dm.alloc(&d_y, yout.size() * es)); HIPCHK(hipMemset(d_y, 0, yout.size() * es));
    std::vector<float> bp(round_up(cout, 16), 0.f);
    std::memcpy(bp.data(), bias, (size_t)cout * 4);
    if (half) {
        std::vector<uint16_t> pk(packed_weight_halfs(cout, cin, 1));
        pack_conv_weights_f16(w_oihw, cout, cin, 1, pk.data());
        HIPCHK(dm.alloc(&d_w, pk.size() * 2)); HIPCHK(hipMemcpy(d_w, pk.data(), pk.size() * 2, hipMemcpyHostToDevice));
    } else {
        std::vector<float> pk(packed_weight_floats(cout, cin, 1));
        pack_conv_weights(w_oihw, cout, cin, 1, pk.data());
        HIPCHK(dm.alloc(&d_w, pk.size() * 4)); HIPCHK(hipMemcpy(d_w, pk.data(), pk.size() * 4, hipMemcpyHostToDevice));
    }
    HIPCHK(dm.alloc(&d_b, bp.size() * 4)); HIPCHK(hipMemcpy(d_b, bp.data(), bp.size() * 4, hipMemcpyHostToDevice));
    ConvArgs a{};
    a.src = d_x; a.src_cs = cs_in; a.dst = d_y; a.dst_cs = cs_out; a.wpk = d_w; a.bias = d_b; a.zeros = d_z;
    a.src2 = d_h; a.src2_cs = cs_h; a.up_c = up_c; a.dtype = half ? 1 : 0;
    a.B = n; a.Hin = h; a.Win = w; a.Hout = h; a.Wout = w; a.Cin = cin; a.Cout = cout; a.k = 1; a.stride = 1; a.pad = 0; a.act = silu ? 1 : 0;
    std::vector<ConvLaunch> cands;
    KCHK(plan_conv_candidates(a, &cands));
    const ConvLaunch& l = cands[(size_t)(plan_index < 0 ? 0 : plan_index) % cands.size()];
    if (n_plans) *n_plans = (int)cands.size();
    KCHK(run_conv(l, nullptr));
    HIPCHK(hipDeviceSynchronize());
    if (!half) {
        HIPCHK(hipMemcpy(yout.data(), d_y, yout.size() * 4, hipMemcpyDeviceToHost));
    } else {
        std::vector<uint16_t> hb(yout.size());
        HIPCHK(hipMemcpy(hb.data(), d_y, hb.size() * 2, hipMemcpyDeviceToHost));
        halfs_to_floats(hb.data(), yout.data(), hb.size());
    }
    for (size_t p = 0; p < np; ++p) std::memcpy(y + p * cout, &yout[p * cs_out], (size_t)cout * 4);
    return MI355_OK;
}

int mi355_op_conv1x1_upcat(int device_id, const float* x_half, const float* x_skip, int n, int h, int w, int up_c, int skip_c,
                           const float* w_oihw, const float* bias, int cout, int silu, float* y, int plan_index, int* n_plans) {
    return op_conv1x1_upcat_impl(device_id, x_half, x_skip, n, h, w, up_c, skip_c, w_oihw, bias, cout, silu, y, plan_index, n_plans, false);
}

int mi355_op_conv1x1_upcat_f16(int device_id, const float* x_half, const float* x_skip, int n, int h, int w, int up_c, int skip_c,
                               const float* w_oihw, const float* bias, int cout, int silu, float* y, int plan_index, int* n_plans) {
    return op_conv1x1_upcat_impl(device_id, x_half, x_skip, n, h, w, up_c, skip_c, w_oihw, bias, cout, silu, y, plan_index, n_plans, true);
}

// Conv3x3 (+bias+SiLU) -> Conv1x1 (+bias, optional SiLU) as ONE fused launch (conv_igemm_f32 / _f16 <..., F2 = true>): the parity
// hook of the fused pairs the engine runs (stride-2 conv -> C2f.cv1, head branch [1] -> [2]).
static int op_conv2d_fused_impl(int device_id, const float* x, int n, int h, int w, int cin, const float* w1_oihw, const float* b1, int c1,
                                int stride, const float* w2_oihw, const float* b2, int c2, int silu2, float* y, int plan_index, int* n_plans,
                                bool half, bool out_f32, const float* residual = nullptr, const float* lead = nullptr, int lead_c = 0) {
    if (!x || !w1_oihw || !b1 || !w2_oihw || !b2 || !y || n <= 0 || h <= 0 || w <= 0 || cin <= 0 || c1 <= 0 || c2 <= 0) return fail(MI355_EINVAL, "bad argument");
    if ((stride != 1 && stride != 2) || (h % stride) || (w % stride)) return fail(MI355_EINVAL, "stride must be 1 or 2 and divide h and w");
    HIPCHK(hipSetDevice(device_id));
    const int ho = h / stride, wo = w / stride;
    const int es_in = half ? 2 : 4, es_out = (half && !out_f32) ? 2 : 4;
    const int cs_in = round_up(cin, 16 / es_in), cs_out = round_up(c2, 16 / es_out), cs_mid = round_up(c1, 16 / es_in);
    const size_t npi = (size_t)n * h * w, npo = (size_t)n * ho * wo;
    std::vector<float> xin(npi * cs_in, 0.f), yout(npo * cs_out, 0.f);
    for (size_t p = 0; p < npi; ++p) std::memcpy(&xin[p * cs_in], x + p * cin, (size_t)cin * 4);
    DevMem dm; float *d_x, *d_y, *d_w1, *d_b1, *d_w2, *d_b2, *d_z, *d_mid;
    HIPCHK(dm.alloc(&d_z, 256)); HIPCHK(hipMemset(d_z, 0, 256));
    HIPCHK(dm.alloc(&d_x, xin.size() * es_in));
    if (half) {
        std::vector<uint16_t> hb(xin.size());
        floats_to_halfs(xin.data(), hb.data(), xin.size());
        HIPCHK(hipMemcpy(d_x, hb.data(), hb.size() * 2, hipMemcpyHostToDevice));
    } else {
        HIPCHK(hipMemcpy(d_x, xin.data(), xin.size() * 4, hipMemcpyHostToDevice));
    }
    HIPCHK(dm.alloc(&d_y, yout.size() * es_out)); HIPCHK(hipMemset(d_y, 0, yout.size() * es_out));
    HIPCHK(dm.alloc(&d_mid, npo * cs_mid * es_in));               // the unfused destination of the first conv: must stay untouched
    HIPCHK(hipMemset(d_mid, 0, npo * cs_mid * es_in));
    auto upload_conv = [&](const float* wt, const float* b, int co, int ci, int k, float** dw, float** db) -> int {
        std::vector<float> bp(round_up(co, 16), 0.f);
        std::memcpy(bp.data(), b, (size_t)co * 4);
        if (half) {
            std::vector<uint16_t> pk(packed_weight_halfs(co, ci, k));
            pack_conv_weights_f16(wt, co, ci, k, pk.data());
            HIPCHK(dm.alloc(dw, pk.size() * 2)); HIPCHK(hipMemcpy(*dw, pk.data(), pk.size() * 2, hipMemcpyHostToDevice));
        } else {
            std::vector<float> pk(packed_weight_floats(co, ci, k));
            pack_conv_weights(wt, co, ci, k, pk.data());
            HIPCHK(dm.alloc(dw, pk.size() * 4)); HIPCHK(hipMemcpy(*dw, pk.data(), pk.size() * 4, hipMemcpyHostToDevice));
        }
        HIPCHK(dm.alloc(db, bp.size() * 4)); HIPCHK(hipMemcpy(*db, bp.data(), bp.size() * 4, hipMemcpyHostToDevice));
        return MI355_OK;
    };
    if ((residual || lead_c) && half) return fail(MI355_EINVAL, "residual / lead channels exist in the fp32 fused kernel only");
    if (lead_c < 0 || (lead_c > 0 && !lead)) return fail(MI355_EINVAL, "bad lead argument");
    int rc = upload_conv(w1_oihw, b1, c1, cin, 3, &d_w1, &d_b1); if (rc) return rc;
    rc = upload_conv(w2_oihw, b2, c2, lead_c + c1, 1, &d_w2, &d_b2); if (rc) return rc;       // pointwise weights over cat(lead, conv1 output)
    ConvArgs a{};
    // lead channels and the first conv's (unused) destination share ONE buffer [lead | mid], as the C2f concat buffer does
    float* d_cat = nullptr; float* d_res = nullptr;
    const int cs_cat = round_up(lead_c + c1, 4);
    if (lead_c) {
        std::vector<float> cat(npo * cs_cat, 0.f);
        for (size_t p = 0; p < npo; ++p) std::memcpy(&cat[p * cs_cat], lead + p * lead_c, (size_t)lead_c * 4);
        HIPCHK(dm.alloc(&d_cat, cat.size() * 4)); HIPCHK(hipMemcpy(d_cat, cat.data(), cat.size() * 4, hipMemcpyHostToDevice));
    }
    if (residual) {
        std::vector<float> rs(npo * cs_mid, 0.f);
        for (size_t p = 0; p < npo; ++p) std::memcpy(&rs[p * cs_mid], residual + p * c1, (size_t)c1 * 4);
        HIPCHK(dm.alloc(&d_res, rs.size() * 4)); HIPCHK(hipMemcpy(d_res, rs.data(), rs.size() * 4, hipMemcpyHostToDevice));
        a.res = d_res; a.res_cs = cs_mid;
    }
    if (lead_c) { a.f2_lead = d_cat; a.f2_lead_cs = cs_cat; a.f2_lead_c = lead_c; }
    a.src = d_x; a.src_cs = cs_in; a.dst = lead_c ? d_cat + lead_c : d_mid; a.dst_cs = lead_c ? cs_cat : cs_mid; a.wpk = d_w1; a.bias = d_b1; a.zeros = d_z;
    a.B = n; a.Hin = h; a.Win = w; a.Hout = ho; a.Wout = wo; a.Cin = cin; a.Cout = c1; a.k = 3; a.stride = stride; a.pad = 1; a.act = 1;
    a.dtype = half ? 1 : 0;
    a.f2_wpk = d_w2; a.f2_bias = d_b2; a.f2_dst = d_y; a.f2_dst_cs = cs_out; a.f2_cout = c2; a.f2_act = silu2 ? 1 : 0;
    a.f2_out_f32 = (half && out_f32) ? 1 : 0;
    std::vector<ConvLaunch> cands;
    KCHK(plan_conv_candidates(a, &cands));
    if (n_plans) *n_plans = (int)cands.size();
    KCHK(run_conv(cands[(size_t)(plan_index < 0 ? 0 : plan_index) % cands.size()], nullptr));
    HIPCHK(hipDeviceSynchronize());
    if (es_out == 4) {
        HIPCHK(hipMemcpy(yout.data(), d_y, yout.size() * 4, hipMemcpyDeviceToHost));
    } else {
        std::vector<uint16_t> hb(yout.size());
        HIPCHK(hipMemcpy(hb.data(), d_y, hb.size() * 2, hipMemcpyDeviceToHost));
        halfs_to_floats(hb.data(), yout.data(), hb.size());
    }
    for (size_t p = 0; p < npo; ++p) std::memcpy(y + p * c2, &yout[p * cs_out], (size_t)c2 * 4);
    return MI355_OK;
}

// Two independent convs (same input tensor, different weights) run as ONE grouped launch (conv_f32_group.hip) with candidate
// plans plan_a / plan_b (indices into each conv's candidate list, skipping plans whose kernel is not on the group kernel's
// menu: *n_menu_a / *n_menu_b return how many are): the parity hook of the grouped launches -- must equal mi355_op_conv2d of each.
int mi355_op_conv2d_group(int device_id, const float* x, int n, int h, int w, int cin, const float* wa, const float* ba, int cout_a, int k_a,
                          int stride_a, const float* wb, const float* bb, int cout_b, int k_b, int stride_b, float* ya, float* yb, int plan_a,
                          int plan_b, int* n_menu_a, int* n_menu_b, const float* w2a, const float* b2a, int cout2_a) {
    if (!x || !wa || !ba || !wb || !bb || !ya || !yb || n <= 0 || h <= 0 || w <= 0 || cin <= 0 || cout_a <= 0 || cout_b <= 0) return fail(MI355_EINVAL, "bad argument");
    if (cout2_a > 0 && (!w2a || !b2a || k_a != 3)) return fail(MI355_EINVAL, "the fused pointwise stage needs weights and a 3x3 first conv");
    HIPCHK(hipSetDevice(device_id));
    const int cs_in = round_up(cin, 4);
    const size_t npi = (size_t)n * h * w;
    std::vector<float> xin(npi * cs_in, 0.f);
    for (size_t p = 0; p < npi; ++p) std::memcpy(&xin[p * cs_in], x + p * cin, (size_t)cin * 4);
    DevMem dm; float *d_x, *d_z;
    HIPCHK(dm.alloc(&d_z, 256)); HIPCHK(hipMemset(d_z, 0, 256));
    HIPCHK(dm.alloc(&d_x, xin.size() * 4)); HIPCHK(hipMemcpy(d_x, xin.data(), xin.size() * 4, hipMemcpyHostToDevice));
    struct One { const float* w; const float* b; int cout, k, stride; float* y; int cout2; float* d_y; int cs_out; size_t npo; std::vector<ConvLaunch> menu; std::vector<int> kinds; };
    One c[2] = {{wa, ba, cout_a, k_a, stride_a, ya, cout2_a > 0 ? cout2_a : 0}, {wb, bb, cout_b, k_b, stride_b, yb, 0}};
    for (One& o : c) {
        if (!((o.k == 1 && o.stride == 1) || (o.k == 3 && (o.stride == 1 || o.stride == 2))) || (h % o.stride) || (w % o.stride)) return fail(MI355_EINVAL, "k/stride not supported");
        const int c_final = o.cout2 ? o.cout2 : o.cout;                 // channels of the tensor that is written
        o.cs_out = round_up(c_final, 4); o.npo = (size_t)n * (h / o.stride) * (w / o.stride);
        float *d_w, *d_b;
        std::vector<float> pk(packed_weight_floats(o.cout, cin, o.k)), bp(round_up(o.cout, 16), 0.f);
        pack_conv_weights(o.w, o.cout, cin, o.k, pk.data());
        std::memcpy(bp.data(), o.b, (size_t)o.cout * 4);
        HIPCHK(dm.alloc(&d_w, pk.size() * 4)); HIPCHK(hipMemcpy(d_w, pk.data(), pk.size() * 4, hipMemcpyHostToDevice));
        HIPCHK(dm.alloc(&d_b, bp.size() * 4)); HIPCHK(hipMemcpy(d_b, bp.data(), bp.size() * 4, hipMemcpyHostToDevice));
        HIPCHK(dm.alloc(&o.d_y, o.npo * o.cs_out * 4)); HIPCHK(hipMemset(o.d_y, 0, o.npo * o.cs_out * 4));
        ConvArgs a{};
        a.src = d_x; a.src_cs = cs_in; a.dst = o.d_y; a.dst_cs = o.cs_out; a.wpk = d_w; a.bias = d_b; a.zeros = d_z;
        a.B = n; a.Hin = h; a.Win = w; a.Hout = h / o.stride; a.Wout = w / o.stride; a.Cin = cin; a.Cout = o.cout; a.k = o.k; a.stride = o.stride;
        a.pad = o.k / 2; a.act = 1;
        if (o.cout2) {                       // Conv3x3 -> Conv1x1 fused: the 3x3's own output goes nowhere, the 1x1 writes d_y
            float *d_mid, *d_w2, *d_b2;
            HIPCHK(dm.alloc(&d_mid, o.npo * round_up(o.cout, 4) * 4));
            std::vector<float> pk2(packed_weight_floats(o.cout2, o.cout, 1)), bp2(round_up(o.cout2, 16), 0.f);
            pack_conv_weights(w2a, o.cout2, o.cout, 1, pk2.data());
            std::memcpy(bp2.data(), b2a, (size_t)o.cout2 * 4);
            HIPCHK(dm.alloc(&d_w2, pk2.size() * 4)); HIPCHK(hipMemcpy(d_w2, pk2.data(), pk2.size() * 4, hipMemcpyHostToDevice));
            HIPCHK(dm.alloc(&d_b2, bp2.size() * 4)); HIPCHK(hipMemcpy(d_b2, bp2.data(), bp2.size() * 4, hipMemcpyHostToDevice));
            a.dst = d_mid; a.dst_cs = round_up(o.cout, 4);
            a.f2_wpk = d_w2; a.f2_bias = d_b2; a.f2_dst = o.d_y; a.f2_dst_cs = o.cs_out; a.f2_cout = o.cout2; a.f2_act = 0;
        }
        std::vector<ConvLaunch> cands;
        KCHK(plan_conv_candidates(a, &cands));
        for (const ConvLaunch& l : cands) { const int kd = group_kind(l, o.k, o.stride); if (kd >= 0) { o.menu.push_back(l); o.kinds.push_back(kd); } }
    }
    if (n_menu_a) *n_menu_a = (int)c[0].menu.size();
    if (n_menu_b) *n_menu_b = (int)c[1].menu.size();
    if (c[0].menu.empty() || c[1].menu.empty()) return fail(MI355_EINVAL, "no candidate plan of one conv is on the group kernel's menu");
    const size_t ia = (size_t)(plan_a < 0 ? 0 : plan_a) % c[0].menu.size(), ib = (size_t)(plan_b < 0 ? 0 : plan_b) % c[1].menu.size();
    GroupLaunch g{};
    KCHK(plan_group({c[0].menu[ia], c[1].menu[ib]}, {c[0].kinds[ia], c[1].kinds[ib]}, &g));
    KCHK(run_group(g, nullptr));
    HIPCHK(hipDeviceSynchronize());
    for (One& o : c) {
        std::vector<float> yo(o.npo * o.cs_out);
        HIPCHK(hipMemcpy(yo.data(), o.d_y, yo.size() * 4, hipMemcpyDeviceToHost));
        const int c_final = o.cout2 ? o.cout2 : o.cout;
        for (size_t p = 0; p < o.npo; ++p) std::memcpy(o.y + p * c_final, &yo[p * o.cs_out], (size_t)c_final * 4);
    }
    return MI355_OK;
}

int mi355_op_conv2d_fused(int device_id, const float* x, int n, int h, int w, int cin, const float* w1_oihw, const float* b1, int c1,
                          int stride, const float* w2_oihw, const float* b2, int c2, int silu2, float* y, int plan_index, int* n_plans) {
    return op_conv2d_fused_impl(device_id, x, n, h, w, cin, w1_oihw, b1, c1, stride, w2_oihw, b2, c2, silu2, y, plan_index, n_plans, false, false);
}

int mi355_op_c2f_tail(int device_id, const float* x, int n, int h, int w, int cin, const float* w1_oihw, const float* b1, int c1,
                      const float* residual, const float* lead, int lead_c, const float* w2_oihw, const float* b2, int c2, float* y,
                      int plan_index, int* n_plans) {
    return op_conv2d_fused_impl(device_id, x, n, h, w, cin, w1_oihw, b1, c1, 1, w2_oihw, b2, c2, 1, y, plan_index, n_plans, false, false,
                                residual, lead, lead_c);
}

int mi355_op_conv2d_fused_f16(int device_id, const float* x, int n, int h, int w, int cin, const float* w1_oihw, const float* b1, int c1,
                              int stride, const float* w2_oihw, const float* b2, int c2, int silu2, float* y, int out_f32, int plan_index,
                              int* n_plans) {
    return op_conv2d_fused_impl(device_id, x, n, h, w, cin, w1_oihw, b1, c1, stride, w2_oihw, b2, c2, silu2, y, plan_index, n_plans, true,
                                out_f32 != 0);
}

static int bench_conv2d_impl(int device_id, int n, int h, int w, int cin, int cout, int k, int stride, int silu, int residual,
                             int plan_index, int iters, float* avg_ms, int* n_plans, char* plan_desc, int plan_desc_len, bool half) {
    if (!avg_ms || n <= 0 || h <= 0 || w <= 0 || cin <= 0 || cout <= 0 || iters <= 0) return fail(MI355_EINVAL, "bad argument");
    if (!((k == 1 && stride == 1) || (k == 3 && (stride == 1 || stride == 2)))) return fail(MI355_EINVAL, "k/stride not supported");
    HIPCHK(hipSetDevice(device_id));
    const int es = half ? 2 : 4;
    const int ho = h / stride, wo = w / stride, cs_in = round_up(cin, 16 / es), cs_out = round_up(cout, 16 / es);
    const size_t nin = (size_t)n * h * w * cs_in, nout = (size_t)n * ho * wo * cs_out;     // elements
    DevMem dm; float *d_x, *d_y, *d_r = nullptr, *d_w, *d_b, *d_z;
    HIPCHK(dm.alloc(&d_x, nin * es)); HIPCHK(dm.alloc(&d_y, nout * es)); HIPCHK(dm.alloc(&d_z, 256)); HIPCHK(hipMemset(d_z, 0, 256));
    {   // random activations / weights (benchmarks on zeros read high: DVFS)
        std::vector<float> hx(std::min<size_t>(nin, 1u << 22));
        std::vector<uint16_t> hh(half ? hx.size() : 0);
        unsigned st = 12345u;
        for (float& v : hx) { st = st * 1664525u + 1013904223u; v = ((st >> 8) & 0xffff) / 32768.0f - 1.0f; }
        if (half) floats_to_halfs(hx.data(), hh.data(), hx.size());
        const void* hsrc = half ? (const void*)hh.data() : (const void*)hx.data();
        for (size_t o = 0; o < nin; o += hx.size())
            HIPCHK(hipMemcpy((char*)d_x + o * es, hsrc, std::min(hx.size(), nin - o) * es, hipMemcpyHostToDevice));
        if (residual) { HIPCHK(dm.alloc(&d_r, nout * es)); HIPCHK(hipMemcpy(d_r, d_x, std::min(nin, nout) * es, hipMemcpyDeviceToDevice)); }
        std::vector<float> wt((size_t)cout * cin * k * k), bp(round_up(cout, 16), 0.1f);
        for (float& v : wt) { st = st * 1664525u + 1013904223u; v = (((st >> 8) & 0xffff) / 32768.0f - 1.0f) / std::sqrt((float)cin * k * k); }
        if (half) {
            std::vector<uint16_t> pk(packed_weight_halfs(cout, cin, k));
            pack_conv_weights_f16(wt.data(), cout, cin, k, pk.data());
            HIPCHK(dm.alloc(&d_w, pk.size() * 2));
            HIPCHK(hipMemcpy(d_w, pk.data(), pk.size() * 2, hipMemcpyHostToDevice));
        } else {
            std::vector<float> pk(packed_weight_floats(cout, cin, k));
            pack_conv_weights(wt.data(), cout, cin, k, pk.data());
            HIPCHK(dm.alloc(&d_w, pk.size() * 4));
            HIPCHK(hipMemcpy(d_w, pk.data(), pk.size() * 4, hipMemcpyHostToDevice));
        }
        HIPCHK(dm.alloc(&d_b, bp.size() * 4));
        HIPCHK(hipMemcpy(d_b, bp.data(), bp.size() * 4, hipMemcpyHostToDevice));
    }
    ConvArgs a{};
    a.src = d_x; a.src_cs = cs_in; a.dst = d_y; a.dst_cs = cs_out; a.res = d_r; a.res_cs = cs_out; a.wpk = d_w; a.bias = d_b; a.zeros = d_z;
    a.dtype = half ? 1 : 0;
    a.B = n; a.Hin = h; a.Win = w; a.Hout = ho; a.Wout = wo; a.Cin = cin; a.Cout = cout; a.k = k; a.stride = stride; a.pad = k / 2; a.act = silu ? 1 : 0;
    std::vector<ConvLaunch> cands;
    KCHK(plan_conv_candidates(a, &cands));
    if (n_plans) *n_plans = (int)cands.size();
    const ConvLaunch& l = cands[(size_t)(plan_index < 0 ? 0 : plan_index) % cands.size()];
    if (plan_desc && plan_desc_len > 0)
        snprintf(plan_desc, plan_desc_len, "v%d CT%d PT%d WP%d tile %dx%d ck%d lds %zu grid %ux%u", l.version, l.CT, l.PT, l.WP, l.a.TW, l.a.TH, l.a.ck,
                 l.lds, l.grid_x, l.grid_y);
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    for (int i = 0; i < 2; ++i) KCHK(run_conv(l, nullptr));
    HIPCHK(hipEventRecord(e0, nullptr));
    for (int i = 0; i < iters; ++i) KCHK(run_conv(l, nullptr));
    HIPCHK(hipEventRecord(e1, nullptr));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    *avg_ms = ms / iters;
    return MI355_OK;
}

int mi355_bench_conv2d(int device_id, int n, int h, int w, int cin, int cout, int k, int stride, int silu, int residual,
                       int plan_index, int iters, float* avg_ms, int* n_plans, char* plan_desc, int plan_desc_len) {
    return bench_conv2d_impl(device_id, n, h, w, cin, cout, k, stride, silu, residual, plan_index, iters, avg_ms, n_plans, plan_desc,
                             plan_desc_len, false);
}

int mi355_bench_conv2d_f16(int device_id, int n, int h, int w, int cin, int cout, int k, int stride, int silu, int residual,
                           int plan_index, int iters, float* avg_ms, int* n_plans, char* plan_desc, int plan_desc_len) {
    return bench_conv2d_impl(device_id, n, h, w, cin, cout, k, stride, silu, residual, plan_index, iters, avg_ms, n_plans, plan_desc,
                             plan_desc_len, true);
}

// Host-only view of the launch planner (no kernel is launched, no device memory is touched): which kernel versions would be
// offered for a conv of this shape and these buffer strides.  Used by the CPU tests of the planner's guards.
static int plan_query_impl(int n, int h, int w, int cin, int cout, int k, int stride, int src_cs, int dst_cs, int res_cs, int f2_cout, int f2_dst_cs,
                           int half, int* out, int cap, int* n_plans, bool tiles) {
    if (!n_plans || n <= 0 || h <= 0 || w <= 0 || cin <= 0 || cout <= 0 || cap < 0 || (cap > 0 && !out)) return fail(MI355_EINVAL, "bad argument");
    if (stride != 1 && stride != 2) return fail(MI355_EINVAL, "stride must be 1 or 2");
    float* fake = (float*)(uintptr_t)0x10000;                    // aligned, never dereferenced
    ConvArgs a{};
    a.src = fake; a.src_cs = src_cs; a.dst = fake; a.dst_cs = dst_cs; a.res = res_cs ? fake : nullptr; a.res_cs = res_cs;
    a.wpk = fake; a.bias = fake; a.zeros = fake;
    a.B = n; a.Hin = h; a.Win = w; a.Hout = h / stride; a.Wout = w / stride; a.Cin = cin; a.Cout = cout; a.k = k; a.stride = stride;
    a.pad = k / 2; a.act = 1; a.dtype = half ? 1 : 0;
    if (f2_cout > 0) { a.f2_wpk = fake; a.f2_bias = fake; a.f2_dst = fake; a.f2_dst_cs = f2_dst_cs; a.f2_cout = f2_cout; a.f2_act = 0; }
    std::vector<ConvLaunch> cands;
    if (const char* e = plan_conv_candidates(a, &cands)) { *n_plans = 0; return fail(MI355_EINVAL, e); }
    *n_plans = (int)cands.size();
    for (int i = 0; i < (int)cands.size() && i < cap; ++i) {
        const ConvLaunch& l = cands[i];
        const int version = l.version + (l.a.w2 ? 100 : 0);
        if (!tiles) { out[i] = version; continue; }
        const int f[MI355_PLAN_TILE_FIELDS] = {version, l.PT, l.CT, l.WP, l.a.TW, l.a.TH, l.a.cgroups, (int)l.grid_x, (int)l.grid_y};
        std::copy(f, f + MI355_PLAN_TILE_FIELDS, out + (size_t)i * MI355_PLAN_TILE_FIELDS);
    }
    return MI355_OK;
}

int mi355_plan_query(int n, int h, int w, int cin, int cout, int k, int stride, int src_cs, int dst_cs, int res_cs, int f2_cout,
                     int f2_dst_cs, int half, int* versions, int cap, int* n_plans) {
    return plan_query_impl(n, h, w, cin, cout, k, stride, src_cs, dst_cs, res_cs, f2_cout, f2_dst_cs, half, versions, cap, n_plans, false);
}

// ... and every candidate's wave tile, output tile and grid (which tile a conv of this shape can run with: tests, tools/plan_tiles.py)
int mi355_plan_query_tiles(int n, int h, int w, int cin, int cout, int k, int stride, int src_cs, int dst_cs, int res_cs, int f2_cout,
                           int f2_dst_cs, int half, int* tiles, int cap, int* n_plans) {
    return plan_query_impl(n, h, w, cin, cout, k, stride, src_cs, dst_cs, res_cs, f2_cout, f2_dst_cs, half, tiles, cap, n_plans, true);
}

static int op_stem_impl(int device_id, const uint8_t* bgr, int n, int h, int w, const float* w_oihw, const float* bias, int cout,
                        int k, int stride, bool half, int variant, void* y) {
    if (!bgr || !w_oihw || !bias || !y || n <= 0 || h <= 0 || w <= 0 || cout <= 0) return fail(MI355_EINVAL, "bad argument");
    if ((k != 3 && k != 6) || (h % stride) || (w % stride)) return fail(MI355_EINVAL, "k/stride not supported");
    HIPCHK(hipSetDevice(device_id));
    const int ho = h / stride, wo = w / stride, cs = round_up(cout, 4);
    const size_t es = half ? 2 : 4;
    DevMem dm; uint8_t* d_img; float *d_y, *d_w, *d_b, *d_l;
    const size_t ib = (size_t)n * h * w * 3, yn = (size_t)n * ho * wo * cs;
    float lut[256];
    for (int i = 0; i < 256; ++i) lut[i] = (float)i / 255.0f;
    HIPCHK(dm.alloc(&d_img, ib)); HIPCHK(dm.alloc(&d_y, yn * es)); HIPCHK(dm.alloc(&d_w, (size_t)cout * 3 * k * k * 4));
    const int bn = round_up(cout, 16);                               // the engine's bias arrays are padded the same way
    HIPCHK(dm.alloc(&d_b, (size_t)bn * 4)); HIPCHK(dm.alloc(&d_l, sizeof(lut)));
    HIPCHK(hipMemcpy(d_img, bgr, ib, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_w, w_oihw, (size_t)cout * 3 * k * k * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(d_b, 0, (size_t)bn * 4));
    HIPCHK(hipMemcpy(d_b, bias, (size_t)cout * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_l, lut, sizeof(lut), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(d_y, 0, yn * es));
    StemArgs s{};
    if (half && k == 3) {
        std::vector<uint16_t> fr;
        stem3_weight_frags(w_oihw, cout, fr);
        uint16_t* d_f;
        HIPCHK(dm.alloc(&d_f, fr.size() * 2));
        HIPCHK(hipMemcpy(d_f, fr.data(), fr.size() * 2, hipMemcpyHostToDevice));
        s.wfrag = d_f;
    } else if (k == 3) {
        std::vector<float> fr;
        stem3_weight_frags_f32(w_oihw, cout, fr);
        float* d_f;
        HIPCHK(dm.alloc(&d_f, fr.size() * 4));
        HIPCHK(hipMemcpy(d_f, fr.data(), fr.size() * 4, hipMemcpyHostToDevice));
        s.wfrag = d_f;
    }
    s.img = d_img; s.dst = d_y; s.dst_cs = cs; s.w = d_w; s.bias = d_b; s.lut = d_l;
    s.B = n; s.H = h; s.W = w; s.Hout = ho; s.Wout = wo; s.Cout = cout; s.k = k; s.stride = stride; s.pad = (k == 6 ? 2 : k / 2);
    s.out_half = half ? 1 : 0; s.variant = variant;
    KCHK(launch_stem(s, nullptr));
    HIPCHK(hipDeviceSynchronize());
    std::vector<uint8_t> yo(yn * es);
    HIPCHK(hipMemcpy(yo.data(), d_y, yn * es, hipMemcpyDeviceToHost));
    for (size_t p = 0; p < (size_t)n * ho * wo; ++p) std::memcpy((uint8_t*)y + p * cout * es, &yo[p * cs * es], (size_t)cout * es);
    return MI355_OK;
}

int mi355_op_stem(int device_id, const uint8_t* bgr, int n, int h, int w, const float* w_oihw, const float* bias, int cout,
                  int k, int stride, float* y) {
    return op_stem_impl(device_id, bgr, n, h, w, w_oihw, bias, cout, k, stride, false, 0, y);
}

int mi355_op_stem_f16(int device_id, const uint8_t* bgr, int n, int h, int w, const float* w_oihw, const float* bias, int cout,
                      int k, int stride, int variant, uint16_t* y) {
    if (variant < 0 || (variant & 255) > 2 || (variant >> 8) > 31) return fail(MI355_EINVAL, "variant must be 0 (the launcher's choice), 1 (general) or 2 (k3 s2)");
    if ((variant & 255) == 2 && (k != 3 || stride != 2 || (w & 3))) return fail(MI355_EINVAL, "variant 2 is the k 3, stride 2 kernel for widths that are multiples of 4");
    return op_stem_impl(device_id, bgr, n, h, w, w_oihw, bias, cout, k, stride, true, variant, y);
}

int mi355_op_nms(int device_id, const float* pred, int n, int nc, int extra, int anchors, float conf, float iou,
                 const int* classes, int n_classes, int max_det, mi355_det* out_rows, int cap, int* out_counts) {
    if (!pred || !out_rows || !out_counts || n <= 0 || nc <= 0 || extra < 0 || anchors <= 0 || cap < 1) return fail(MI355_EINVAL, "bad argument");
    if (max_det <= 0) max_det = 300;
    if (max_det > 1024) return fail(MI355_EINVAL, "max_det must be <= 1024");
    if (extra > MI355_MAX_KPT_FLOATS) return fail(MI355_EINVAL, "too many extra columns");
    HIPCHK(hipSetDevice(device_id));
    const int no = 4 + nc + extra;
    int ap2 = 1; while (ap2 < anchors) ap2 <<= 1;
    DevMem dm; float *d_in, *d_am; float2* d_best; unsigned long long* d_keys; mi355_det* d_rows; int* d_counts; unsigned* d_mask = nullptr;
    const size_t pn = (size_t)n * no * anchors;
    HIPCHK(dm.alloc(&d_in, pn * 4)); HIPCHK(dm.alloc(&d_am, pn * 4)); HIPCHK(dm.alloc(&d_best, (size_t)n * anchors * sizeof(float2)));
    HIPCHK(dm.alloc(&d_keys, (size_t)n * ap2 * 8)); HIPCHK(dm.alloc(&d_rows, (size_t)n * max_det * sizeof(mi355_det)));
    HIPCHK(dm.alloc(&d_counts, (size_t)3 * n * sizeof(int)));
    HIPCHK(hipMemcpy(d_in, pred, pn * 4, hipMemcpyHostToDevice));
    if (n_classes > 0 && classes) {
        std::vector<unsigned> m((nc + 31) / 32, 0u);
        for (int i = 0; i < n_classes; ++i) if (classes[i] >= 0 && classes[i] < nc) m[classes[i] >> 5] |= 1u << (classes[i] & 31);
        HIPCHK(dm.alloc(&d_mask, m.size() * 4));
        HIPCHK(hipMemcpy(d_mask, m.data(), m.size() * 4, hipMemcpyHostToDevice));
    }
    KCHK(launch_transpose_pred(d_in, d_am, n, no, anchors, nullptr));      // [n][no][A] -> [n][A][no]
    KCHK(launch_best_from_pred(d_am, n, anchors, no, nc, d_best, nullptr));
    NmsArgs na{};
    na.pred = d_am; na.best = d_best; na.B = n; na.A = anchors; na.no = no; na.nc = nc; na.nk = extra; na.kdim = 0;
    na.conf = conf; na.iou = iou; na.max_det = max_det; na.max_nms = 30000; na.max_wh = 7680.f;
    na.class_mask = d_mask; na.keys = d_keys; na.Apow2 = ap2; na.scale_back = 0; na.gain = 1.f;
    na.out_rows = d_rows; na.out_counts = d_counts;
    KCHK(launch_nms(na, nullptr));
    HIPCHK(hipDeviceSynchronize());
    std::vector<mi355_det> rows((size_t)n * max_det);
    std::vector<int> counts(n);
    HIPCHK(hipMemcpy(rows.data(), d_rows, rows.size() * sizeof(mi355_det), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(counts.data(), d_counts, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) {
        const int c = std::min(counts[i], cap);
        out_counts[i] = c;
        std::memcpy(out_rows + (size_t)i * cap, rows.data() + (size_t)i * max_det, (size_t)c * sizeof(mi355_det));
    }
    return MI355_OK;
}

// launch_nms (+ launch_compact_rows) as a pass enqueues them, with every argument the engine sets open to the caller.  Nothing is
// chosen here: launch_nms picks the fused / two-launch / multi-launch path from n and anchors as it does for the engine.
int mi355_op_nms_ex(int device_id, const float* pred, const float* best, int n, int nc, int extra, int anchors, float conf, float iou,
                    const int* classes, int n_classes, int max_det, int max_nms, int kdim, const float* geom, int geom_mode, int pack,
                    uint32_t* rows, int* counts, uint32_t* packed, int* offsets) {
    if (!pred || !rows || !counts || n <= 0 || nc <= 0 || extra < 0 || anchors <= 0) return fail(MI355_EINVAL, "bad argument");
    if (max_det < 1 || max_det > 1024) return fail(MI355_EINVAL, "max_det must lie in 1 .. 1024");
    if (max_nms < 1) return fail(MI355_EINVAL, "max_nms must be at least 1");
    if (extra > MI355_MAX_KPT_FLOATS) return fail(MI355_EINVAL, "too many extra columns");
    if (kdim != 0 && kdim != 2 && kdim != 3) return fail(MI355_EINVAL, "kdim must be 0, 2 or 3");
    if (kdim && (extra == 0 || extra % kdim)) return fail(MI355_EINVAL, "kdim must divide the extra columns (and needs some)");
    if (!(conf >= 0.f)) return fail(MI355_EINVAL, "conf must be >= 0 (the sort key orders positive scores only)");
    if (geom_mode < 0 || geom_mode > 2 || (geom_mode != 0) != (geom != nullptr))
        return fail(MI355_EINVAL, "geom_mode: 0 without geom, 1 = seven scalars, 2 = [n][7]");
    if (pack && (!packed || !offsets)) return fail(MI355_EINVAL, "pack needs the packed and offsets outputs");
    if (n_classes < 0 || (n_classes > 0 && !classes)) return fail(MI355_EINVAL, "bad class list");
    const int no = 4 + nc + extra;
    if ((long)anchors * n * no > (1l << 28) || n > (1 << 20)) return fail(MI355_EINVAL, "too many anchors");
    std::vector<unsigned> mask;
    if (n_classes > 0) {
        mask.assign((nc + 31) / 32, 0u);
        for (int i = 0; i < n_classes; ++i) if (classes[i] >= 0 && classes[i] < nc) mask[classes[i] >> 5] |= 1u << (classes[i] & 31);
        // the candidate filter indexes the mask with best[]'s class: it must name a class
        if (best)
            for (long i = 0; i < (long)anchors * n; ++i)
                if (!(best[2 * i + 1] >= 0.f && best[2 * i + 1] < (float)nc)) return fail(MI355_EINVAL, "best[] holds a class outside 0 .. nc-1");
    }
    HIPCHK(hipSetDevice(device_id));
    int ap2 = 1; while (ap2 < anchors) ap2 <<= 1;
    const int RW = (int)(sizeof(mi355_det) / 4);
    DevMem dm; float *d_in, *d_am, *d_geom = nullptr; float2* d_best; unsigned long long* d_keys; uint32_t *d_rows, *d_packed = nullptr;
    int *d_counts, *d_offsets = nullptr; unsigned* d_mask = nullptr;
    const size_t pn = (size_t)n * no * anchors, rw = (size_t)n * max_det * RW;
    HIPCHK(dm.alloc(&d_in, pn * 4)); HIPCHK(dm.alloc(&d_am, pn * 4)); HIPCHK(dm.alloc(&d_best, (size_t)n * anchors * sizeof(float2)));
    HIPCHK(dm.alloc(&d_keys, (size_t)n * ap2 * 8)); HIPCHK(dm.alloc(&d_rows, rw * 4));
    HIPCHK(dm.alloc(&d_counts, (size_t)3 * n * sizeof(int)));
    HIPCHK(hipMemcpy(d_in, pred, pn * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_rows, rows, rw * 4, hipMemcpyHostToDevice));       // whatever the caller filled them with stays where nothing is written
    HIPCHK(hipMemset(d_counts, 0xFF, (size_t)3 * n * sizeof(int)));
    if (pack) {
        HIPCHK(dm.alloc(&d_packed, rw * 4)); HIPCHK(hipMemcpy(d_packed, packed, rw * 4, hipMemcpyHostToDevice));
        HIPCHK(dm.alloc(&d_offsets, (size_t)(n + 1) * sizeof(int)));
        HIPCHK(hipMemcpy(d_offsets, offsets, (size_t)(n + 1) * sizeof(int), hipMemcpyHostToDevice));
    }
    if (!mask.empty()) { HIPCHK(dm.alloc(&d_mask, mask.size() * 4)); HIPCHK(hipMemcpy(d_mask, mask.data(), mask.size() * 4, hipMemcpyHostToDevice)); }
    if (geom_mode == 2) { HIPCHK(dm.alloc(&d_geom, (size_t)n * 7 * 4)); HIPCHK(hipMemcpy(d_geom, geom, (size_t)n * 7 * 4, hipMemcpyHostToDevice)); }
    KCHK(launch_transpose_pred(d_in, d_am, n, no, anchors, nullptr));      // [n][no][A] -> [n][A][no]
    if (best) HIPCHK(hipMemcpy(d_best, best, (size_t)n * anchors * sizeof(float2), hipMemcpyHostToDevice));
    else KCHK(launch_best_from_pred(d_am, n, anchors, no, nc, d_best, nullptr));
    NmsArgs na{};
    na.pred = d_am; na.best = d_best; na.B = n; na.A = anchors; na.no = no; na.nc = nc; na.nk = extra; na.kdim = kdim;
    na.conf = conf; na.iou = iou; na.max_det = max_det; na.max_nms = max_nms; na.max_wh = 7680.f;
    na.class_mask = d_mask; na.keys = d_keys; na.Apow2 = ap2; na.scale_back = geom_mode ? 1 : 0; na.gain = 1.f;
    if (geom_mode == 1) {
        na.gain = geom[0]; na.pad_x = geom[1]; na.pad_y = geom[2]; na.kpad_x = geom[3]; na.kpad_y = geom[4]; na.orig_w = geom[5]; na.orig_h = geom[6];
    }
    na.frame_geom = d_geom;
    na.out_rows = d_rows; na.out_counts = d_counts;
    KCHK(launch_nms(na, nullptr));
    if (pack) KCHK(launch_compact_rows(d_rows, d_counts, n, max_det, RW, d_offsets, d_packed, nullptr));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(rows, d_rows, rw * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(counts, d_counts, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    if (pack) {
        HIPCHK(hipMemcpy(packed, d_packed, rw * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(offsets, d_offsets, (size_t)(n + 1) * sizeof(int), hipMemcpyDeviceToHost));
    }
    return MI355_OK;
}

// the transform stage of the JPEG encoder alone (jpeg_kernels.hip): quantised coefficients in zigzag order, on the GPU or by the host twin
int mi355_op_jpeg_coefficients(int device, const mi355_render_frame* frames, int n, int quality, int subsampling, int16_t* const* coefs) {
    if (!coefs) return fail(MI355_EINVAL, "jpeg: null output");
    JpegCtx ctx;
    const int rc = jpeg_run(ctx, device, frames, n, quality, subsampling, nullptr, coefs, nullptr, nullptr);
    if (device >= 0) jpeg_ctx_free(ctx);
    return rc;
}

}  // extern "C"
