// One pass of the net (launch_net), one chunk (run_chunk) and one infer call (infer_impl): letterbox -> stem -> conv program ->
// decode -> NMS -> rows.  Replaces BasePredictor.stream_inference behind /root/reference/model.py:38.
#include "engine_internal.h"

namespace mi355 {

// ---- sparse box branch: which ops form the box chain of every head level (program structure, decided at load time) ----
void detect_sparse_head(mi355_yolo* h) {
    h->sp_levels = 0;
    h->sp_skip.assign(h->ops.size(), 0); h->sp_late.assign(h->bufs.size(), 0);
    if (h->half || (h->opt_flags & MI355_OPT_NO_SPARSE_BOX) || h->levels.empty() || h->levels.size() > 3 || h->hdr.reg_max != 16) return;
    const int n = (int)h->ops.size();
    auto conv_op = [&](int i, int k) { const FileOp& o = h->ops[i]; return o.type == OP_CONV && (int)h->convs[o.conv].k == k && h->convs[o.conv].s == 1 && o.res_buf < 0; };
    int m[3], b1[3], b2[3];
    for (size_t l = 0; l < h->levels.size(); ++l) {
        const FileLevel& lv = h->levels[l];
        m[l] = b1[l] = b2[l] = -1;
        for (int i = 0; i < n; ++i)
            if (conv_op(i, 1) && h->ops[i].dst_buf == (int)lv.buf && h->ops[i].dst_choff == (int)lv.box_off && h->ops[i].dst_c == 64 && h->ops[i].src_c == 64 && h->ops[i].act == 0) b2[l] = i;
        if (b2[l] < 0) return;
        const FileOp& o2 = h->ops[b2[l]];
        for (int i = 0; i < n; ++i)
            if (conv_op(i, 3) && h->ops[i].dst_buf == o2.src_buf && h->ops[i].dst_choff == o2.src_choff && h->ops[i].dst_c == 64 && h->ops[i].src_c == 64 && h->convs[h->ops[i].conv].pad == 1) b1[l] = i;
        if (b1[l] < 0) return;
        const FileOp& o1 = h->ops[b1[l]];
        for (int i = 0; i < n; ++i)
            if (conv_op(i, 3) && h->ops[i].dst_buf == o1.src_buf && h->ops[i].dst_choff == o1.src_choff && h->ops[i].dst_c >= 64 &&
                (h->ops[i].src_c % 16) == 0 && h->convs[h->ops[i].conv].pad == 1 && h->ops[i].act == o1.act) m[l] = i;
        if (m[l] < 0) return;
        // nobody but cv2.i.1 reads the box slice of cv2.i.0's output, nobody but cv2.i.2 reads cv2.i.1's
        for (int j = 0; j < n; ++j) {
            const FileOp& o = h->ops[j];
            if (o.type == OP_STEM) continue;
            auto touches = [&](int buf, int off, int c) { return (o.src_buf == buf && o.src_choff < off + c && off < o.src_choff + o.src_c) ||
                                                                 (o.res_buf == buf && o.res_choff < off + c && off < o.res_choff + o.dst_c); };
            if (j != b1[l] && touches(o1.src_buf, o1.src_choff, 64)) return;
            if (j != b2[l] && touches(o2.src_buf, o2.src_choff, 64)) return;
        }
    }
    h->sp_levels = (int)h->levels.size();
    for (int l = 0; l < h->sp_levels; ++l) {
        h->sp_m[l] = m[l]; h->sp_b1[l] = b1[l]; h->sp_b2[l] = b2[l];
        h->sp_skip[b1[l]] = h->sp_skip[b2[l]] = 1;
        if (h->ops[m[l]].dst_c == 64) h->sp_skip[m[l]] = 1;          // an unmerged cv2.i.0 is box work as a whole
        h->sp_late[h->ops[m[l]].src_buf] = 1; h->sp_late[h->ops[m[l]].dst_buf] = 1;
    }
}

// ---- object features: the op that reads each level's Detect input.  From the level's box-logit writer (cv2.i.2: the pointwise conv
// that fills the 4 * reg_max channels at box_off) back through cv2.i.1 (the 3x3 conv that writes exactly its input slice) to cv2.i.0
// (the 3x3 conv whose output slice BEGINS with cv2.i.1's input: alone, or merged with cv3.i.0 / cv4.i.0 behind it).  Program
// structure only: which of these run fused or grouped does not matter.  That op's source slice is the map Ultralytics' pre-hook sees.
void detect_feature_sources(mi355_yolo* h) {
    h->feat_levels = 0; h->feat_dim = 0;
    if (h->levels.empty() || h->levels.size() > 4) return;
    const int n = (int)h->ops.size(), box_c = 4 * (int)h->hdr.reg_max;
    auto conv_op = [&](int i, int k) { const FileOp& o = h->ops[i]; return o.type == OP_CONV && (int)h->convs[o.conv].k == k && h->convs[o.conv].s == 1 && o.res_buf < 0; };
    int src[4], dim = 1 << 30;
    for (size_t l = 0; l < h->levels.size(); ++l) {
        const FileLevel& lv = h->levels[l];
        int b2 = -1, b1 = -1, m = -1;
        for (int i = 0; i < n; ++i)
            if (conv_op(i, 1) && h->ops[i].dst_buf == (int)lv.buf && h->ops[i].dst_choff == (int)lv.box_off && h->ops[i].dst_c == box_c) b2 = i;
        if (b2 < 0) return;
        const FileOp& o2 = h->ops[b2];
        for (int i = 0; i < n; ++i)
            if (conv_op(i, 3) && h->ops[i].dst_buf == o2.src_buf && h->ops[i].dst_choff == o2.src_choff && h->ops[i].dst_c == o2.src_c) b1 = i;
        if (b1 < 0) return;
        const FileOp& o1 = h->ops[b1];
        for (int i = 0; i < n; ++i)
            if (conv_op(i, 3) && h->ops[i].dst_buf == o1.src_buf && h->ops[i].dst_choff == o1.src_choff && h->ops[i].dst_c >= o1.src_c) m = i;
        if (m < 0) return;
        src[l] = m;
        dim = std::min(dim, h->ops[m].src_c);
    }
    for (size_t l = 0; l < h->levels.size(); ++l) if (dim < 1 || h->ops[src[l]].src_c % dim) return;
    h->feat_levels = (int)h->levels.size(); h->feat_dim = dim;
    for (int l = 0; l < h->feat_levels; ++l) h->feat_src[l] = src[l];
}

bool sparse_wanted(const mi355_yolo* h, int nb) {
    if (h->sp_levels <= 0 || h->half || h->use_graph) return false;
    if (const char* e = getenv("MI355_SPARSE_BOX")) return atoi(e) != 0;
    return nb >= h->sparse_min_batch;
}

// a planned 3x3 launch over the cout tiles [t0, t0 + nt) of its conv: offsets into the packed weights, the bias and the
// destination slice, and a grid over fewer cout groups -- the op program, the weight file and the plan files stay as they are
ConvLaunch cout_subrange(const ConvLaunch& l0, int t0, int nt) {
    ConvLaunch l = l0;
    l.a.wpk += (size_t)t0 * 9 * l.a.cib * 256; l.a.bias += t0 * 16; l.a.dst += t0 * 16;
    l.a.Cout = std::min(nt * 16, l0.a.Cout - t0 * 16); l.a.n_ctiles = nt;
    const int per = l.CT * (l.version == 6 ? 1 : 4 / l.WP);
    l.a.cgroups = std::max(1, std::min(l0.a.cgroups, (nt + per - 1) / per));
    l.grid_y = (unsigned)((nt + per * l.a.cgroups - 1) / (per * l.a.cgroups));
    l.a.fd_gy = make_fastdiv(std::max(1u, l.grid_y));
    l.flops = l0.flops * nt / std::max(1, l0.a.n_ctiles);
    return l;
}

// capacity of a level's position lists over `pos` positions: the sparse_cap share of them, at least 64, never more than there are
static int sparse_list_cap(const mi355_yolo* h, long long pos) {
    return (int)std::min<long long>(pos, std::max<long long>(64, (long long)std::ceil((double)h->sparse_cap * (double)pos)));
}

// A position enters each list at most once per pass, so a list that holds every position of the chunk cannot overflow: the gated dense
// fall-back is then not enqueued at all (launch_sparse_tail), and is not counted among the pass's launches (ensure_shape).
bool sparse_lists_can_overflow(const mi355_yolo* h, int nb) {
    for (int l = 0; l < h->sp_levels; ++l) {
        const long long pos = (long long)nb * (h->cur_H / h->levels[l].stride) * (h->cur_W / h->levels[l].stride);
        if (std::min(h->sp_cap[l], sparse_list_cap(h, pos)) < pos) return true;      // (a tail chunk uses the head of the full chunk's lists)
    }
    return false;
}

int prepare_sparse_shape(mi355_yolo* h, int nb, int Hl, int Wl) {
    h->sparse_shape = false;
    // sparse_why (plan_info): 0 runs, 1 the program has no such head / half / switched off, 2 below the frames-per-pass threshold
    // (or MI355_SPARSE_BOX=0, hipGraph), 3 the shape's tuned plan of cv2.i.1 is not the fused 3x3 + 1x1 launch, 4 the plan of
    // cv2.i.0 is not one of the gated 3x3 kernels (v1 / v6)
    h->sparse_why = h->sp_levels <= 0 || h->half ? 1 : 2;
    if (!sparse_wanted(h, nb)) return MI355_OK;
    for (int l = 0; l < h->sp_levels; ++l) {
        const int m = h->sp_m[l], b1 = h->sp_b1[l], b2 = h->sp_b2[l];
        const ConvLaunch& pm = h->plans[m]; const ConvLaunch& p1 = h->plans[b1];
        // the dense fall-back must be launches of the gated kernels: cv2.i.1 with cv2.i.2 fused behind it, plain 3x3 kernels
        if (h->fuse2[b1] != b2 || !h->skip_op[b2] || !p1.a.w2 || p1.version != 1) { h->sparse_why = 3; return MI355_OK; }
        if ((pm.version != 1 && pm.version != 6) || pm.a.w2 || pm.a.res || h->skip_op[m]) { h->sparse_why = 4; return MI355_OK; }
    }
    if (!h->sp_state) {
        HIPCHK(hipMalloc(&h->sp_state, 16 * sizeof(int)));
        HIPCHK(hipMemset(h->sp_state, 0, 16 * sizeof(int)));
    }
    size_t ints = 0;
    for (int l = 0; l < h->sp_levels; ++l) {
        const FileLevel& lv = h->levels[l];
        h->sp_cap[l] = sparse_list_cap(h, (long long)nb * (Hl / lv.stride) * (Wl / lv.stride));
        h->sp_off_dil[l] = ints; ints += (size_t)h->sp_cap[l];
        h->sp_off_cand[l] = ints; ints += (size_t)h->sp_cap[l];
    }
    GROW(h->sp_lists, ints * sizeof(int));
    for (int l = 0; l < h->sp_levels; ++l) {
        const int m = h->sp_m[l];
        const int nt = h->plans[m].a.n_ctiles;
        if (nt > 4) { h->sp_cls[l] = cout_subrange(h->plans[m], 4, nt - 4); h->sp_box[l] = cout_subrange(h->plans[m], 0, 4); }
        else h->sp_box[l] = h->plans[m];
        h->sp_box[l].a.gate = h->sp_state + 8;
        h->sp_b1l[l] = h->plans[h->sp_b1[l]];
        h->sp_b1l[l].a.gate = h->sp_state + 8;
    }
    h->sparse_shape = true; h->sparse_why = 0;
    return MI355_OK;
}

// run the net (+decode) on nb frames that sit in `frames_dev` (original size h0 x w0, dense).
// Launch-bound regime: the stem..decode sequence (60-100 launches) is captured once per chunk size into a hipGraph
// and replayed; the frames are first copied into the engine's own staging buffer so the captured pointers stay valid.
int run_chunk(mi355_yolo* h, Prof& pf, const uint8_t* frames_dev, int nb, const Geometry& g, bool full_pred) {
    const uint8_t* stem_in = frames_dev;
    const bool graph = h->use_graph && !h->profiling && !full_pred;
    if (g.identity && graph) {
        HIPCHK(hipMemcpyAsync(h->lbox, frames_dev, (size_t)nb * g.Hl * g.Wl * 3, hipMemcpyDeviceToDevice, h->stream));
        stem_in = h->lbox;
    }
    if (!g.identity) {
        LetterboxArgs la{};
        la.src = frames_dev; la.H = g.h0; la.W = g.w0; la.frame_stride = (long long)g.h0 * g.w0 * 3; la.row_stride = g.w0 * 3;
        la.dst = h->lbox; la.Hd = g.Hl; la.Wd = g.Wl; la.top = g.top; la.left = g.left; la.Hr = g.Hr; la.Wr = g.Wr;
        la.xtab = (const int*)h->d_xtab.p; la.ytab = (const int*)h->d_ytab.p; la.resize = g.resize ? 1 : 0; la.B = nb;
        TIMED(pf, K_LETTERBOX, launch_letterbox(la, h->stream));
        stem_in = h->lbox;
    }
    if (!graph) return launch_net(h, pf, stem_in, nb, g, full_pred);
    hipGraphExec_t exec = nullptr;
    for (auto& ge : h->graphs) if (ge.first == nb) exec = ge.second;
    if (!exec) {
        hipGraph_t gr = nullptr;
        HIPCHK(hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
        const int rc = launch_net(h, pf, stem_in, nb, g, full_pred);
        const hipError_t e = hipStreamEndCapture(h->stream, &gr);
        if (rc) { if (gr) (void)hipGraphDestroy(gr); return rc; }
        if (e != hipSuccess) return fail(MI355_EHIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
        const hipError_t ei = hipGraphInstantiate(&exec, gr, nullptr, nullptr, 0);
        (void)hipGraphDestroy(gr);
        if (ei != hipSuccess) return fail(MI355_EHIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(ei));
        h->graphs.push_back({nb, exec});
    }
    HIPCHK(hipGraphLaunch(exec, h->stream));
    return MI355_OK;
}

// A launch planned for cur_nb frames, for a tail chunk of nb frames: same buffers, fewer pixels (pointwise forms: px = pixels of one
// frame of the conv's input map) or fewer tiles (3x3 forms).
static ConvLaunch fit_frames(const mi355_yolo* h, const ConvLaunch& planned, int k, int nb, int px) {
    ConvLaunch l = planned;
    if (nb == h->cur_nb) return l;
    if (k == 1 && l.version == 3) {
        l.a.Win = l.a.Wout = nb * px;
        const int per_block = 4 * 16 * (int)((size_t)l.a.TW / 64);       // TW = PT * 64 pixels per block
        l.grid_x = (unsigned)((l.a.Wout + per_block - 1) / per_block);
        return l;
    }
    if (k == 1) {
        l.a.Win = l.a.Wout = nb * px;
        l.a.tiles_x = (l.a.Wout + l.a.TW - 1) / l.a.TW;
        l.a.n_tiles_total = l.a.tiles_x;
    } else {
        l.a.n_tiles_total = (int)((long)nb * l.a.tiles_x * l.a.tiles_y);
    }
    // v1 / v6: one block per tile; v4 (persistent): keep the planned grid unless fewer tiles exist
    // v7 / v10 (persistent over (tile, cout group) units): likewise
    l.grid_x = l.version == 4 ? std::min(l.grid_x, (unsigned)l.a.n_tiles_total)
             : (l.version == 7 || l.version == 10) ? std::min(l.grid_x, (unsigned)l.a.n_tiles_total * (unsigned)l.a.cgroups) : (unsigned)l.a.n_tiles_total;
    return l;
}

// one pass: what every op launch of it needs
struct Pass {
    mi355_yolo* h; Prof& pf; const uint8_t* stem_in; int nb; const Geometry& g;
    bool sparse;        // the box chain's ops are not launched (cv2.i.0 merged with its siblings runs without its box couts)
};

// op i of the program on stream st: pick the launch, fit it to nb frames, run it timed
static int launch_op(const Pass& p, size_t i, hipStream_t st) {
    mi355_yolo* h = p.h; Prof& pf = p.pf; const Geometry& g = p.g; const int nb = p.nb;
    const FileOp& o = h->ops[i];
    if (p.sparse && h->sp_skip[i]) return MI355_OK;
    const int sd_out = h->bufs[o.dst_buf].stride_div;
    float* dst = h->view(o.dst_buf, o.dst_choff);
    if (o.type == OP_STEM) {
        const FileConv& c = h->convs[o.conv];
        StemArgs s{};
        s.img = p.stem_in; s.dst = dst; s.dst_cs = h->dbuf_cs[o.dst_buf];
        s.w = h->dconv[o.conv].w_raw; s.bias = h->dconv[o.conv].bias; s.lut = h->lut; s.wfrag = h->dconv[o.conv].w_frag;
        s.B = nb; s.H = g.Hl; s.W = g.Wl; s.Hout = g.Hl / sd_out; s.Wout = g.Wl / sd_out;
        s.Cout = c.cout; s.k = c.k; s.stride = c.s; s.pad = c.pad;
        s.out_half = h->dbuf_es[o.dst_buf] == 2; s.fast_act = h->fast_act ? 1 : 0;
        TIMED(pf, K_STEM, launch_stem(s, st));
    } else if (o.type == OP_CONV) {
        if (h->skip_op[i]) return MI355_OK;         // a pointwise conv that runs inside its producer's launch
        int spl = -1;
        for (int l = 0; p.sparse && l < h->sp_levels; ++l) if (h->sp_m[l] == (int)i) spl = l;
        const int sd_in = h->bufs[o.src_buf].stride_div;
        const ConvLaunch l = fit_frames(h, spl >= 0 ? h->sp_cls[spl] : h->plans[i], (int)h->convs[o.conv].k, nb, (g.Hl / sd_in) * (g.Wl / sd_in));
        TIMED(pf, K_CONV, run_conv(l, st));
    } else if (o.type == OP_UPSAMPLE) {
        if (h->fused_away[i]) return MI355_OK;      // read by its only consumer straight from the half-size map
        const int sd_in = h->bufs[o.src_buf].stride_div;
        if (h->dbuf_es[o.src_buf] != h->dbuf_es[o.dst_buf]) return fail(MI355_EFORMAT, "upsample between buffers of different precision");
        // fp16 buffers: a pure copy, so two halfs travel as one float (channel counts / offsets are multiples of 8)
        const int dv = h->dbuf_es[o.src_buf] == 2 ? 2 : 1;
        if (o.src_c % dv) return fail(MI355_EFORMAT, "half: odd channel count in upsample");
        TIMED(pf, K_UPSAMPLE, launch_upsample2x(h->view(o.src_buf, o.src_choff), h->dbuf_cs[o.src_buf] / dv, dst, h->dbuf_cs[o.dst_buf] / dv, nb,
                                                g.Hl / sd_in, g.Wl / sd_in, o.src_c / dv, st));
    } else if (o.type == OP_SPPF_POOL) {
        if (o.k != 5) return fail(MI355_EFORMAT, "SPPF pool size must be 5");
        if (h->dbuf_es[o.src_buf] == 2)
            TIMED(pf, K_POOL, launch_sppf_pools_f16(h->view(o.src_buf, o.src_choff), h->dbuf_cs[o.src_buf], dst, h->dbuf_cs[o.dst_buf], nb,
                                                    g.Hl / sd_out, g.Wl / sd_out, o.src_c, st));
        else
            TIMED(pf, K_POOL, launch_sppf_pools(h->view(o.src_buf, o.src_choff), h->dbuf_cs[o.src_buf], dst, h->dbuf_cs[o.dst_buf], nb,
                                                g.Hl / sd_out, g.Wl / sd_out, o.src_c, st));
    } else if (o.type == OP_DWCONV) {
        const FileConv& c = h->convs[o.conv];
        DwConvArgs a{};
        a.src = h->view(o.src_buf, o.src_choff); a.src_cs = h->dbuf_cs[o.src_buf];
        a.dst = dst; a.dst_cs = h->dbuf_cs[o.dst_buf];
        if (o.res_buf >= 0) { a.res = h->view(o.res_buf, o.res_choff); a.res_cs = h->dbuf_cs[o.res_buf]; }
        a.w = h->dconv[o.conv].w_raw; a.bias = h->dconv[o.conv].bias;
        a.B = nb; a.H = g.Hl / sd_out; a.W = g.Wl / sd_out; a.C = o.dst_c; a.k = c.k; a.act = o.act; a.c_pad = round_up(o.dst_c, 4);
        TIMED(pf, K_CONV, launch_dwconv(a, st));
    } else if (o.type == OP_ATTN) {
        PsaAttnArgs a{};
        a.qkv = h->view(o.src_buf, o.src_choff); a.qkv_cs = h->dbuf_cs[o.src_buf];
        a.dst = dst; a.dst_cs = h->dbuf_cs[o.dst_buf];
        a.B = nb; a.N = (g.Hl / sd_out) * (g.Wl / sd_out); a.heads = o.r0; a.key_dim = o.k; a.head_dim = o.s;
        a.scale = (float)(1.0 / std::sqrt((double)o.k));      // Attention.scale = key_dim ** -0.5, rounded to fp32 once
        TIMED(pf, K_CONV, launch_psa_attention(a, st));
    } else {
        return fail(MI355_EFORMAT, "unknown op type in program");
    }
    return MI355_OK;
}

// The sparse tail of a pass: score stage -> position lists -> (gated dense box branch) -> box branch at the listed positions.
// Everything is enqueued; which of the two forms does the work is decided on the device (SparseArgs.state[8]).
static int launch_sparse_tail(mi355_yolo* h, Prof& pf, int nb, DecodeArgs& d) {
    SparseArgs sa{};
    const bool can_overflow = sparse_lists_can_overflow(h, nb);
    sa.n_levels = h->sp_levels; sa.B = nb; sa.A = h->A; sa.no = h->no(); sa.pred = h->pred; sa.best = h->best;
    sa.conf = h->pass_conf; sa.class_mask = h->pass_cmask; sa.state = h->sp_state;
    int* lists = (int*)h->sp_lists.p;
    for (int l = 0; l < h->sp_levels; ++l) {
        const FileOp& om = h->ops[h->sp_m[l]]; const FileOp& o1 = h->ops[h->sp_b1[l]]; const FileOp& o2 = h->ops[h->sp_b2[l]];
        SparseLevel& L = sa.lv[l];
        L.src = h->view(om.src_buf, om.src_choff); L.src_cs = h->dbuf_cs[om.src_buf]; L.cib = om.src_c / 16;
        L.mid = h->view(om.dst_buf, om.dst_choff); L.mid_cs = h->dbuf_cs[om.dst_buf];
        L.wA = h->dconv[om.conv].wpk; L.biasA = h->dconv[om.conv].bias;
        L.wB = h->dconv[o1.conv].wpk; L.biasB = h->dconv[o1.conv].bias;
        L.wC = h->dconv[o2.conv].wpk; L.biasC = h->dconv[o2.conv].bias;
        L.H = d.lv[l].H; L.W = d.lv[l].W; L.stride = d.lv[l].stride; L.anchor0 = d.lv[l].anchor0;
        // the cap is a share of THIS chunk's positions: a tail chunk uses the head of the full chunk's lists
        L.dil = lists + h->sp_off_dil[l]; L.cand = lists + h->sp_off_cand[l];
        L.cap_dil = L.cap_cand = std::min(h->sp_cap[l], sparse_list_cap(h, (long long)nb * L.H * L.W));
        sa.act = h->plans[h->sp_b1[l]].a.act;
    }
    if (pf.begin(K_DECODE)) return fail(MI355_EHIP, "event");       // one span over the score stage, the reset and the lists
    KCHK(launch_decode(d, false, h->stream, 1));
    HIPCHK(hipMemsetAsync(h->sp_state, 0, 12 * sizeof(int), h->stream));
    KCHK(launch_sparse_lists(sa, h->stream));
    pf.end();
    // the gated dense fall-back (two convs per level and the box decode) is enqueued only where the flag can be raised at all: with the
    // default sparse_cap of 1.0 every list holds the whole chunk, and the launches would each leave at their first instruction
    if (can_overflow) {
        for (int l = 0; l < h->sp_levels; ++l) {
            TIMED(pf, K_CONV, run_conv(fit_frames(h, h->sp_box[l], 3, nb, 0), h->stream));
            TIMED(pf, K_CONV, run_conv(fit_frames(h, h->sp_b1l[l], 3, nb, 0), h->stream));
        }
        d.gate = h->sp_state + 8; d.fallback_count = h->sp_state + 12;
        TIMED(pf, K_DECODE, launch_decode(d, false, h->stream, 2));
    }
    TIMED(pf, K_CONV, launch_sparse_box(sa, h->stream));
    // this chunk's counts travel to pinned host memory behind the kernels (no wait here): infer_impl judges them after the call's
    // own final synchronisation
    if (h->h_sp) {
        const int slot = h->sp_slot++ % 64;
        HIPCHK(hipMemcpyAsync(h->h_sp + 12 * slot, h->sp_state, 12 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        for (int l = 0; l < 3; ++l) h->h_sp_pos[slot][l] = l < h->sp_levels ? (long long)nb * sa.lv[l].H * sa.lv[l].W : 0;
    }
    ++h->sp_passes;
    return MI355_OK;
}

int launch_net(mi355_yolo* h, Prof& pf, const uint8_t* stem_in, int nb, const Geometry& g, bool full_pred) {
    const Pass p{h, pf, stem_in, nb, g, h->sparse_shape && !full_pred && !h->sp_dense_now};
    // several streams along the dependency DAG (profiling keeps the single in-order stream; under hipGraph capture the
    // event waits fork the aux streams into the capture and the decode join brings them back)
    const bool multi = h->n_streams > 1 && !h->profiling && nb <= h->streams_max_batch && nb >= h->streams_min_batch;
    if (!multi && !h->steps.empty() && nb == h->cur_nb) {
        // single in-order stream, step by step: the ops of a step are mutually independent; its grouped convs are one grid
        for (const auto& stp : h->steps) {
            for (int i : stp.singles) { const int rc = launch_op(p, (size_t)i, h->stream); if (rc) return rc; }
            if (stp.group >= 0) TIMED(pf, K_CONV, run_group(h->groups[stp.group], h->stream));
        }
    } else if (!multi) {
        for (size_t i = 0; i < h->ops.size(); ++i) { const int rc = launch_op(p, i, h->stream); if (rc) return rc; }
    } else {
        for (int idx : h->sched_order) {
            const int sid = h->op_stream[idx];
            hipStream_t st = sid == 0 ? h->stream : h->aux[sid - 1];
            for (int dep : h->op_xdeps[idx]) {
                // an upsample fused into its consumer's read side is never launched (its event is never recorded): the
                // consumer already depends on the upsample's SOURCE producer (build_schedule)
                if (h->ops[dep].type == OP_UPSAMPLE && h->fused_away[dep]) continue;
                HIPCHK(hipStreamWaitEvent(st, h->op_done[dep], 0));
            }
            const int rc = launch_op(p, (size_t)idx, st); if (rc) return rc;
            if (h->skip_op[idx] || (p.sparse && h->sp_skip[idx])) continue;              // its event was recorded behind the producer's (fused) launch
            if (h->op_signals[idx] && !(h->ops[idx].type == OP_UPSAMPLE && h->fused_away[idx])) HIPCHK(hipEventRecord(h->op_done[idx], st));
            if (h->fuse2[idx] >= 0 && h->skip_op[h->fuse2[idx]] && h->op_signals[h->fuse2[idx]])
                HIPCHK(hipEventRecord(h->op_done[h->fuse2[idx]], st));
        }
        for (int l : h->leaf_ops)
            if (h->op_stream[l] != 0) HIPCHK(hipStreamWaitEvent(h->stream, h->op_done[l], 0));
    }
    DecodeArgs d{};
    d.n_levels = (int)h->levels.size();
    int a0 = 0;
    for (int l = 0; l < d.n_levels; ++l) {
        const FileLevel& lv = h->levels[l];
        d.lv[l] = HeadLevelArgs{h->dbuf[lv.buf], h->dbuf_cs[lv.buf], (int)lv.box_off, (int)lv.cls_off, (int)lv.kpt_off,
                                g.Hl / (int)lv.stride, g.Wl / (int)lv.stride, (int)lv.stride, a0};
        a0 += (g.Hl / lv.stride) * (g.Wl / lv.stride);
    }
    d.B = nb; d.A = h->A; d.nc = h->hdr.nc; d.nkpt = h->hdr.nkpt; d.kdim = h->hdr.kdim;
    d.pred = h->pred; d.best = h->best;
    if (p.sparse) return launch_sparse_tail(h, pf, nb, d);
    TIMED(pf, K_DECODE, launch_decode(d, full_pred, h->stream));
    return MI355_OK;
}

int prepare_geometry(mi355_yolo* h, const Geometry& g, int imgsz) {
    if (g.resize && (h->tab_h0 != g.h0 || h->tab_w0 != g.w0 || h->tab_imgsz != imgsz)) {
        std::vector<int> xt, yt;
        resize_table(g.Wr, g.w0, xt); resize_table(g.Hr, g.h0, yt);
        // An asynchronous call's queued letterbox launches may still read the tables, and the blocking copies below are not ordered behind
        // the engine's (non-blocking) stream: wait for it.  (The free of the old tables used to order this: hipFree synchronises the device.)
        HIPCHK(hipStreamSynchronize(h->stream));
        GROW(h->d_xtab, xt.size() * 4); GROW(h->d_ytab, yt.size() * 4);
        HIPCHK(hipMemcpy(h->d_xtab.p, xt.data(), xt.size() * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(h->d_ytab.p, yt.data(), yt.size() * 4, hipMemcpyHostToDevice));
        h->tab_h0 = g.h0; h->tab_w0 = g.w0; h->tab_imgsz = imgsz;
    }
    return MI355_OK;
}

static int collect_timing(mi355_yolo* h, Prof& pf, int frames) {
    mi355_timing t{};
    t.frames = frames;
    (void)hipEventElapsedTime(&t.total_ms, h->ev0, h->ev1);
    for (auto& sp : pf.spans) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, h->pev[sp.second], h->pev[sp.second + 1]);
        switch (sp.first) {
            case K_LETTERBOX: t.letterbox_ms += ms; break;
            case K_STEM: t.stem_ms += ms; break;
            case K_CONV: t.conv_ms += ms; t.conv_launches++; break;
            case K_POOL: t.pool_ms += ms; break;
            case K_UPSAMPLE: t.upsample_ms += ms; break;
            case K_DECODE: t.decode_ms += ms; break;
            case K_NMS: t.nms_ms += ms; break;
        }
    }
    h->last = t;
    return MI355_OK;
}

// ---------------------------------------------------------------------------------------------- one infer call, step by step
// What the steps of a call hand on: the caller's arguments after defaulting (c), and what was derived from them.
struct CallState {
    InferCall c;
    bool async_out = false;             // packed rows, counts and the row total stay in the caller's DEVICE buffers
    Geometry g{}; int nb = 0; MultiCall mc; YuvCall yc;
    size_t frame_bytes = 0, slot_bytes = 0;     // one dense frame (single shape); one staging slot = one chunk of host frames
    const unsigned* cmask = nullptr;
    bool single_chunk = false, direct_host = false, sp_adaptive = false;
    bool feats = false;                 // this call produces object features (opts.obj_feats, a blocking form)
    mi355_det* host_rows_dev = nullptr; int* host_counts_dev = nullptr;     // the pinned host buffers as the NMS kernel sees them
    float* host_feats_dev = nullptr;    // ... and the gather kernel (direct rows)
};

// step 1: the arguments, checked and defaulted in the order the ABI documents
static int check_call(mi355_yolo* h, CallState& s) {
    InferCall& c = s.c;
    s.async_out = c.dev_rows != nullptr;
    if (!h || !(c.src || c.multi || c.yuv) || (!s.async_out && (!c.out_rows || !c.out_counts)) || (s.async_out && (!c.dev_counts || !c.dev_total)))
        return fail(MI355_EINVAL, "null argument");
    if (c.yuv) {                        // NV12 / I420 frames: one size -> the single-shape call on the converted frames, else `multi`
        const int rc = yuv_check(c.yuv, c.n); if (rc) return rc;
        YuvCall& yc = s.yc;
        for (int i = 0; i < c.n; ++i) { yc.heights.push_back(c.yuv[i].height); yc.widths.push_back(c.yuv[i].width); }
        for (int i = 1; i < c.n; ++i) yc.same = yc.same && yc.heights[i] == yc.heights[0] && yc.widths[i] == yc.widths[0];
        yc.mf = MultiFrames{nullptr, yc.heights.data(), yc.widths.data(), nullptr, false};    // the converted frames lie where host frames are staged
        c.src = nullptr; c.multi = yc.same ? nullptr : &yc.mf;
        c.height = yc.heights[0]; c.width = yc.widths[0]; c.row_stride = 0;
    }
    if (c.multi) {                      // frames of different sizes: the size arguments are per frame (mi355_yolo_infer_multi)
        if (!c.yuv) { const int rc = multi_check(*c.multi, c.n); if (rc) return rc; c.on_device = c.multi->on_device; }
        c.height = c.width = 1; c.row_stride = 0;
    }
    if (c.n <= 0 || c.height <= 0 || c.width <= 0) return fail(MI355_EINVAL, "n, height and width must be positive");
    if (c.max_det <= 0) c.max_det = 300;
    if (c.max_det > 1024) return fail(MI355_EINVAL, "max_det must be <= 1024");
    if (c.cap < 1) return fail(MI355_EINVAL, "out_capacity_per_image must be >= 1");
    if (c.imgsz <= 0) c.imgsz = 640;
    if (c.imgsz % 32) return fail(MI355_EINVAL, "imgsz must be a multiple of 32");
    if (c.row_stride == 0) c.row_stride = c.width * 3;
    if (c.row_stride < c.width * 3) return fail(MI355_EINVAL, "row_stride_bytes smaller than a row");
    if (c.n_classes < 0 || (c.n_classes > 0 && !c.classes)) return fail(MI355_EINVAL, "bad classes argument");
    return MI355_OK;
}

// step 2: frames per pass, the canvas and its launch plans, the letterbox geometry (mixed sizes: per frame, in s.mc)
static int call_shape(mi355_yolo* h, CallState& s) {
    const InferCall& c = s.c;
    s.g = make_geometry(c.height, c.width, c.imgsz);
    s.nb = std::min(c.n, h->chunk);
    s.single_chunk = c.n <= s.nb;
    if (c.yuv && !c.on_device) yuv_layout(c.yuv, c.n, s.nb, s.yc);
    if (c.multi) {
        multi_prepare(*c.multi, c.n, s.nb, c.imgsz, s.mc);
        s.slot_bytes = s.mc.slot_bytes;                     // the largest chunk's frames, packed
        s.yc.bgr_off = s.mc.stage_off;                      // (YUV frames: where the conversion writes them)
        return ensure_shape(h, s.nb, s.mc.Hd, s.mc.Wd);
    }
    s.frame_bytes = (size_t)c.height * c.width * 3;
    s.slot_bytes = (size_t)s.nb * s.frame_bytes;
    for (int i = 0; c.yuv && i < c.n; ++i) s.yc.bgr_off.push_back((size_t)(i % s.nb) * s.frame_bytes);
    const int rc = ensure_shape(h, s.nb, s.g.Hl, s.g.Wl); if (rc) return rc;
    return prepare_geometry(h, s.g, c.imgsz);
}

// step 3: the row and count scratch of a call of n frames (the staging area grows where the first chunk is staged)
static int grow_scratch(mi355_yolo* h, const CallState& s) {
    const size_t n = (size_t)s.c.n, rows = n * s.c.max_det * sizeof(mi355_det);
    GROW(h->d_rows, rows);
    GROW(h->d_counts, (2 * n + 3 * (size_t)h->chunk) * sizeof(int));    // + [counts | candidate counts | sort lengths] of one chunk
    GROW(h->d_packed, rows);
    GROW(h->d_offsets, (n + 1) * sizeof(int));
    if (!s.async_out) GROW(h->h_rows, rows);
    GROW(h->h_counts, n * sizeof(int));
    if (s.feats) {                      // the features follow the rows: slots on the device, packed copy, pinned host copy
        const size_t fb = n * s.c.max_det * h->feat_dim * sizeof(float);
        GROW(h->d_feats, fb); GROW(h->d_feats_packed, fb); GROW(h->h_feats, fb);
    }
    return MI355_OK;
}

// Host frames of chunk [s0, s0 + m) -> staging slot `slot` of d_in, on the copy stream: chunk k+1 is copied while chunk k's kernels
// run; a slot is only overwritten after the kernels that read it (letterbox / stem) have been passed.
static int copy_chunk(mi355_yolo* h, const CallState& s, int s0, int m, int slot) {
    const InferCall& c = s.c;
    if (c.yuv) return yuv_stage_chunk(h, c.yuv, s.yc, s0, m, slot);
    if (c.multi) return multi_stage_chunk(h, *c.multi, s.mc, s0, m, slot);
    HIPCHK(hipStreamWaitEvent(h->copy_stream, h->ev_consumed[slot], 0));
    HIPCHK(hipMemcpy2DAsync(h->d_in.p + (size_t)slot * s.slot_bytes, (size_t)c.width * 3, c.src + (size_t)s0 * c.height * c.row_stride,
                            (size_t)c.row_stride, (size_t)c.width * 3, (size_t)c.height * m, hipMemcpyHostToDevice, h->copy_stream));
    HIPCHK(hipEventRecord(h->ev_copied[slot], h->copy_stream));
    return MI355_OK;
}

// step 4: the class list as a bit mask on the device (ids outside [0, nc) are ignored)
static int class_mask(mi355_yolo* h, CallState& s) {
    const InferCall& c = s.c;
    if (c.n_classes <= 0) return MI355_OK;
    const int words = ((int)h->hdr.nc + 31) / 32;
    GROW(h->d_cmask, words * 4); GROW(h->h_cmask, words * 4);
    unsigned* hm = (unsigned*)h->h_cmask.p;
    std::memset(hm, 0, words * 4);
    for (int i = 0; i < c.n_classes; ++i)
        if (c.classes[i] >= 0 && c.classes[i] < (int)h->hdr.nc) hm[c.classes[i] >> 5] |= 1u << (c.classes[i] & 31);
    HIPCHK(hipMemcpyAsync(h->d_cmask.p, hm, words * 4, hipMemcpyHostToDevice, h->stream));
    s.cmask = (const unsigned*)h->d_cmask.p;
    return MI355_OK;
}

// step 5: call-to-call feedback of the sparse box branch, before the call: where the previous synchronous call's data
// did not favour the sparse kernels the dense head runs, and every 64th such call probes the sparse one again; a call with another
// conf or class filter starts afresh.
static int sparse_feedback_before(mi355_yolo* h, CallState& s) {
    const InferCall& c = s.c;
    h->pass_conf = c.conf; h->pass_cmask = s.cmask;       // the sparse box branch filters its positions as nms_collect will
    s.sp_adaptive = h->sparse_shape && !getenv("MI355_SPARSE_BOX");
    unsigned long long filt = 1469598103934665603ull;
    for (int i = 0; i < c.n_classes; ++i) filt = (filt ^ (unsigned)c.classes[i]) * 1099511628211ull;
    if (c.conf != h->sp_last_conf || filt != h->sp_last_filter) { h->sp_prefer_dense = false; h->sp_dense_calls = 0; }
    h->sp_last_conf = c.conf; h->sp_last_filter = filt;
    h->sp_dense_now = s.sp_adaptive && h->sp_prefer_dense && (++h->sp_dense_calls % 64) != 0;
    if (s.sp_adaptive && !h->h_sp) HIPCHK(hipHostMalloc(&h->h_sp, 64 * 12 * sizeof(int)));
    h->sp_slot = 0;
    return MI355_OK;
}

// step 8: ... and after it, behind the call's final synchronisation (nothing of it is inside a pass); then the timing
static int sparse_feedback_after(mi355_yolo* h, const CallState& s, Prof& pf) {
    if (s.sp_adaptive && !h->sp_dense_now && h->h_sp) {
        bool over = false;
        for (int c = 0; c < std::min(h->sp_slot, 64); ++c) {          // every chunk of the call (the last 64 of a longer one)
            const int* st = h->h_sp + 12 * c;
            over |= st[8] != 0;
            for (int l = 0; l < h->sp_levels; ++l) over |= (double)st[l] > (double)h->sparse_max_share * (double)h->h_sp_pos[c][l];
        }
        h->sp_prefer_dense = over; h->sp_dense_calls = 0;
    }
    return collect_timing(h, pf, s.c.n);
}

// step 6: chunk by chunk: the net, then NMS into the row slots of the chunk's frames
static int run_chunks(mi355_yolo* h, const CallState& s, Prof& pf) {
    const InferCall& c = s.c;
    const int n = c.n, nb = s.nb;
    for (int s0 = 0, ci = 0; s0 < n; s0 += nb, ++ci) {
        const int m = std::min(nb, n - s0);
        const uint8_t* chunk_frames = c.multi || c.yuv ? nullptr : c.src + (size_t)s0 * s.frame_bytes;
        if (!c.on_device) {
            HIPCHK(hipStreamWaitEvent(h->stream, h->ev_copied[ci & 1], 0));
            chunk_frames = h->d_in.p + (size_t)(ci & 1) * s.slot_bytes;
        }
        if (c.yuv) {                    // NV12 / I420 planes (staged, or the caller's on the device) -> the BGR frames of this chunk's d_in slot
            const int rc = yuv_convert_chunk(h, pf, s.yc, s0, m); if (rc) return rc;
            chunk_frames = h->d_in.p + (size_t)(ci & 1) * s.slot_bytes;
        }
        int rc = c.multi ? run_chunk_multi(h, pf, s.mc, s0, m, false) : run_chunk(h, pf, chunk_frames, m, s.g, false); if (rc) return rc;
        if (!c.on_device) {
            // the frames of this slot have been consumed once the net's kernels are enqueued behind this event; the
            // (host-blocking) copy of the next chunk is issued AFTER this chunk's launches so that it overlaps them
            HIPCHK(hipEventRecord(h->ev_consumed[ci & 1], h->stream));
            if (s0 + nb < n) { rc = copy_chunk(h, s, s0 + nb, std::min(nb, n - s0 - nb), (ci + 1) & 1); if (rc) return rc; }
        }
        NmsArgs na{};
        na.pred = h->pred; na.best = h->best; na.B = m; na.A = h->A; na.no = h->no(); na.nc = h->hdr.nc;
        na.nk = h->hdr.nkpt * h->hdr.kdim; na.kdim = h->hdr.kdim;
        na.conf = c.conf; na.iou = c.iou; na.max_det = c.max_det; na.max_nms = 30000; na.max_wh = 7680.f;
        na.class_mask = s.cmask; na.keys = h->keys; na.Apow2 = h->Apow2;
        na.scale_back = 1; na.gain = (float)s.g.gain; na.pad_x = (float)s.g.pad_x; na.pad_y = (float)s.g.pad_y;
        na.kpad_x = (float)s.g.kpad_x; na.kpad_y = (float)s.g.kpad_y; na.orig_w = (float)c.width; na.orig_h = (float)c.height;
        if (c.multi) na.frame_geom = s.mc.d_geom + (size_t)s0 * 7;      // this chunk's frames' rows of [n][7]
        na.out_rows = h->rows_dev() + (size_t)s0 * c.max_det;
        if (s.direct_host) {                     // rows and counts straight into the pinned host buffers (slot layout: frame i at i * max_det)
            na.out_rows = s.host_rows_dev;
            na.host_counts = s.host_counts_dev;
        }
        // one chunk: the sort kernels' scratch [n, 3n) lies inside the counts allocation (2n + 3 * chunk ints, n <= chunk).  Several:
        // counts of this chunk belong at [s0, s0 + m), but the sort kernels use out_counts[B, 3B) as scratch: they run on a temporary
        // block [2n, 2n + 3 * chunk) and the counts are copied into place
        na.out_counts = s.single_chunk ? h->counts_dev() : h->counts_dev() + 2 * n;
        if (pf.begin(K_NMS)) return fail(MI355_EHIP, "event");
        KCHK(launch_nms(na, h->stream));
        if (!s.single_chunk) HIPCHK(hipMemcpyAsync(h->counts_dev() + s0, na.out_counts, (size_t)m * sizeof(int), hipMemcpyDeviceToDevice, h->stream));
        if (s.feats) {
            // the kept rows' embeddings, while this chunk's Detect-input maps are still in the arena: the next chunk's pass is enqueued
            // behind this launch.  Rows and counts are read where NMS has just written them (direct rows: the pinned host block).
            ObjFeatArgs fa{};
            fa.n_levels = h->feat_levels; fa.half = h->half ? 1 : 0;
            fa.B = m; fa.cap = c.max_det; fa.A = h->A; fa.dim = h->feat_dim;
            int a0 = 0;
            for (int l = 0; l < h->feat_levels; ++l) {
                const FileOp& o = h->ops[h->feat_src[l]];
                const int sd = h->bufs[o.src_buf].stride_div, H = h->cur_H / sd, W = h->cur_W / sd;
                fa.lv[l] = ObjFeatLevel{h->dbuf[o.src_buf], h->dbuf_cs[o.src_buf], o.src_choff, o.src_c, H, W, a0};
                a0 += H * W;
            }
            fa.rows = na.out_rows; fa.row_words = (int)(sizeof(mi355_det) / 4); fa.anchor_word = (int)(offsetof(mi355_det, anchor_idx) / 4);
            fa.counts = na.out_counts;
            fa.feats = (s.direct_host ? s.host_feats_dev : (float*)h->d_feats.p) + (size_t)s0 * c.max_det * h->feat_dim;
            KCHK(launch_obj_feats(fa, h->stream));
        }
        pf.end();
    }
    return MI355_OK;
}

// step 7, host forms: the features beside the rows.  Direct rows: the gather wrote h_feats at slot i * max_det, nothing is left to do.
// Otherwise the slots are compacted with the rows' offsets and sum(counts) rows of them copied (one more wait: large calls only).
static int fetch_feats(mi355_yolo* h, const CallState& s, size_t total) {
    const InferCall& c = s.c;
    if (!s.direct_host && total) {
        KCHK(launch_compact_rows(h->d_feats.p, h->counts_dev(), c.n, c.max_det, h->feat_dim, (int*)h->d_offsets.p, h->d_feats_packed.p, h->stream));
        HIPCHK(hipMemcpyAsync(h->h_feats.p, h->d_feats_packed.p, total * h->feat_dim * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    h->last_feat_n = c.n; h->last_feat_max_det = c.max_det; h->last_feat_packed = !s.direct_host;
    return MI355_OK;
}

// step 7, host forms: counts clipped to the caller's capacity, frame i's rows from h_rows: packed back to back, or at slot i
static void copy_out(const mi355_yolo* h, const InferCall& c, bool packed) {
    size_t at = 0;
    for (int i = 0; i < c.n; ++i) {
        const int cnt = std::min(h->counts_host()[i], c.cap);
        c.out_counts[i] = cnt;
        std::memcpy(c.out_rows + (size_t)i * c.cap, h->rows_host() + (packed ? at : (size_t)i * c.max_det), (size_t)cnt * sizeof(mi355_det));
        at += (size_t)h->counts_host()[i];
    }
}

// where the call's BGR frames lie on the device now that its chunks are enqueued (mi355_yolo_render reads them until the next call): the
// caller's own memory, or the d_in slot of the frame's chunk -- which only the call's last two chunks still own
static void record_frames(mi355_yolo* h, const CallState& s) {
    const InferCall& c = s.c;
    const int nchunks = (c.n + s.nb - 1) / s.nb;
    h->last_frames.resize((size_t)c.n);
    for (int i = 0; i < c.n; ++i) {
        mi355_yolo::LastFrame& f = h->last_frames[i];
        f.h = c.multi ? c.multi->heights[i] : c.height; f.w = c.multi ? c.multi->widths[i] : c.width; f.pitch = f.w * 3;
        if (c.on_device && !c.yuv) {
            if (c.multi) { f.p = c.multi->frames[i]; if (c.multi->row_strides && c.multi->row_strides[i]) f.pitch = c.multi->row_strides[i]; }
            else f.p = c.src + (size_t)i * s.frame_bytes;
            continue;
        }
        const int ci = i / s.nb;
        const size_t off = c.multi ? s.mc.stage_off[i] : (size_t)(i % s.nb) * s.frame_bytes;
        f.p = ci >= nchunks - 2 ? h->d_in.p + (size_t)(ci & 1) * s.slot_bytes + off : nullptr;
    }
}

int infer_impl(mi355_yolo* h, const InferCall& call) {
    CallState s; s.c = call;
    h->last_frames.clear();
    int rc = check_call(h, s); if (rc) return rc;
    const InferCall& c = s.c;
    HIPCHK(hipSetDevice(h->device));
    if (h->async_pending) {             // an asynchronous call may still be reading the per-call scratch (class mask, row slots)
        HIPCHK(hipStreamSynchronize(h->stream));
        h->async_pending = false;
    }
    h->last_feat_n = 0;                 // until this call has produced its features
    s.feats = h->obj_feats && !s.async_out && !c.tile;      // a tiled call's rows are merged across entries: no features for it
    rc = call_shape(h, s); if (rc) return rc;
    if (!c.on_device || c.yuv) GROW(h->d_in, 2 * s.slot_bytes);     // host frames / converted YUV frames: a double-buffered staging area of two chunks
    if (c.yuv) { rc = yuv_upload(h, c.yuv, c.on_device, c.n, s.nb, s.slot_bytes, s.yc); if (rc) return rc; }
    if (c.multi) { rc = multi_upload(h, *c.multi, c.n, s.nb, s.mc); if (rc) return rc; }    // descriptors point into d_in (host frames)
    if (!c.on_device) {
        HIPCHK(hipEventRecord(h->ev_consumed[0], h->stream));
        HIPCHK(hipEventRecord(h->ev_consumed[1], h->stream));
        rc = copy_chunk(h, s, 0, std::min(s.nb, c.n), 0); if (rc) return rc;
    }
    rc = grow_scratch(h, s); if (rc) return rc;
    rc = class_mask(h, s); if (rc) return rc;
    // Small synchronous calls (the reference's frame-by-frame loop, model.py:38): the greedy NMS kernel writes its rows and
    // counts straight into the pinned host buffers -- no compaction kernels, no copy-engine hand-overs (five stream operations,
    // ~45 us of a 425-us frame at batch 1), one stream synchronisation.  MI355_DIRECT_ROWS=0 keeps the copy path.
    const bool direct_rows_on = getenv("MI355_DIRECT_ROWS") ? atoi(getenv("MI355_DIRECT_ROWS")) != 0 : !(h->opt_flags & MI355_OPT_NO_DIRECT_ROWS);
    s.direct_host = !s.async_out && s.single_chunk && c.n <= 16 && direct_rows_on && !c.tile;   // tiled: the entry rows stay on the device
    if (s.direct_host) {                // taken after the growth: the device view of the pinned blocks as they are now
        HIPCHK(hipHostGetDevicePointer((void**)&s.host_rows_dev, h->h_rows.p, 0));
        HIPCHK(hipHostGetDevicePointer((void**)&s.host_counts_dev, h->h_counts.p, 0));
        if (s.feats) HIPCHK(hipHostGetDevicePointer((void**)&s.host_feats_dev, h->h_feats.p, 0));
    }
    rc = sparse_feedback_before(h, s); if (rc) return rc;
    Prof pf{h};
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    rc = run_chunks(h, s, pf); if (rc) return rc;
    if (!c.tile && !s.async_out) record_frames(h, s);         // (a tiled call's frames are the entries' sources: engine_tiled.hip records them)
    if (c.tile) { rc = tile_merge_enqueue(h, c, pf, direct_rows_on); if (rc) return rc; }      // one launch behind the last chunk's NMS
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    if (c.tile) {                       // only the merged rows travel (engine_tiled.hip)
        rc = tile_merge_fetch(h, c); if (rc) return rc;
        return sparse_feedback_after(h, s, pf);
    }
    const int n = c.n, det_words = (int)(sizeof(mi355_det) / 4);
    if (s.async_out) {
        // packed rows (frame order), counts and their sum go to the caller's device buffers; no host copy, no sync
        KCHK(launch_compact_rows(h->rows_dev(), h->counts_dev(), n, c.max_det, det_words, (int*)h->d_offsets.p, c.dev_rows, h->stream));
        HIPCHK(hipMemcpyAsync(c.dev_counts, h->counts_dev(), (size_t)n * sizeof(int), hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(c.dev_total, (int*)h->d_offsets.p + n, sizeof(int), hipMemcpyDeviceToDevice, h->stream));
        h->async_pending = true;
        return MI355_OK;
    }
    if (s.direct_host) {
        HIPCHK(hipStreamSynchronize(h->stream));
        copy_out(h, c, false);
        if (s.feats) { rc = fetch_feats(h, s, 0); if (rc) return rc; }
        return sparse_feedback_after(h, s, pf);
    }
    // rows -> host: compact on the GPU first (a frame keeps counts[i] of its max_det slots; copying the slots would be 35 MB
    // per 512 frames), then two small copies: the counts, and sum(counts) rows
    mi355_det* packed = (mi355_det*)h->d_packed.p;
    KCHK(launch_compact_rows(h->rows_dev(), h->counts_dev(), n, c.max_det, det_words, (int*)h->d_offsets.p, packed, h->stream));
    HIPCHK(hipMemcpyAsync(h->counts_host(), h->counts_dev(), (size_t)n * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    // Small calls (the reference's frame-by-frame loop): the first rows travel speculatively behind the counts, so that one
    // stream synchronisation serves both copies (a sync costs 15-20 us; at batch 1 the whole frame takes 500); a second
    // copy follows only when a call keeps more rows than were guessed.
    const size_t guess = n <= 16 ? std::min((size_t)n * c.max_det, (size_t)64 * n) : 0;
    if (guess) HIPCHK(hipMemcpyAsync(h->rows_host(), packed, guess * sizeof(mi355_det), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    size_t total = 0;
    for (int i = 0; i < n; ++i) total += (size_t)h->counts_host()[i];
    if (total > guess) {
        HIPCHK(hipMemcpyAsync(h->rows_host() + guess, packed + guess, (total - guess) * sizeof(mi355_det), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    copy_out(h, c, true);
    if (s.feats) { rc = fetch_feats(h, s, total); if (rc) return rc; }
    return sparse_feedback_after(h, s, pf);
}

// ---------------------------------------------------------------------------------------------- the two raw_head entry points
// mi355_yolo_raw_head's own part between the shape query and the first chunk: all n frames in one copy on the engine's stream
static int raw_head_upload(mi355_yolo* h, const RawHeadCall& c, int imgsz, int nb, const Geometry& g) {
    if (!c.bgr) return fail(MI355_EINVAL, "null argument");
    HIPCHK(hipSetDevice(h->device));
    // no wait on async_pending: the copy and the launches go to the engine's stream, behind that call's work (same stream, so ordering
    // holds); prepare_geometry orders its own table upload
    int rc = ensure_shape(h, nb, g.Hl, g.Wl); if (rc) return rc;
    rc = prepare_geometry(h, g, imgsz); if (rc) return rc;
    const size_t row = (size_t)c.width * 3;
    GROW(h->d_in, row * c.height * c.n);
    HIPCHK(hipMemcpy2DAsync(h->d_in.p, row, c.bgr, c.row_stride ? (size_t)c.row_stride : row, row, (size_t)c.height * c.n, hipMemcpyHostToDevice, h->stream));
    return MI355_OK;
}

// mi355_yolo_raw_head_multi's: descriptors now, host frames staged chunk by chunk
static int raw_head_upload_multi(mi355_yolo* h, const RawHeadCall& c, int nb, MultiCall& mc) {
    HIPCHK(hipSetDevice(h->device));
    // waits for an asynchronous call as infer does (mi355_yolo_raw_head does not: same stream, so ordering holds there)
    if (h->async_pending) { HIPCHK(hipStreamSynchronize(h->stream)); h->async_pending = false; }
    const int rc = ensure_shape(h, nb, mc.Hd, mc.Wd); if (rc) return rc;
    if (!c.multi->on_device) GROW(h->d_in, mc.slot_bytes * 2);
    return multi_upload(h, *c.multi, c.n, nb, mc);
}

// What the two entry points share: imgsz, the anchor count and the shape query, the transposed head's buffer, and the chunk loop (net
// with the full decode, transpose, copy out, synchronise).  Profiling is off inside and back on every way out.
int raw_head_impl(mi355_yolo* h, const RawHeadCall& c) {
    h->last_frames.clear();             // d_in is about to hold this call's frames
    int imgsz = c.imgsz;
    if (imgsz <= 0) imgsz = 640;
    if (imgsz % 32) return fail(MI355_EINVAL, "imgsz must be a multiple of 32");
    const int n = c.n, nb = std::min(n, h->chunk);
    Geometry g{}; MultiCall mc;
    if (c.multi) multi_prepare(*c.multi, n, nb, imgsz, mc);
    else { g = make_geometry(c.height, c.width, imgsz); mc.Hd = g.Hl; mc.Wd = g.Wl; }
    int A = 0;
    for (const FileLevel& lv : h->levels) A += (mc.Hd / lv.stride) * (mc.Wd / lv.stride);
    *c.out_channels = h->no(); *c.out_anchors = A;
    if (!c.out) return MI355_OK;
    int rc = c.multi ? raw_head_upload_multi(h, c, nb, mc) : raw_head_upload(h, c, imgsz, nb, g); if (rc) return rc;
    const size_t per = (size_t)A * h->no(), frame_bytes = (size_t)c.height * c.width * 3;
    GROW(h->d_rawhead, per * nb * 4);
    struct ProfilingOff {
        mi355_yolo* h; bool was;
        explicit ProfilingOff(mi355_yolo* h_) : h(h_), was(h_->profiling) { h->profiling = false; }
        ~ProfilingOff() { h->profiling = was; }
    } guard(h);
    Prof pf{h};
    for (int s = 0, ci = 0; s < n; s += nb, ++ci) {
        const int m = std::min(nb, n - s);
        if (c.multi && !c.multi->on_device) {
            HIPCHK(hipEventRecord(h->ev_consumed[ci & 1], h->stream));
            rc = multi_stage_chunk(h, *c.multi, mc, s, m, ci & 1); if (rc) return rc;
            HIPCHK(hipStreamWaitEvent(h->stream, h->ev_copied[ci & 1], 0));
        }
        rc = c.multi ? run_chunk_multi(h, pf, mc, s, m, true) : run_chunk(h, pf, h->d_in.p + (size_t)s * frame_bytes, m, g, true); if (rc) return rc;
        KCHK(launch_transpose_pred(h->pred, (float*)h->d_rawhead.p, m, A, h->no(), h->stream));
        HIPCHK(hipMemcpyAsync(c.out + (size_t)s * per, h->d_rawhead.p, per * m * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    return MI355_OK;
}

}  // namespace mi355
