// Internals shared by the engine's translation units (engine_load / engine_memory / engine_plans / engine_run / engine_abi /
// engine_ops .hip): the .mi355w records, the engine object behind the opaque mi355_yolo handle and the functions that cross files.
// Replaces what the reference reaches through ultralytics (model.py:18,38): Model.__init__/AutoBackend (weights + fuse),
// BasePredictor.stream_inference (preprocess -> model -> postprocess).
#pragma once
#include "common.h"
#include "dev_buf.h"
#include "crop_resize.h"
#include "../../include/mi355_yolo.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>
#include <sys/stat.h>
#include <unistd.h>

namespace mi355 {

extern thread_local std::string g_err;          // engine_abi.hip; mi355_last_error() reads it
inline int fail(int code, const std::string& msg) { g_err = msg; return code; }

#define HIPCHK(expr)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return fail(MI355_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_));      \
    } while (0)
#define KCHK(expr)                                                                           \
    do {                                                                                     \
        const char* m_ = (expr);                                                             \
        if (m_) return fail(MI355_EHIP, std::string("launch failed: ") + m_);                \
    } while (0)
// one launch inside a profiling span of `kind` (Prof below: two branches on a flag when profiling is off)
#define TIMED(pf, kind, expr)                                                                \
    do {                                                                                     \
        if ((pf).begin(kind)) return fail(MI355_EHIP, "event");                              \
        KCHK(expr);                                                                          \
        (pf).end();                                                                          \
    } while (0)
// grow-only scratch (dev_buf.h).  grow_or_fail -> 1 when it reallocated: the owner says beside the call what that invalidates
inline int grow_or_fail(Buf& b, size_t need, const char* name) {
    const int r = buf_grow(b, need);
    if (r < 0) fail(MI355_EHIP, std::string("out of device or pinned memory: ") + name);
    return r;
}
#define GROW(buf, need) do { if (grow_or_fail(buf, need, #buf) < 0) return MI355_EHIP; } while (0)

// render_kernels.hip: the grow-only scratch of render calls -- one device buffer [descriptors | primitives | bins |
// staged host frames], the pinned image of its first two parts and the pinned landing area of host outputs -- and one call: checks, staging, the two launches, the copy back.
// device = -1 runs the host twin.  The call returns behind `st`; launch_ms (or NULL) receives the time from the bins' memset to the end
// of the draw launch.
struct RenderCtx { Buf d_work; Buf h_img{true}, h_out{true}; hipEvent_t ev0 = nullptr, ev1 = nullptr; };
int render_run(RenderCtx& ctx, int device, const mi355_render_frame* frames, int n, const int32_t* const* prims, const int* n_prims,
               const mi355_render_out* outs, hipStream_t st, float* launch_ms);
void render_ctx_free(RenderCtx& ctx);

// crop_kernels.hip: the grow-only scratch of crop calls -- one device buffer [descriptors | tap tables | staged rows of host
// frames | outputs bound for the host], the pinned image of its first two parts and the pinned landing area of host outputs.  The call
// itself (crops_call, crops_run_gpu) is declared in crop_resize.h.
struct CropCtx { Buf d_work; Buf h_img{true}, h_out{true}; hipEvent_t ev0 = nullptr, ev1 = nullptr; };
void crop_ctx_free(CropCtx& ctx);

// jpeg_kernels.hip: the grow-only scratch of JPEG calls -- one device buffer [descriptors | tables | lengths | headers |
// per frame: coefficients, segment words, segment sizes, stream | staged host frames], the pinned image of its first part and the pinned
// landing areas of the lengths and the streams -- and one call: checks, staging, the three launches (the transform launch alone when
// `coefs` is given instead of `outs`), the copy back of the streams' bytes.  device = -1 runs the host twin.  launch_ms (or NULL) receives
// the device time of the launches.
struct JpegCtx { Buf d_work; Buf h_img{true}, h_out{true}, h_len{true}; hipEvent_t ev0 = nullptr, ev1 = nullptr; };
int jpeg_run(JpegCtx& ctx, int device, const mi355_render_frame* frames, int n, int quality, int subsampling, mi355_jpeg_out* outs,
             int16_t* const* coefs, hipStream_t st, float* launch_ms);
void jpeg_ctx_free(JpegCtx& ctx);

// jpeg_decode_kernels.hip: the grow-only scratch of JPEG decode calls -- one device buffer [descriptors | Huffman tables |
// status | per frame: segment offsets (sync: segment and sequence tables) and scan bytes, or host-decoded coefficients || coefficients of
// the lane and sync frames | a sync frame's states, counts and block indices | planes | frames bound for the host], the pinned image of its first part and the pinned landing areas of the frames and the status words.  The calls
// themselves are declared in jpeg_decode.h.
struct JpegDecCtx { Buf d_work; Buf h_img{true}, h_out{true}, h_stat{true}; hipEvent_t ev0 = nullptr, ev1 = nullptr; };
void jpeg_dec_ctx_free(JpegDecCtx& ctx);

// OP_DWCONV / OP_ATTN (YOLO11, file version 2): FileOp.r0 = groups (== channels) / heads; for OP_ATTN k = key_dim, s = head_dim
enum { OP_STEM = 0, OP_CONV = 1, OP_UPSAMPLE = 2, OP_SPPF_POOL = 3, OP_DWCONV = 4, OP_ATTN = 5 };

#pragma pack(push, 1)
struct FileHeader {
    char magic[8];
    uint32_t version, header_bytes;
    uint32_t family, scale, task, nc, nkpt, kdim, reg_max;
    uint32_t n_buffers, n_ops, n_convs, n_levels;
    uint32_t json_off, json_bytes;
    uint64_t data_bytes;
};
struct FileBuf { uint32_t channels, stride_div; };
struct FileOp { int32_t type, k, s, act, src_buf, src_choff, src_c, dst_buf, dst_choff, dst_c, res_buf, res_choff, conv, pad, r0, r1; };
struct FileConv { char name[64]; uint32_t cin, cout, k, s, pad, act; uint64_t w_off, b_off; };
struct FileLevel { uint32_t buf, box_off, cls_off, kpt_off, stride; };
#pragma pack(pop)

struct DevConv { float* wpk = nullptr; float* bias = nullptr; float* w_raw = nullptr; void* w_frag = nullptr; };   // w_frag: stem3_weight_frags (half k3 stems)
                                                                                                             // depthwise convs: w_raw = [k*k][round_up(c, 4)]

// LetterBox geometry (data/augment.py:LetterBox, auto=True, scaleup=True, center=True, stride 32) and the
// scale-back constants of utils/ops.py:scale_boxes / scale_coords, in the same double arithmetic as Python.
// auto_pad = false: LetterBox((imgsz, imgsz), auto=False), the square canvas BasePredictor.pre_transform uses when the frames of
// one call do not all have the same shape (Hl = Wl = imgsz, the padding is not reduced modulo 32).
struct Geometry {
    int h0, w0, Hl, Wl;          // original and letterboxed size
    int Hr, Wr, top, left;       // resized region
    bool resize, identity;
    double gain; double pad_x, pad_y, kpad_x, kpad_y;
};

inline double py_round(double x) { return std::nearbyint(x); }   // round-half-even, like Python's round()
inline size_t round_up_sz(size_t x, size_t m) { return (x + m - 1) / m * m; }

inline Geometry make_geometry(int h0, int w0, int imgsz, bool auto_pad = true) {
    Geometry g{};
    g.h0 = h0; g.w0 = w0;
    const double r = std::min((double)imgsz / h0, (double)imgsz / w0);
    g.Wr = (int)py_round(w0 * r); g.Hr = (int)py_round(h0 * r);
    double dw = imgsz - g.Wr, dh = imgsz - g.Hr;
    if (auto_pad) { dw = std::fmod(dw, 32.0); dh = std::fmod(dh, 32.0); }
    dw /= 2; dh /= 2;
    const int top = (int)py_round(dh - 0.1), bottom = (int)py_round(dh + 0.1);
    const int left = (int)py_round(dw - 0.1), right = (int)py_round(dw + 0.1);
    g.top = top; g.left = left;
    g.Hl = g.Hr + top + bottom; g.Wl = g.Wr + left + right;
    g.resize = (g.Wr != w0) || (g.Hr != h0);
    g.identity = !g.resize && top == 0 && left == 0 && bottom == 0 && right == 0;
    g.gain = std::min((double)g.Hl / h0, (double)g.Wl / w0);
    g.pad_x = py_round((g.Wl - w0 * g.gain) / 2 - 0.1);
    g.pad_y = py_round((g.Hl - h0 * g.gain) / 2 - 0.1);
    g.kpad_x = (g.Wl - w0 * g.gain) / 2;
    g.kpad_y = (g.Hl - h0 * g.gain) / 2;
    return g;
}

// cv2.resize(INTER_LINEAR) coefficient table: for each destination index: source index, 2 taps in 1/2048 units.  The arithmetic is
// crop_resize.h's crop_tap_table (that header also builds without HIP, for the crop host twin): the letterbox kernel and the crop
// kernel read tables of ONE builder
inline void resize_table(int dn, int sn, std::vector<int>& tab) {
    tab.resize((size_t)dn * 3);
    crop_tap_table(dn, sn, tab.data());
}

}  // namespace mi355

using namespace mi355;

struct mi355_yolo {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t copy_stream = nullptr;  // H2D of the next chunk overlaps the current chunk's kernels (host-frame entry point)
    hipEvent_t ev_copied[2] = {nullptr, nullptr}, ev_consumed[2] = {nullptr, nullptr};
    FileHeader hdr{};
    std::vector<FileBuf> bufs;
    std::vector<FileOp> ops;
    std::vector<FileConv> convs;
    std::vector<FileLevel> levels;
    std::vector<DevConv> dconv;
    float* lut = nullptr;
    float* zeros = nullptr;             // 256 zero bytes: DMA source of padded LDS slots
    int chunk = 64;
    // tuned launch-plan choice per (frames, H, W): candidate index per op, so a shape seen before is not re-timed
    std::vector<std::pair<std::array<int, 3>, std::vector<int>>> tuned;
    int autotune = 32;                  // candidate launch plans timed per conv when a shape is first seen (0 = off)
    long long n_params = 0, macs640 = 0;

    // per-shape state: activation buffers are GROW-ONLY for a letterboxed size (alloc_nb frames); launch plans belong to
    // (cur_nb, cur_H, cur_W) and are rebuilt -- from the tuned-choice cache, without touching the buffers -- when only the
    // frame count of a call changes (sweep tails, track() at n = 1 between batched predicts)
    int cur_nb = 0, cur_H = 0, cur_W = 0, alloc_nb = 0;
    long long act_bytes = 0;            // bytes of activation buffers currently allocated
    unsigned long long model_hash = 0;  // FNV-1a of the .mi355w image: key of the persisted plan choices
    std::vector<float*> dbuf;           // activation buffers (fp32, or fp16 bytes behind a float* when `half`): views into `arena`
    bool host_only = false;             // mi355_memory_plan: program analysis without a device (no weights uploaded, nothing launched)
    char* arena = nullptr;              // ONE allocation; buffers whose lifetimes cannot overlap under ANY legal schedule share bytes
    int mem_reuse = 1;                  // MI355_OPT_NO_MEM_REUSE: every buffer gets bytes of its own (the round-1/2 layout)
    // mi355_opts (include/mi355_yolo.h); the MI355_* environment variables override them for A/B runs only
    int opt_flags = 0;                  // MI355_OPT_*
    bool fast_act = false;              // opts.fast_act: v_exp / v_rcp SiLU in the fp32 conv epilogues (tolerance mode)
    std::string plan_dir;               // shipped plan files, read-only, looked up first ("" = none)
    std::string plan_cache_dir;         // freshly timed choices are written here ("" = not persisted)
    bool plan_cache_on = true;
    long long act_bytes_noreuse = 0;    // what the same shape takes without sharing (reported beside act_bytes)
    std::vector<std::vector<unsigned long long>> anc;   // anc[i] = bitset over ops: RAW ancestors of op i (transitive)
    std::vector<int> dbuf_cs;           // pixel stride in ELEMENTS of the buffer's dtype
    std::vector<int> dbuf_es;           // element size in bytes: 4, or 2 for the fp16 buffers of the half=True path
    bool half = false;                  // opts.half: fp16 storage of activations / weights, fp32 arithmetic (conv_igemm_f16.hip)
    float* view(int buf, int choff) const { return (float*)((char*)dbuf[buf] + (size_t)choff * dbuf_es[buf]); }
    std::vector<ConvLaunch> plans;      // per op (valid for OP_CONV)
    // Upsample -> Concat -> Conv1x1 of the neck, fused on the conv's read side: fuse_up[j] = index of the OP_UPSAMPLE op whose
    // output only conv op j reads (or -1); fused_away[i] = that upsample is not launched.  Decided when the weights are
    // loaded (program structure) and confirmed per shape (a v4 launch plan must exist), MI355_FUSE_UPSAMPLE=0 disables it.
    std::vector<int> fuse_up; std::vector<char> fused_away;
    // Conv3x3 -> Conv1x1 fused into one launch: fuse2[i] = index of the pointwise conv op whose ONLY input is conv op
    // i's output slice, which nobody else reads (or -1): the stride-2 convs in front of every C2f / C3 and the last two convs
    // of every head branch.  Decided from the program at load time, confirmed per shape (a fused launch plan must exist);
    // skip_op[j] = the pointwise op j runs inside its producer's launch.  MI355_FUSE_1X1=0 disables it.
    std::vector<int> fuse2; std::vector<char> skip_op;
    // ... and its generalisation to the tail of a C2f block: the LAST Bottleneck's second 3x3 conv (with its residual) feeds only
    // C2f.cv2, a pointwise conv over cat(ys) whose input slice ENDS with that conv's output: fuse2_lead[i] = the channels of the
    // concat buffer in front of it (read by the fused pointwise stage straight from global memory), 0 = exact-slice pairs.
    std::vector<int> fuse2_lead;
    // Small chunks leave most of the chip idle inside one conv launch, but the graph has independent branches (the box / class /
    // keypoint chains of the three head levels run beside the rest of the neck): ops are dealt to a few HIP streams along the
    // program's dependency DAG (RAW on buffer slices), in depth order, a chain inheriting its producer's stream; an op waits
    // on the events of producers that live on other streams.  Measured gain: +14 % at batch 1, +10 % at 8, +3 % at 64 and
    // still +2 % at 512 (the tails of one launch fill with the blocks of another); MI355_STREAMS=1 turns it off.
    int n_streams = 4, streams_max_batch = 1 << 30, streams_min_batch = 6;   // below 6 frames per pass one in-order stream is faster
                                                  // (round 2, merged + fused program: batch 1 1,990 vs 1,844 frames/s, batch 4 4,780 vs 4,530;
                                                  // batch 8 6,150 vs 6,360): the cross-stream event waits cost more than the overlap buys
    std::vector<hipStream_t> aux;             // streams 1 .. n_streams-1 (0 = `stream`)
    std::vector<hipEvent_t> op_done;          // per op: recorded after its launch when someone on another stream waits for it
    std::vector<int> sched_order, op_stream;  // launch order (depth, index) and stream of each op
    std::vector<std::vector<int>> op_xdeps;   // producers on other streams
    std::vector<char> op_signals;             // op has a consumer on another stream (or is a head output: decode joins on it)
    std::vector<int> leaf_ops;                // ops that write the head-level buffers
    std::vector<std::vector<int>> deps;       // RAW producers of every op (program order indices)
    // Grouped launches (conv_f32_group.hip), the single-stream regime's answer to the idle chip: the launched ops are list-
    // scheduled into STEPS (all ops of a step are mutually independent: every producer ran in an earlier step); the conv ops
    // of a step whose tuned kernel is on the group kernel's menu run as ONE grid when the stopwatch says that beats the
    // separate launches.  group_sel[i] >= 0: op i runs inside its step's group with plan group_sel[i] of its candidate list
    // (fused list when its pointwise consumer runs inside it).  MI355_GROUPS=0 turns it off.
    struct Step { std::vector<int> singles; int group = -1; };
    std::vector<Step> steps;
    std::vector<GroupLaunch> groups;
    std::vector<int> group_sel;
    int use_groups = 1, group_max_batch = 5;
    // Sparse box branch (conv_f32_sparse.hip): the head's box chain cv2.i.0 -> cv2.i.1 -> cv2.i.2 -> DFL runs at the
    // anchors that reach NMS only.  sp_m / sp_b1 / sp_b2[l] = the ops of level l (cv2.i.0 alone or merged with its siblings, cv2.i.1,
    // cv2.i.2), found from the program when the weights are loaded (sp_levels = 0: the program has no such head).  sparse_shape:
    // the current shape runs it (decided per shape like the other fusions; MI355_SPARSE_BOX=0/1 overrides the frames-per-pass
    // threshold).  sp_cls = the merged conv without its box couts, sp_box = its box couts alone and sp_b1 = cv2.i.1 (+ fused
    // cv2.i.2) as gated launches: they leave at once unless a position list overflowed its capacity in this chunk.
    int sp_levels = 0, sp_m[3] = {-1, -1, -1}, sp_b1[3] = {-1, -1, -1}, sp_b2[3] = {-1, -1, -1};
    std::vector<char> sp_skip, sp_late;       // per op: not launched in a sparse pass; per buffer: read by the sparse tail, after the last op of a pass
    std::vector<char> late_read;              // sp_late for the shapes that may run the sparse tail (plan_memory), empty otherwise
    bool sparse_shape = false; int sparse_why = 1;   // why the current shape keeps the dense head (prepare_sparse_shape), 0 = it does not
    int sparse_min_batch = 32;          // frames per pass from which the sparse branch wins
    float sparse_cap = 1.0f;            // share of a level's positions the lists hold; beyond it the dense launches run
    ConvLaunch sp_cls[3], sp_box[3], sp_b1l[3];
    int* sp_state = nullptr;            // device: 12 ints of SparseArgs.state + [12] dense fall-backs so far
    Buf sp_lists;                       // int: per level the dilated list, then the candidate list
    int sp_cap[3] = {0, 0, 0}; size_t sp_off_dil[3] = {0, 0, 0}, sp_off_cand[3] = {0, 0, 0};   // list capacities / offsets into sp_lists of the current shape
    float pass_conf = 0.25f; const unsigned* pass_cmask = nullptr;   // the call's candidate filter (infer_impl sets them before its chunks)
    long long sp_passes = 0;
    // Feedback from the data, outside the pass: every sparse chunk's counts are copied asynchronously to pinned
    // memory (h_sp, 64 slots) and read after a synchronous call's own final stream synchronisation; when a list overflowed or a
    // level's dilated share exceeded sparse_max_share (where the sparse kernels stop winning) the following calls with the same
    // conf and class filter run the dense head, and every 64th of them probes the sparse one again.  Off under MI355_SPARSE_BOX=0/1
    // (A/B runs want one path); asynchronous device-output calls neither update nor reset it.
    int* h_sp = nullptr; long long h_sp_pos[64][3] = {}; int sp_slot = 0; float sp_last_conf = -1.f; unsigned long long sp_last_filter = 0;
    bool sp_prefer_dense = false, sp_dense_now = false; int sp_dense_calls = 0; float sparse_max_share = 0.5f;
    float* pred = nullptr; float2* best = nullptr; unsigned long long* keys = nullptr;
    int A = 0, Apow2 = 0;
    uint8_t* lbox = nullptr;            // letterboxed frames of one chunk (also the stable stem input of the graph path)
    std::vector<std::pair<int, hipGraphExec_t>> graphs;   // (frames in chunk, captured stem..decode sequence)
    int use_graph = 0;                  // MI355_GRAPH=1: replay stem..decode as a hipGraph (measured: no gain, the small-batch
                                        // regime is bound by per-kernel latency of tiny grids, not by host launches)
    // per-call scratch, grow-only (dev_buf.h; h_* = pinned host memory)
    Buf d_in;                           // staged host frames: two chunk slots (infer), all n frames (raw_head)
    Buf d_rows, d_counts;               // mi355_det [n][max_det]; int [2n + 3 * chunk]: counts, sort scratch, one chunk's temporary block
    Buf d_packed, d_offsets;            // rows compacted on the GPU before the D2H copy; int [n + 1]
    Buf h_rows{true}, h_counts{true};
    Buf d_cmask, h_cmask{true};         // unsigned [ceil(nc / 32)]
    Buf d_xtab, d_ytab; int tab_h0 = -1, tab_w0 = -1, tab_imgsz = -1;
    Buf d_rawhead;                      // float [nb][A][no]
    mi355_det* rows_dev() const { return (mi355_det*)d_rows.p; }
    int* counts_dev() const { return (int*)d_counts.p; }
    mi355_det* rows_host() const { return (mi355_det*)h_rows.p; }
    int* counts_host() const { return (int*)h_counts.p; }
    // batches of frames of different sizes (engine_multi.hip): pinned staging of host frames (two chunk slots), and ONE device buffer
    // holding the per-frame letterbox descriptors, the per-frame scale-back constants and the resize tables, uploaded from a pinned
    // image of it (h_multi) -- only when that image changed since the last upload (the same cameras call after call)
    Buf h_stage{true};
    Buf d_multi, h_multi{true}; size_t multi_bytes = 0;   // multi_bytes: what d_multi holds of h_multi's image (0 = nothing)
    // NV12 / I420 frames (engine_yuv.hip): the packed planes of host frames (two chunk slots; pinned staging is h_stage), and the
    // per-frame conversion descriptors of a call with their pinned image
    Buf d_yuv, d_yuvdesc, h_yuvdesc{true};
    // Object features (opts.obj_feats): feat_src[l] = the op whose SOURCE slice is level l's Detect input (cv2.l.0, alone
    // or merged with its siblings), found from the program at load time (feat_levels = 0: not found); feat_dim = min over the levels'
    // channels.  With the option on plan_memory gives those buffers bytes of their own, so the maps outlive the pass until the chunk's
    // NMS and the gather behind it have run.  d_feats [n][max_det][dim] follows d_rows, d_feats_packed d_packed, h_feats h_rows.
    bool obj_feats = false; int feat_levels = 0, feat_src[4] = {-1, -1, -1, -1}, feat_dim = 0;
    Buf d_feats, d_feats_packed, h_feats{true};
    // Tiled predict (engine_tiled.hip): the call's host (or converted YUV) frames, uploaded once each; the per-frame entry
    // ranges and origins of the merge [entry_off (n + 1) | origins (2 per entry)] with their pinned image, uploaded when the bytes change;
    // the merge kernel's key scratch (frames with more than 4096 candidates); its counts and entry indices [counts n | idx slots | idx packed]
    Buf d_tile_frames, d_tile, h_tile{true}, d_tile_keys, d_tile_out, h_tile_out{true}; size_t tile_bytes = 0;
    bool tile_direct = false;           // the last tiled call's merged rows went straight to the pinned host blocks (slot layout)
    // what mi355_yolo_last_feats hands out: the last blocking call's n and max_det, and whether h_feats holds its rows packed in frame
    // order (counts in h_counts) or at slot i * max_det (the direct-rows path); last_feat_n = 0: the last call produced none
    int last_feat_n = 0, last_feat_max_det = 0; bool last_feat_packed = false;
    // Evidence frames (render_kernels.hip): where the BGR frames of the last blocking infer call lie on the device, so that
    // mi355_yolo_render draws them without a second upload -- the d_in slot a host or YUV frame was staged / converted into, the one
    // copy of a tiled call (d_tile_frames), or the caller's own device memory.  p = nullptr: the slot has since been reused (host
    // frames of a call of more than two chunks, except its last two).  Cleared by every infer call before it touches a buffer.
    struct LastFrame { const uint8_t* p; int h, w, pitch; };
    std::vector<LastFrame> last_frames;
    RenderCtx render;
    JpegCtx jpeg;                       // mi355_yolo_encode's scratch
    JpegDecCtx jpeg_dec;                // mi355_yolo_decode's scratch
    CropCtx crops;                      // mi355_yolo_crops' scratch
    unsigned long long plan_hash = 0;   // fingerprint of the candidate lists + the chosen indices of the current shape
    int plan_source = 0, plan_launches = 0;   // 0 static guess (autotune off), 1 memory, 2 this machine's plan cache, 3 tuned now, 4 shipped plan file; launches of one pass (stem..last conv)
    bool async_pending = false;         // mi355_yolo_infer_device_async work may still be in flight on `stream`
    // timing
    bool profiling = false;
    mi355_timing last{};
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::vector<hipEvent_t> pev;        // profiling events

    int no() const { return 4 + (int)hdr.nc + (int)(hdr.nkpt * hdr.kdim); }
    void free_shape();
    ~mi355_yolo();
};

namespace mi355 {

// event bookkeeping for per-kind timing
enum Kind { K_LETTERBOX, K_STEM, K_CONV, K_POOL, K_UPSAMPLE, K_DECODE, K_NMS, K_COUNT };
struct Prof {
    mi355_yolo* h; size_t used = 0; std::vector<std::pair<int, size_t>> spans;
    int begin(int kind) {
        if (!h->profiling) return 0;
        if (used + 2 > h->pev.size()) { for (int i = 0; i < 64; ++i) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return -1; h->pev.push_back(e); } }
        spans.push_back({kind, used});
        return hipEventRecord(h->pev[used], h->stream) == hipSuccess ? 0 : -1;
    }
    int end() {
        if (!h->profiling) return 0;
        const int r = hipEventRecord(h->pev[used + 1], h->stream) == hipSuccess ? 0 : -1;
        used += 2; return r;
    }
};

struct DevMem {   // RAII for the one-shot operator entry points
    std::vector<void*> ptrs;
    ~DevMem() { for (void* p : ptrs) (void)hipFree(p); }
    template <class T> hipError_t alloc(T** p, size_t bytes) { hipError_t e = hipMalloc(p, bytes ? bytes : 16); if (e == hipSuccess) ptrs.push_back(*p); return e; }
};

// engine_load.hip: .mi355w image -> op program, weights on the device, dependency DAG + stream assignment
int parse_blob(mi355_yolo* h, const uint8_t* blob, size_t n);
int create_impl(const uint8_t* blob, size_t nbytes, int device_id, const mi355_opts* opts, mi355_yolo** out);
// engine_run.hip: the sparse box branch: program analysis (at load), per-shape launches, statistics
void detect_sparse_head(mi355_yolo* h);
void detect_feature_sources(mi355_yolo* h);                       // the three Detect-input slices (object features)
bool sparse_wanted(const mi355_yolo* h, int nb);
int prepare_sparse_shape(mi355_yolo* h, int nb, int Hl, int Wl);
ConvLaunch cout_subrange(const ConvLaunch& l0, int t0, int nt);   // a planned 3x3 launch over the cout tiles [t0, t0 + nt) of its conv
bool sparse_lists_can_overflow(const mi355_yolo* h, int nb);   // a chunk of nb frames of the current shape: is some list shorter than its level's positions?
// engine_memory.hip: liveness-based placement of the activation buffers in ONE arena (host arithmetic only)
void plan_memory(mi355_yolo* h, int nb, int Hl, int Wl, std::vector<size_t>* off_out, std::vector<size_t>* bytes_out,
                 size_t* arena_out, size_t* plain_out);
// engine_plans.hip: buffers + launch plans of (frames per pass, letterboxed H, W): candidate lists, plan files, the stopwatch
int ensure_shape(mi355_yolo* h, int nb, int Hl, int Wl);
// engine_run.hip: one pass of the net, one chunk, one call
int launch_net(mi355_yolo* h, Prof& pf, const uint8_t* stem_in, int nb, const Geometry& g, bool full_pred);
int run_chunk(mi355_yolo* h, Prof& pf, const uint8_t* frames_dev, int nb, const Geometry& g, bool full_pred);
int prepare_geometry(mi355_yolo* h, const Geometry& g, int imgsz);
// engine_multi.hip: one call over frames of different sizes (mi355_yolo_infer_multi).  All frames the same shape: the rect
// geometry of make_geometry (what mi355_yolo_infer does with them stacked); otherwise every frame is letterboxed into the square
// imgsz x imgsz canvas (auto_pad = false) -- Ultralytics' BasePredictor.pre_transform rule.
struct MultiFrames {
    const uint8_t* const* frames; const int* heights; const int* widths; const int* row_strides;   // row_strides may be NULL (w*3)
    bool on_device;
};
struct MultiCall {
    int Hd = 0, Wd = 0;                       // canvas: rect letterbox size of the common shape, or imgsz x imgsz
    std::vector<Geometry> g;                  // per frame
    std::vector<size_t> stage_off;            // host frames: byte offset of frame i inside its chunk's staging slot (rows w*3 apart)
    size_t slot_bytes = 0;                    // host frames: bytes of the largest chunk
    const LetterboxFrame* d_desc = nullptr; const float* d_geom = nullptr; const int* d_tabs = nullptr;
};
// the host image of a call's per-frame data: [descriptors | scale-back rows [n][7] | resize tables], each part 256-byte aligned
struct MultiImage {
    std::vector<char> bytes; size_t geom_off = 0, tabs_off = 0, tab_ints = 0;
};
int multi_check(const MultiFrames& mf, int n);
void multi_prepare(const MultiFrames& mf, int n, int nb, int imgsz, MultiCall& mc);
void multi_image(const MultiFrames& mf, const MultiCall& mc, int n, int nb, const uint8_t* staged, MultiImage& img);
int multi_upload(mi355_yolo* h, const MultiFrames& mf, int n, int nb, MultiCall& mc);
int multi_stage_chunk(mi355_yolo* h, const MultiFrames& mf, const MultiCall& mc, int s0, int m, int slot);
int run_chunk_multi(mi355_yolo* h, Prof& pf, const MultiCall& mc, int s0, int m, bool full_pred);

// engine_yuv.hip: NV12 / I420 frames.  Per chunk ONE conversion launch in front of run_chunk / run_chunk_multi writes
// the dense BGR frames into the d_in slot those read, laid out as a host-frame call's staging would be: frames of one size back to back
// (the single-shape path follows), frames of different sizes at MultiCall.stage_off (the `multi` path follows, fed by YuvCall.mf).  Host
// planes travel chunk by chunk through pinned staging into the two slots of d_yuv, rows packed.
struct YuvCall {
    std::vector<int> heights, widths;         // per frame
    bool same = true;                         // all frames one (h, w)
    MultiFrames mf{};                         // the converted frames of different sizes as the multi path sees them (staged: host layout)
    std::vector<size_t> bgr_off;              // frame i's BGR bytes inside its chunk's d_in slot
    std::vector<size_t> plane_off;            // host planes: frame i's packed planes inside its chunk's d_yuv slot (Y, then chroma)
    size_t yuv_slot_bytes = 0;
    const YuvFrameDesc* d_desc = nullptr;     // device [n]
};
int yuv_check(const mi355_yuv_frame* frames, int n);
YuvFrameDesc yuv_desc(const mi355_yuv_frame& f, uint8_t* dst);     // a frame where it lies, with the caller's strides
void yuv_layout(const mi355_yuv_frame* frames, int n, int nb, YuvCall& yc);
int yuv_upload(mi355_yolo* h, const mi355_yuv_frame* frames, bool on_device, int n, int nb, size_t bgr_slot_bytes, YuvCall& yc);
int yuv_stage_chunk(mi355_yolo* h, const mi355_yuv_frame* frames, const YuvCall& yc, int s0, int m, int slot);
int yuv_convert_chunk(mi355_yolo* h, Prof& pf, const YuvCall& yc, int s0, int m);

// engine_tiled.hip: a tiled call.  The frames of the InferCall are the ENTRIES (every source frame's tiles, then the frame itself), on the
// device; frame f owns entries [entry_off[f], entry_off[f + 1]).  The entry rows stay on the device, one merge launch follows the last
// chunk's NMS and only the merged rows travel to out_rows [n_frames][cap] / out_counts / out_tile_idx (may be NULL).
struct TileCall {
    int n_frames = 0, max_entries = 0;
    std::vector<int> entry_off, origins;                      // [n_frames + 1]; [entries][2] = ox, oy
    int metric = 0; float thr = 0.5f;
    mi355_det* out_rows = nullptr; int cap = 1; int* out_counts = nullptr; int* out_tile_idx = nullptr;
};
struct InferCall;
int tile_merge_enqueue(mi355_yolo* h, const InferCall& c, Prof& pf, bool direct_rows_on);
int tile_merge_fetch(mi355_yolo* h, const InferCall& c);

// engine_run.hip: one infer call.  An entry point fills what it uses: the frames (one dense block of one shape, `multi`, or `yuv`), the
// filter, and one of the two output forms.
struct InferCall {
    const TileCall* tile = nullptr;                           // set by the tiled entry points only (with `multi` = the entry list)
    const uint8_t* src = nullptr; bool on_device = false;
    int n = 0, height = 0, width = 0, row_stride = 0;         // row_stride 0 = width * 3; host frames only
    const MultiFrames* multi = nullptr;                       // frames of different sizes: src, on_device and the sizes above are not read
    const mi355_yuv_frame* yuv = nullptr;                     // n NV12 / I420 frames (on_device: where their planes live): src, multi and the sizes are not read
    float conf = 0.25f, iou = 0.7f; const int* classes = nullptr; int n_classes = 0, max_det = 0, imgsz = 0;
    mi355_det* out_rows = nullptr; int cap = 1; int* out_counts = nullptr;                        // host rows [n][cap] and counts
    mi355_det* dev_rows = nullptr; int* dev_counts = nullptr; int* dev_total = nullptr;          // or: packed device rows, asynchronous
};
int infer_impl(mi355_yolo* h, const InferCall& call);
// ... and one raw_head call: n frames of one shape on the host (bgr), or `multi`; out = NULL asks for the shape only
struct RawHeadCall {
    const uint8_t* bgr = nullptr; int n = 0, height = 0, width = 0, row_stride = 0;
    const MultiFrames* multi = nullptr;
    int imgsz = 0; float* out = nullptr; int* out_channels = nullptr; int* out_anchors = nullptr;
};
int raw_head_impl(mi355_yolo* h, const RawHeadCall& call);

}  // namespace mi355
