// JPEG ingest (include/mi355_yolo.h "jpeg decode"): the decoder's rules, stated once for the kernels
// (jpeg_decode_kernels.hip) and their host twin.  Integers only, and libjpeg's default decoder step for step, so the kernels, the twin and
// Pillow (libjpeg-turbo) give the same bytes.
//
// Streams: baseline sequential DCT (SOF0), 8 bits, Huffman, ONE interleaved scan; 3 components with Y sampled 1x1 (4:4:4), 2x1 (4:2:2) or
// 2x2 (4:2:0) and chroma 1x1, or 1 component (gray: B = G = R = Y).  Any DQT (8-bit steps, ids 0..3), any DHT (ids 0..1 per class), DRI
// optional, APPn / COM skipped.  Everything else is refused by the parser with a reason, before any work.
//   entropy  Annex F.2.2 per restart segment, DC predictors 0 at a segment's start; coefficients int16 [blocks][64] in zigzag order, blocks
//            in scan order, DC absolute (the low 16 bits of the running sum).  Reads past a segment's end supply zero bits; a run that
//            leaves the block, a 16-bit code that matches nothing, a segment that ends early or late set a status -- never a wild store.
//   dequant  coef * step
//   IDCT     libjpeg's jpeg_idct_islow: 13-bit constants, columns first (descale 11: 2 bits kept), then rows (descale 18), every descale
//            (x + (1 << (n - 1))) >> n; sample = clamp(x + 128, 0, 255).  64-bit arithmetic, except for blocks whose sum of |coef * step|
//            is at most kJpegIdctNarrowSum, where every intermediate fits 32 bits (the derivation is in DESIGN.md 3.21).
//   upsample libjpeg's "fancy" (triangle) filter, neighbours clamped to the chroma plane; chroma planes of at most 2 columns are replicated
//   colour   R = Y + ((91881 cr + 32768) >> 16), G = Y + ((-22554 cb - 46802 cr + 32768) >> 16), B = Y + ((116130 cb + 32768) >> 16),
//            cb, cr less 128, each clamped to 0 .. 255; stored B, G, R
#pragma once
#include <stddef.h>

#include "jpeg_codec.h"
#include "../../include/mi355_yolo.h"

#include <cstring>
#include <string>
#include <vector>

namespace mi355 {

// per-frame status of the entropy stage
constexpr int kJpegDecOk = 0, kJpegDecCodeNotFound = 1, kJpegDecRunPastBlock = 2, kJpegDecSegmentShort = 3, kJpegDecSegmentLong = 4;
constexpr long long kJpegIdctNarrowSum = 4094;  // sum of |coef * step| over a block up to which the 32-bit IDCT is exact

inline const char* jpeg_dec_status_name(int s) {
    switch (s) {
        case kJpegDecOk: return "ok";
        case kJpegDecCodeNotFound: return "a 16-bit code matches no Huffman code";
        case kJpegDecRunPastBlock: return "a zero run leaves the block";
        case kJpegDecSegmentShort: return "a segment ends before its last MCU";
        case kJpegDecSegmentLong: return "a segment has bytes left over behind its last MCU";
    }
    return "unknown status";
}

// One Huffman table as the decoder reads it (Annex F.2.2.3 with an 8-bit look-ahead in front)
struct JpegHuff {
    uint16_t look[256];                         // the next 8 bits -> length << 8 | symbol of a code of <= 8 bits; 0: the code is longer
    int32_t maxcode[17];                        // [l], l = 1 .. 16: the largest code of l bits, -1 when there is none
    int32_t valoff[17];                         // [l]: index of the first symbol of l bits minus its code
    uint8_t vals[256];
};

// entropy = sync (jpeg_sync.h): a decoder state, the segment and sequence tables, and what a sync frame's launches work on
constexpr int kJpegSyncSubBytes = 128;          // S of product calls (measured against 64 and 256: DESIGN.md 3.21)
constexpr int kJpegSyncSeqSubs = 256;           // Q: the lanes of a workgroup
struct JpegSyncOpts {                           // mi355_op_jpeg_sync's S and Q, and where its states and stats go
    int S = kJpegSyncSubBytes, Q = kJpegSyncSeqSubs;
    mi355_jpeg_sync_state* states = nullptr;
    mi355_jpeg_sync_stats* stats = nullptr;
};
struct JpegSyncState {
    uint32_t byte, meta;                        // meta: bit | j << 3 | k << 6
};
MI355_HD bool jpeg_sync_same(JpegSyncState a, JpegSyncState b) { return a.byte == b.byte && a.meta == b.meta; }

struct JpegSyncSeg {
    uint32_t begin, len;                        // the segment's bytes within the scan
    uint32_t blk0, nblk;                        // its blocks
    uint32_t sub0, nsub;                        // its subsequences (of the frame's), at least one
    uint32_t seq0, nseq;
};
struct JpegSyncSeq {
    uint32_t seg;
    uint32_t sub0, nsub;                        // of the frame's subsequences
    uint32_t lsub0;                             // sub0's index within its segment
};
// what a sync frame's launches work on: tables from the host, the rest in the work buffer
struct JpegSync {
    int S, Q;
    uint32_t nsub, nseq;
    const JpegSyncSeg* segs;
    const JpegSyncSeq* seqs;
    JpegSyncState* X;                           // [nsub] exit states
    uint32_t* E;                                // [nsub] blocks completed
    uint32_t* B;                                // [nsub] block in progress at the entry
    uint32_t* seq_blk;                          // [nseq] B of a sequence's first subsequence
    JpegSyncState* entry;                       // [nseq] global rounds: the entry read before anything is written
    uint32_t* mark;                             // [2][nseq]
    uint32_t* stats;                            // rounds_local, rounds_global (zeroed with the coefficients)
};

// One frame of a call: geometry and tables from the parser, then the GPU path's pointers
struct JpegDecFrame {
    int H, W, ncomp, hs, vs;                    // Y's sampling factors: 1x1, 2x1, 2x2 (gray: 1x1)
    int mcus_x, mcus_y, bpm;                    // MCUs of 8 hs x 8 vs pixels, blocks per MCU (hs vs + 2, gray 1)
    int ri, nseg, seg_mcus;                     // restart interval (0: none), segments, MCUs per segment (the last may hold fewer)
    int cw, ch;                                 // the chroma planes' real extent: ceil(W / hs) x ceil(H / vs)
    int pitch;                                  // of `out`
    int lanes;                                  // GPU path: 1 when the frame's entropy stage runs on the GPU's lanes, 2: entropy = sync
    uint8_t zigzag[64];                         // GPU path: kJpegZigzag, which device code cannot index
    uint8_t q[3][64];                           // per component: the quantisation steps in zigzag order
    uint8_t dc_tab[3], ac_tab[3];               // per component: index into huff[] (DC tables 0 .. 1, AC tables 2 .. 3)
    const JpegHuff* huff;                       // [4]
    const uint8_t* scan;                        // the entropy-coded bytes; the GPU's copy is 4-byte aligned and padded to whole words
    const uint32_t* seg;                        // [nseg][2]: begin and end of every segment's bytes within `scan` (RSTm excluded)
    int16_t* coef;                              // [blocks][64]
    int* status;
    uint8_t* plane[3]; int pw[3], ph[3];        // component planes, padded to whole MCUs
    uint8_t* out;                               // BGR [H][pitch]
    JpegSync sy;                                // entropy = sync
};
MI355_HD long long jpeg_dec_blocks(const JpegDecFrame& f) { return (long long)f.mcus_x * f.mcus_y * f.bpm; }

// ---- entropy -----------------------------------------------------------------------------------------------------------------------------
// byte i of a segment's bytes: plain on the host ...
struct JpegFetchBytes {
    const uint8_t* p;
    MI355_HD unsigned at(uint32_t i) { return p[i]; }
};
// ... and through aligned 32-bit words on the GPU (base 4-byte aligned, the buffer padded to whole words)
struct JpegFetchWords {
    const uint32_t* w; uint32_t idx = 0xFFFFFFFFu, cur = 0;
    MI355_HD unsigned at(uint32_t i) {
        if ((i >> 2) != idx) { idx = i >> 2; cur = w[idx]; }
        return (cur >> ((i & 3u) * 8u)) & 0xFFu;
    }
};

// a 64-bit window over [pos, end): bytes are unstuffed (FF 00 -> FF) as they are shifted in; past `end` zero bytes arrive and are counted
template <class Fetch>
struct JpegBits {
    Fetch f; uint32_t pos, end; unsigned long long win = 0; int n = 0, pad = 0;
    MI355_HD void fill() {
        while (n <= 56) {
            unsigned b = 0;
            if (pos < end) {
                b = f.at(pos++);
                if (b == 0xFFu && pos < end && f.at(pos) == 0u) ++pos;
            } else ++pad;
            win |= (unsigned long long)b << (56 - n);
            n += 8;
        }
    }
    MI355_HD unsigned peek(int len) const { return (unsigned)(win >> (64 - len)); }     // 1 <= len <= 32
    MI355_HD void drop(int len) { win <<= len; n -= len; }
};

// one symbol: -1 when the next 16 bits match no code.  The window holds at least 32 bits behind a fill.
template <class Bits>
MI355_HD int jpeg_dec_symbol(Bits& b, const JpegHuff& h) {
    const unsigned e = h.look[b.peek(8)];
    if (e) { b.drop((int)(e >> 8)); return (int)(e & 0xFFu); }
    int len = 9;
    int code = (int)b.peek(9);
    while (len <= 16 && code > h.maxcode[len]) { ++len; if (len <= 16) code = (int)b.peek(len); }
    if (len > 16) return -1;
    b.drop(len);
    return h.vals[(code + h.valoff[len]) & 0xFF];
}
// s bits, 0 <= s <= 15, as the signed value they stand for (F.2.2.1 EXTEND)
template <class Bits>
MI355_HD int jpeg_dec_receive(Bits& b, int s) {
    if (!s) return 0;
    const int v = (int)b.peek(s);
    b.drop(s);
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// One restart segment: MCUs [mcu0, mcu0 + nmcu) of frame f from the bytes [begin, end) of its scan.  Non-zero coefficients go to
// coef (zeroed by the caller); -> status.  Every loop is bounded: nmcu MCUs of bpm blocks of at most 63 symbols behind the DC.
template <class Fetch>
MI355_HD int jpeg_dec_segment(const JpegDecFrame& f, const JpegHuff* huff, Fetch fetch, uint32_t begin, uint32_t end, long long mcu0, int nmcu,
                              int16_t* coef) {
    JpegBits<Fetch> b{fetch, begin, end};
    uint32_t pred[3] = {0u, 0u, 0u};
    const int ny = f.ncomp == 1 ? 1 : f.hs * f.vs;
    for (int m = 0; m < nmcu; ++m) {
        for (int j = 0; j < f.bpm; ++j) {
            const int c = j < ny ? 0 : j - ny + 1;
            int16_t* zz = coef + ((mcu0 + m) * f.bpm + j) * 64;
            const JpegHuff& hd = huff[f.dc_tab[c]];
            const JpegHuff& ha = huff[2 + f.ac_tab[c]];
            b.fill();
            int s = jpeg_dec_symbol(b, hd);
            if (s < 0) return kJpegDecCodeNotFound;
            pred[c] += (uint32_t)jpeg_dec_receive(b, s & 15);            // the parser admits DC symbols 0 .. 15 only
            const int16_t dc = (int16_t)(uint16_t)pred[c];
            if (dc) zz[0] = dc;
            for (int k = 1; k < 64;) {
                b.fill();
                s = jpeg_dec_symbol(b, ha);
                if (s < 0) return kJpegDecCodeNotFound;
                const int r = s >> 4;
                s &= 15;
                if (!s) {
                    if (r != 15) break;                                  // EOB
                    k += 16;                                             // ZRL
                    if (k > 64) return kJpegDecRunPastBlock;
                    continue;
                }
                k += r;
                if (k > 63) return kJpegDecRunPastBlock;
                const int v = jpeg_dec_receive(b, s);
                if (v) zz[k] = (int16_t)v;
                ++k;
            }
        }
    }
    if (b.pad * 8 > b.n) return kJpegDecSegmentShort;                    // bits behind the segment's end were consumed
    if (b.pos < b.end || b.n - b.pad * 8 >= 8) return kJpegDecSegmentLong;
    return kJpegDecOk;
}

// ---- dequantisation and IDCT ---------------------------------------------------------------------------------------------------------------
// One 8-point pass of jpeg_idct_islow on T = int (blocks within kJpegIdctNarrowSum) or long long; n = 11 (columns), 18 (rows)
template <class T>
MI355_HD void jpeg_idct_1d(T (&v)[8], int n) {
    T z1 = (v[2] + v[6]) * 4433;
    const T t2 = z1 - v[6] * 15137, t3 = z1 + v[2] * 6270;
    const T t0 = (v[0] + v[4]) * 8192, t1 = (v[0] - v[4]) * 8192;
    const T t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    T a0 = v[7], a1 = v[5], a2 = v[3], a3 = v[1];
    z1 = a0 + a3;
    T z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const T z5 = (z3 + z4) * 9633;
    a0 *= 2446; a1 *= 16819; a2 *= 25172; a3 *= 12299;
    z1 *= -7373; z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
    const T h = (T)1 << (n - 1);
    v[0] = (t10 + a3 + h) >> n; v[7] = (t10 - a3 + h) >> n;
    v[1] = (t11 + a2 + h) >> n; v[6] = (t11 - a2 + h) >> n;
    v[2] = (t12 + a1 + h) >> n; v[5] = (t12 - a1 + h) >> n;
    v[3] = (t13 + a0 + h) >> n; v[4] = (t13 - a0 + h) >> n;
}
// the same with the width chosen by the block's own bound; the values between the passes fit 32 bits either way
MI355_HD void jpeg_idct_pass(int (&v)[8], int n, bool narrow) {
    if (narrow) { jpeg_idct_1d(v, n); return; }
    long long w[8];
    for (int k = 0; k < 8; ++k) w[k] = v[k];
    jpeg_idct_1d(w, n);
    for (int k = 0; k < 8; ++k) v[k] = (int)w[k];
}
MI355_HD int jpeg_clamp255(int x) { return x < 0 ? 0 : x > 255 ? 255 : x; }

// ---- upsampling and colour -------------------------------------------------------------------------------------------------------------------
// chroma sample of output pixel (x, y) from plane p (row length pw, real extent cw x ch), Y sampled hs x vs
MI355_HD int jpeg_dec_chroma(const uint8_t* p, int pw, int cw, int ch, int hs, int vs, int x, int y) {
    if (hs == 1) return p[(size_t)y * pw + x];
    const int cx = x >> 1;
    if (cw <= 2) return p[(size_t)(vs == 2 ? y >> 1 : y) * pw + cx];
    const int nx = x & 1 ? jpeg_min(cx + 1, cw - 1) : (cx > 0 ? cx - 1 : 0);
    if (vs == 1) {
        const uint8_t* r = p + (size_t)y * pw;
        return (3 * r[cx] + r[nx] + (x & 1 ? 2 : 1)) >> 2;
    }
    const int cy = y >> 1, fy = y & 1 ? jpeg_min(cy + 1, ch - 1) : (cy > 0 ? cy - 1 : 0);
    const uint8_t* r = p + (size_t)cy * pw;
    const uint8_t* q = p + (size_t)fy * pw;
    const int s = 3 * r[cx] + q[cx], sn = 3 * r[nx] + q[nx];
    return (3 * s + sn + (x & 1 ? 7 : 8)) >> 4;
}
MI355_HD void jpeg_dec_bgr(int y, int cb, int cr, int& b, int& g, int& r) {
    cb -= 128; cr -= 128;
    r = jpeg_clamp255(y + ((91881 * cr + 32768) >> 16));
    g = jpeg_clamp255(y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    b = jpeg_clamp255(y + ((116130 * cb + 32768) >> 16));
}
// pixel (x, y) of frame f from its planes
MI355_HD void jpeg_dec_pixel(const JpegDecFrame& f, int x, int y, int& b, int& g, int& r) {
    const int yy = f.plane[0][(size_t)y * f.pw[0] + x];
    if (f.ncomp == 1) { b = g = r = yy; return; }
    jpeg_dec_bgr(yy, jpeg_dec_chroma(f.plane[1], f.pw[1], f.cw, f.ch, f.hs, f.vs, x, y),
                 jpeg_dec_chroma(f.plane[2], f.pw[2], f.cw, f.ch, f.hs, f.vs, x, y), b, g, r);
}
// where block j of MCU (mx, my) lies: component, and its top-left sample in that component's plane
MI355_HD void jpeg_dec_block_place(const JpegDecFrame& f, int mx, int my, int j, int& c, int& x0, int& y0) {
    const int ny = f.ncomp == 1 ? 1 : f.hs * f.vs;
    if (j < ny) { c = 0; x0 = (mx * f.hs + j % f.hs) * 8; y0 = (my * f.vs + j / f.hs) * 8; }
    else { c = j - ny + 1; x0 = mx * 8; y0 = my * 8; }
}

// ---- the parser ------------------------------------------------------------------------------------------------------------------------------
struct JpegParsed {
    JpegDecFrame f{};
    JpegHuff huff[4];
    long long scan_begin = 0, scan_end = 0;     // within the stream
    std::vector<uint32_t> seg;                  // f.nseg pairs, relative to scan_begin
};

// BITS and HUFFVAL -> the decoder's table; false when the code lengths do not form a prefix code
inline bool jpeg_dec_make_huff(const uint8_t* bits, const uint8_t* vals, int nvals, JpegHuff& h) {
    std::memset(&h, 0, sizeof h);
    for (int i = 0; i < nvals; ++i) h.vals[i] = vals[i];
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        h.valoff[l] = k - code;
        for (int i = 0; i < bits[l - 1]; ++i, ++k, ++code) {
            if (code >= (1 << l)) return false;
            if (l <= 8)
                for (int fillv = 0; fillv < (1 << (8 - l)); ++fillv) h.look[(code << (8 - l)) | fillv] = (uint16_t)(l << 8 | vals[k]);
        }
        h.maxcode[l] = bits[l - 1] ? code - 1 : -1;
        code <<= 1;
    }
    return true;
}

// The whole header and the scan's extent.  false: `why` says what is refused.  Nothing of the stream is decoded here.
inline bool jpeg_dec_parse(const uint8_t* d, long long len, JpegParsed& P, std::string& why) {
    auto no = [&](const std::string& m) { why = m; return false; };
    if (!d || len < 4 || d[0] != 0xFF || d[1] != 0xD8) return no("not a JPEG stream (no SOI)");
    if (len >= (1ll << 31)) return no("a stream must be smaller than 2 GiB");
    uint8_t qt[4][64]; bool have_q[4] = {false, false, false, false}, have_h[4] = {false, false, false, false}, have_sof = false;
    int comp_id[3] = {0, 0, 0}, comp_h[3] = {1, 1, 1}, comp_v[3] = {1, 1, 1}, comp_q[3] = {0, 0, 0};
    JpegDecFrame& f = P.f;
    long long p = 2;
    for (;;) {
        if (p + 4 > len) return no("no SOS before the stream ends");
        if (d[p] != 0xFF) return no("a marker is expected at byte " + std::to_string(p));
        const int m = d[p + 1];
        if (m == 0xFF) { ++p; continue; }                                // fill byte in front of a marker
        if (m == 0xD9) return no("EOI before any scan");
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) return no("marker 0x" + std::to_string(m) + " outside a scan");
        const long long L = (long long)d[p + 2] << 8 | d[p + 3];
        if (L < 2 || p + 2 + L > len) return no("a marker segment runs past the stream's end");
        const uint8_t* s = d + p + 4;
        const long long n = L - 2;
        if (m == 0xC0) {
            if (have_sof) return no("several frame headers");
            if (n < 6) return no("SOF0 too short");
            if (s[0] != 8) return no(std::to_string(s[0]) + "-bit precision (8-bit only)");
            f.H = s[1] << 8 | s[2]; f.W = s[3] << 8 | s[4]; f.ncomp = s[5];
            if (f.H == 0) return no("height 0: the stream defines its height by DNL, which is not accepted");
            if (f.W == 0) return no("width 0");
            if (f.ncomp != 1 && f.ncomp != 3) return no(std::to_string(f.ncomp) + " components (1 or 3 only)");
            if (n < 6 + 3 * f.ncomp) return no("SOF0 too short");
            for (int c = 0; c < f.ncomp; ++c) {
                comp_id[c] = s[6 + 3 * c]; comp_h[c] = s[7 + 3 * c] >> 4; comp_v[c] = s[7 + 3 * c] & 15; comp_q[c] = s[8 + 3 * c];
                if (comp_q[c] > 3) return no("quantisation table id " + std::to_string(comp_q[c]));
            }
            have_sof = true;
        } else if (m >= 0xC1 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {
            static const char* kinds[16] = {"", "SOF1 (extended sequential)", "SOF2 (progressive)", "SOF3 (lossless)", "", "SOF5 (differential)",
                                            "SOF6 (differential progressive)", "SOF7 (differential lossless)", "", "SOF9 (arithmetic coding)",
                                            "SOF10 (arithmetic coding, progressive)", "SOF11 (arithmetic coding, lossless)", "",
                                            "SOF13 (arithmetic coding)", "SOF14 (arithmetic coding)", "SOF15 (arithmetic coding)"};
            return no(std::string(kinds[m - 0xC0]) + ": baseline SOF0 only");
        } else if (m == 0xCC) {
            return no("DAC: arithmetic coding is not accepted");
        } else if (m == 0xDC) {
            return no("DNL is not accepted");
        } else if (m == 0xDB) {
            for (long long i = 0; i < n;) {
                const int pq = s[i] >> 4, id = s[i] & 15;
                if (pq != 0) return no("16-bit quantisation steps");
                if (id > 3) return no("quantisation table id " + std::to_string(id));
                if (i + 65 > n) return no("DQT too short");
                std::memcpy(qt[id], s + i + 1, 64);
                for (int k = 0; k < 64; ++k) if (!qt[id][k]) return no("a quantisation step of 0");
                have_q[id] = true;
                i += 65;
            }
        } else if (m == 0xC4) {
            for (long long i = 0; i < n;) {
                const int cls = s[i] >> 4, id = s[i] & 15;
                if (cls > 1 || id > 1) return no("Huffman table class " + std::to_string(cls) + " id " + std::to_string(id) + " (baseline: ids 0 and 1)");
                if (i + 17 > n) return no("DHT too short");
                int cnt = 0;
                for (int l = 0; l < 16; ++l) cnt += s[i + 1 + l];
                if (cnt > 256 || i + 17 + cnt > n) return no("DHT too short");
                if (!jpeg_dec_make_huff(s + i + 1, s + i + 17, cnt, P.huff[cls * 2 + id])) return no("a Huffman table whose lengths form no prefix code");
                if (cls == 0) for (int k = 0; k < cnt; ++k) if (s[i + 17 + k] > 15) return no("a DC Huffman table with a category above 15");
                have_h[cls * 2 + id] = true;
                i += 17 + cnt;
            }
        } else if (m == 0xDD) {
            if (n < 2) return no("DRI too short");
            f.ri = s[0] << 8 | s[1];
        } else if (m == 0xDA) {
            if (!have_sof) return no("SOS before SOF0");
            if (n < 1 || s[0] != f.ncomp) return no("several scans (the scan holds " + std::to_string(n < 1 ? 0 : s[0]) + " of " + std::to_string(f.ncomp) + " components)");
            if (n < 4 + 2 * f.ncomp) return no("SOS too short");
            for (int c = 0; c < f.ncomp; ++c) {
                if (s[1 + 2 * c] != comp_id[c]) return no("the scan's components are not in the frame's order");
                const int td = s[2 + 2 * c] >> 4, ta = s[2 + 2 * c] & 15;
                if (td > 1 || ta > 1) return no("Huffman table id above 1");
                if (!have_h[td]) return no("missing DC Huffman table " + std::to_string(td));
                if (!have_h[2 + ta]) return no("missing AC Huffman table " + std::to_string(ta));
                if (!have_q[comp_q[c]]) return no("missing quantisation table " + std::to_string(comp_q[c]));
                f.dc_tab[c] = (uint8_t)td; f.ac_tab[c] = (uint8_t)ta;
                std::memcpy(f.q[c], qt[comp_q[c]], 64);
            }
            const uint8_t* t = s + 1 + 2 * f.ncomp;
            if (t[0] != 0 || t[1] != 63 || t[2] != 0) return no("a progressive scan (spectral selection or successive approximation)");
            p += 2 + L;
            break;
        }                                                                // APPn, COM and the rest: skipped
        p += 2 + L;
    }
    if (f.ncomp == 1) { f.hs = f.vs = 1; }
    else {
        f.hs = comp_h[0]; f.vs = comp_v[0];
        const bool ok = comp_h[1] == 1 && comp_v[1] == 1 && comp_h[2] == 1 && comp_v[2] == 1 &&
                        ((f.hs == 1 && f.vs == 1) || (f.hs == 2 && f.vs == 1) || (f.hs == 2 && f.vs == 2));
        if (!ok) return no("sampling factors " + std::to_string(comp_h[0]) + "x" + std::to_string(comp_v[0]) + ", " + std::to_string(comp_h[1]) + "x" +
                           std::to_string(comp_v[1]) + ", " + std::to_string(comp_h[2]) + "x" + std::to_string(comp_v[2]) + " (4:4:4, 4:2:2 and 4:2:0 only)");
    }
    if (3ll * f.H * f.W >= (1ll << 31)) return no("a decoded frame must be smaller than 2 GiB");
    f.bpm = f.ncomp == 1 ? 1 : f.hs * f.vs + 2;
    f.mcus_x = (f.W + 8 * f.hs - 1) / (8 * f.hs); f.mcus_y = (f.H + 8 * f.vs - 1) / (8 * f.vs);
    f.cw = (f.W + f.hs - 1) / f.hs; f.ch = (f.H + f.vs - 1) / f.vs;
    const long long mcus = (long long)f.mcus_x * f.mcus_y;
    f.seg_mcus = f.ri ? f.ri : (int)mcus;
    f.nseg = (int)((mcus + f.seg_mcus - 1) / f.seg_mcus);
    // the scan: cut at RSTm; it ends at EOI
    P.scan_begin = p;
    P.seg.clear(); P.seg.reserve((size_t)f.nseg * 2);
    long long at = p, begin = p;
    int rst = 0;
    for (;;) {
        const uint8_t* q = at < len ? (const uint8_t*)std::memchr(d + at, 0xFF, (size_t)(len - at)) : nullptr;
        if (!q || q + 1 >= d + len) return no("no EOI");
        at = q - d;
        const int m = d[at + 1];
        if (m == 0) { at += 2; continue; }
        if (m >= 0xD0 && m <= 0xD7) {
            if (!f.ri) return no("a restart marker in a stream without a restart interval");
            if (m != 0xD0 + (rst & 7)) return no("RST" + std::to_string(m - 0xD0) + " out of sequence (RST" + std::to_string(rst & 7) + " expected)");
            if (rst + 1 >= f.nseg) return no("more restart markers than the restart interval gives");
            P.seg.push_back((uint32_t)(begin - p)); P.seg.push_back((uint32_t)(at - p));
            ++rst; at += 2; begin = at;
            continue;
        }
        if (m == 0xD9) break;
        if (m == 0xDC) return no("DNL is not accepted");
        if (m == 0xDA || m == 0xC4 || m == 0xDB || m == 0xDD) return no("several scans");
        return no("marker 0x" + std::string(1, "0123456789ABCDEF"[m >> 4]) + std::string(1, "0123456789ABCDEF"[m & 15]) + " inside the scan");
    }
    P.seg.push_back((uint32_t)(begin - p)); P.seg.push_back((uint32_t)(at - p));
    if (rst + 1 != f.nseg) return no(std::to_string(rst) + " restart markers where the restart interval gives " + std::to_string(f.nseg - 1));
    P.scan_end = at;
    return true;
}

// ---- host twin ---------------------------------------------------------------------------------------------------------------------------------
// the entropy stage of one parsed stream into coef (jpeg_dec_blocks x 64, zeroed here) -> status (of the first segment that fails)
inline int jpeg_dec_coefficients_host(const JpegParsed& P, const uint8_t* data, int16_t* coef) {
    const JpegDecFrame& f = P.f;
    std::memset(coef, 0, (size_t)jpeg_dec_blocks(f) * 128);
    const long long mcus = (long long)f.mcus_x * f.mcus_y;
    for (int s = 0; s < f.nseg; ++s) {
        const long long mcu0 = (long long)s * f.seg_mcus;
        const int nm = (int)(mcus - mcu0 < f.seg_mcus ? mcus - mcu0 : f.seg_mcus);
        const int st = jpeg_dec_segment(f, P.huff, JpegFetchBytes{data + P.scan_begin}, P.seg[2 * s], P.seg[2 * s + 1], mcu0, nm, coef);
        if (st) return st;
    }
    return kJpegDecOk;
}
// one block: coefficients -> 64 samples (natural order)
inline void jpeg_dec_block_host(const int16_t* zz, const uint8_t* q, uint8_t* out64) {
    int blk[64];
    long long sum = 0;
    for (int k = 0; k < 64; ++k) { const int v = (int)zz[k] * q[k]; blk[kJpegZigzag[k]] = v; sum += v < 0 ? -(long long)v : v; }
    const bool narrow = sum <= kJpegIdctNarrowSum;
    for (int pass = 0; pass < 2; ++pass)
        for (int i = 0; i < 8; ++i) {
            const int at = pass ? i * 8 : i, step = pass ? 1 : 8;
            int v[8];
            for (int k = 0; k < 8; ++k) v[k] = blk[at + k * step];
            jpeg_idct_pass(v, pass ? 18 : 11, narrow);
            for (int k = 0; k < 8; ++k) blk[at + k * step] = v[k];
        }
    for (int k = 0; k < 64; ++k) out64[k] = (uint8_t)jpeg_clamp255(blk[k] + 128);
}
// coefficients -> BGR [H][pitch]
inline void jpeg_dec_pixels_host(const JpegParsed& P, const int16_t* coef, uint8_t* out, int pitch) {
    JpegDecFrame f = P.f;
    std::vector<uint8_t> planes[3];
    for (int c = 0; c < f.ncomp; ++c) {
        f.pw[c] = f.mcus_x * 8 * (c ? 1 : f.hs); f.ph[c] = f.mcus_y * 8 * (c ? 1 : f.vs);
        planes[c].resize((size_t)f.pw[c] * f.ph[c]);
        f.plane[c] = planes[c].data();
    }
    uint8_t px[64];
    for (int my = 0; my < f.mcus_y; ++my)
        for (int mx = 0; mx < f.mcus_x; ++mx)
            for (int j = 0; j < f.bpm; ++j) {
                int c, x0, y0;
                jpeg_dec_block_place(f, mx, my, j, c, x0, y0);
                jpeg_dec_block_host(coef + (((size_t)my * f.mcus_x + mx) * f.bpm + j) * 64, f.q[c], px);
                for (int r = 0; r < 8; ++r) std::memcpy(f.plane[c] + (size_t)(y0 + r) * f.pw[c] + x0, px + r * 8, 8);
            }
    for (int y = 0; y < f.H; ++y)
        for (int x = 0; x < f.W; ++x) {
            int b, g, r;
            jpeg_dec_pixel(f, x, y, b, g, r);
            uint8_t* o = out + (size_t)y * pitch + (size_t)x * 3;
            o[0] = (uint8_t)b; o[1] = (uint8_t)g; o[2] = (uint8_t)r;
        }
}

// ---- one call (jpeg_decode_host.cpp; the GPU half is jpeg_decode_kernels.hip's) -------------------------------------------------------------
struct JpegDecCtx;                              // the GPU path's grow-only scratch (engine_internal.h); NULL: scratch of the call's own
// parses and checks everything, then runs the twin (device -1) or the GPU.  outs: BGR destinations, or NULL with coefs: the entropy
// stage alone into host int16 [blocks][64].  lanes[i]: 0 host, 1 a lane per segment, 2 sync.  sync: the hook's, NULL for product calls
int jpeg_dec_call(JpegDecCtx* ctx, int device, mi355_jpeg_stream* streams, int n, int entropy, const mi355_render_out* outs,
                  int16_t* const* coefs, int* status, void* stream, float* launch_ms, const JpegSyncOpts* sync = nullptr);
int jpeg_dec_run_gpu(JpegDecCtx* ctx, int device, std::vector<JpegParsed>& P, const mi355_jpeg_stream* streams, int n, const int* lanes,
                     const mi355_render_out* outs, int16_t* const* coefs, int* status, void* stream, float* launch_ms, const JpegSyncOpts& sync);

}  // namespace mi355
