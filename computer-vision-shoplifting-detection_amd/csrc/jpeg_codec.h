// JPEG evidence frames (include/mi355_yolo.h "jpeg"): the codec's rules, stated once for the kernels (jpeg_kernels.hip)
// and their host twin.  Integers only: colour conversion, chroma averaging, the forward DCT, quantisation and the entropy coder give the
// same numbers on both targets, so the two streams are the same bytes.
//
// The stream: baseline sequential DCT, JFIF 1.01, 8 bits, Y Cb Cr, 4:2:0 (Y 2x2, 16 x 16 MCUs) or 4:4:4 (8 x 8 MCUs); the Annex K.1 / K.2
// quantisation tables scaled by the IJG quality rule; the four Annex K.3 Huffman tables; a restart interval of ONE MCU ROW, so every MCU
// row is a segment of its own (DC predictors 0, last byte padded with 1-bits, RSTm with m = row mod 8 between segments).
//   colour   Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
//            Cb = (-11059 R - 21709 G + 32768 B + 8421375) >> 16          8421375 = 128 * 65536 + 32767
//            Cr = ( 32768 R - 27439 G -  5329 B + 8421375) >> 16          (arithmetic shift; all three land in 0 .. 255 without a clamp)
//   extent   pixel (x, y) of the padded frame = pixel (min(x, W - 1), min(y, H - 1)) of the frame
//   4:2:0    chroma sample (x, y) = (c(2x, 2y) + c(2x + 1, 2y) + c(2x, 2y + 1) + c(2x + 1, 2y + 1) + 2) >> 2 of the padded frame's Cb / Cr
//   shift    sample - 128
//   DCT      the Loeffler-Ligtenberg-Moschytz factorisation in 13-bit fixed point (jpeg_fdct_1d below), rows first with 2 extra bits
//            kept, then columns; the result is 8 x the DCT coefficient
//   quant    q8 = 8 q;  |c| -> (|c| + q8 / 2) / q8, sign restored: round half away from zero
//   order    zigzag
#pragma once
#include <stdint.h>

#ifndef MI355_HD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MI355_HD __host__ __device__ __forceinline__
#else
#define MI355_HD inline
#endif
#endif

namespace mi355 {

constexpr int kJpeg420 = 420, kJpeg444 = 444;
constexpr int kJpegMaxSide = 65535;
constexpr int kJpegHeaderMax = 640;             // SOI .. SOS is 629 bytes
// the longest coding of one 8 x 8 block: a DC difference of category 11 behind the longest DC code (11 bits, chroma) and 63 AC
// coefficients of category 10 each behind a 16-bit code
constexpr int kJpegBlockBits = (11 + 11) + 63 * (16 + 10);      // 1660
constexpr int kJpegBlockBytes = (kJpegBlockBits + 7) / 8;       // 208 unstuffed; every byte can be 0xFF and take a 0x00 behind it

// natural index of the k-th coefficient in zigzag order
constexpr uint8_t kJpegZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// Annex K.1 (luminance) and K.2 (chrominance), in zigzag order as a DQT segment carries them
constexpr uint8_t kJpegBaseQ[2][64] = {
    {16, 11, 12, 14, 12, 10, 16, 14, 13, 14, 18, 17, 16, 19, 24, 40, 26, 24, 22, 22, 24, 49, 35, 37, 29, 40, 58, 51, 61, 60, 57, 51,
     56, 55, 64, 72, 92, 78, 64, 68, 87, 69, 55, 56, 80, 109, 81, 87, 95, 98, 103, 104, 103, 62, 77, 113, 121, 112, 100, 120, 92, 101, 103, 99},
    {17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
// Annex K.3: BITS (codes per length 1 .. 16) and HUFFVAL of the DC tables (luminance, chrominance) ...
constexpr uint8_t kJpegDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t kJpegDcVal[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
// ... and of the AC tables
constexpr uint8_t kJpegAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
constexpr uint8_t kJpegAcVal[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1,
     0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA,
     0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6,
     0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9,
     0xFA},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19,
     0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8,
     0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4,
     0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9,
     0xFA}};

// What a call's kernels read besides the pixels, built on the host (jpeg_make_tables) and uploaded with the descriptors: a device
// function cannot index the constexpr arrays above at run time.  Table 0 serves Y, table 1 Cb and Cr.
struct JpegTables {
    uint16_t q[2][64];                          // quantisation steps in zigzag order, 1 .. 255
    uint8_t zigzag[64];
    uint16_t dc_code[2][12], ac_code[2][256];   // code of a symbol, right-aligned ...
    uint8_t dc_len[2][12], ac_len[2][256];      // ... and its length in bits (0: the table has no such symbol)
};

// One frame of a call.  Scratch and output pointers are the GPU path's; the host twin takes src, the geometry and `out`.
struct JpegFrame {
    const uint8_t* src; int H, W, pitch;        // BGR
    int mcu, mcus_x, mcus_y, bpm;               // MCU side (16 | 8), MCUs per row (= the restart interval) and rows, blocks per MCU (6 | 3)
    int hdr_len;
    const uint8_t* hdr;                         // SOI .. SOS
    int16_t* coef;                              // [mcus_y][mcus_x][bpm][64] quantised coefficients, zigzag order, blocks in scan order
    uint32_t* seg_words; size_t seg_cap_words;  // per MCU row: its entropy-coded bits before stuffing, big-endian 32-bit words
    uint32_t* seg_info;                         // per MCU row: {bytes before stuffing, how many of them are 0xFF}
    uint8_t* out; long long* len;               // the stream and its length
};

MI355_HD int jpeg_min(int a, int b) { return a < b ? a : b; }

inline void jpeg_geometry(JpegFrame& f, int subsampling) {
    f.mcu = subsampling == kJpeg420 ? 16 : 8; f.bpm = subsampling == kJpeg420 ? 6 : 3;
    f.mcus_x = (f.W + f.mcu - 1) / f.mcu; f.mcus_y = (f.H + f.mcu - 1) / f.mcu;
}
// Capacity: no stream of an H x W frame is longer than this, whatever the pixels and the quality
inline long long jpeg_bound(int H, int W, int subsampling) {
    JpegFrame f{}; f.H = H; f.W = W; jpeg_geometry(f, subsampling);
    const long long blocks = (long long)f.mcus_x * f.mcus_y * f.bpm;
    return kJpegHeaderMax + blocks * 2 * kJpegBlockBytes + 2ll * f.mcus_y + 2;
}

inline int jpeg_quality_scale(int quality) { return quality < 50 ? 5000 / quality : 200 - 2 * quality; }

inline void jpeg_huff_codes(const uint8_t* bits, const uint8_t* vals, uint16_t* code, uint8_t* len, int nsym) {
    for (int i = 0; i < nsym; ++i) { code[i] = 0; len[i] = 0; }
    unsigned c = 0; int k = 0;
    for (int l = 1; l <= 16; ++l) {                      // Annex C: codes of one length count up, and double when the length grows
        for (int i = 0; i < bits[l - 1]; ++i, ++k) { code[vals[k]] = (uint16_t)c++; len[vals[k]] = (uint8_t)l; }
        c <<= 1;
    }
}
inline void jpeg_make_tables(int quality, JpegTables& t) {
    const int s = jpeg_quality_scale(quality);
    for (int c = 0; c < 2; ++c) {
        for (int k = 0; k < 64; ++k) {
            int v = (kJpegBaseQ[c][k] * s + 50) / 100;
            t.q[c][k] = (uint16_t)(v < 1 ? 1 : v > 255 ? 255 : v);
        }
        jpeg_huff_codes(kJpegDcBits[c], kJpegDcVal, t.dc_code[c], t.dc_len[c], 12);
        jpeg_huff_codes(kJpegAcBits[c], kJpegAcVal[c], t.ac_code[c], t.ac_len[c], 256);
    }
    for (int k = 0; k < 64; ++k) t.zigzag[k] = kJpegZigzag[k];
}

// SOI, APP0, DQT x 2, SOF0, DHT x 4, DRI, SOS -> bytes written (<= kJpegHeaderMax)
inline int jpeg_write_header(const JpegTables& t, const JpegFrame& f, uint8_t* o) {
    uint8_t* p = o;
    auto b = [&](int v) { *p++ = (uint8_t)v; };
    auto w = [&](int v) { *p++ = (uint8_t)(v >> 8); *p++ = (uint8_t)v; };
    w(0xFFD8);
    w(0xFFE0); w(16); b('J'); b('F'); b('I'); b('F'); b(0); w(0x0101); b(0); w(1); w(1); b(0); b(0);
    for (int c = 0; c < 2; ++c) { w(0xFFDB); w(67); b(c); for (int k = 0; k < 64; ++k) b(t.q[c][k]); }
    w(0xFFC0); w(17); b(8); w(f.H); w(f.W); b(3);
    b(1); b(f.bpm == 6 ? 0x22 : 0x11); b(0); b(2); b(0x11); b(1); b(3); b(0x11); b(1);
    for (int c = 0; c < 2; ++c) {
        w(0xFFC4); w(19 + 12); b(c); for (int i = 0; i < 16; ++i) b(kJpegDcBits[c][i]); for (int i = 0; i < 12; ++i) b(kJpegDcVal[i]);
        w(0xFFC4); w(19 + 162); b(0x10 | c); for (int i = 0; i < 16; ++i) b(kJpegAcBits[c][i]); for (int i = 0; i < 162; ++i) b(kJpegAcVal[c][i]);
    }
    w(0xFFDD); w(4); w(f.mcus_x);
    w(0xFFDA); w(12); b(3); b(1); b(0x00); b(2); b(0x11); b(3); b(0x11); b(0); b(63); b(0);
    return (int)(p - o);
}

MI355_HD void jpeg_ycc(int b, int g, int r, int& y, int& cb, int& cr) {
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    cb = (-11059 * r - 21709 * g + 32768 * b + 8421375) >> 16;
    cr = (32768 * r - 27439 * g - 5329 * b + 8421375) >> 16;
}

// One 8-point pass of the forward DCT.  pass 0 (rows): the even outputs keep 2 extra bits, the odd ones are brought down from 13 to 2;
// pass 1 (columns): the 2 bits go and the 13 with them.  After both passes v holds 8 x the coefficient.  Shifts are arithmetic and
// round to nearest, halves up: (x + (1 << (n - 1))) >> n.  |v| stays below 2^16 and every product below 2^31.
MI355_HD void jpeg_fdct_1d(int (&v)[8], int pass) {
    const int t0 = v[0] + v[7], t7 = v[0] - v[7], t1 = v[1] + v[6], t6 = v[1] - v[6];
    const int t2 = v[2] + v[5], t5 = v[2] - v[5], t3 = v[3] + v[4], t4 = v[3] - v[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    const int n = pass ? 15 : 11, h = 1 << (n - 1);
    if (pass) { v[0] = (t10 + t11 + 2) >> 2; v[4] = (t10 - t11 + 2) >> 2; }
    else { v[0] = (t10 + t11) * 4; v[4] = (t10 - t11) * 4; }
    const int z1 = (t12 + t13) * 4433;                   // 0.541196100 * 2^13
    v[2] = (z1 + t13 * 6270 + h) >> n;                   // 0.765366865
    v[6] = (z1 - t12 * 15137 + h) >> n;                  // 1.847759065
    const int z5 = (t4 + t6 + t5 + t7) * 9633;           // 1.175875602
    const int a1 = (t4 + t7) * -7373;                    // 0.899976223
    const int a2 = (t5 + t6) * -20995;                   // 2.562915447
    const int a3 = (t4 + t6) * -16069 + z5;              // 1.961570560
    const int a4 = (t5 + t7) * -3196 + z5;               // 0.390180644
    v[7] = (t4 * 2446 + a1 + a3 + h) >> n;               // 0.298631336
    v[5] = (t5 * 16819 + a2 + a4 + h) >> n;              // 2.053119869
    v[3] = (t6 * 25172 + a2 + a3 + h) >> n;              // 3.072711026
    v[1] = (t7 * 12299 + a1 + a4 + h) >> n;              // 1.501321110
}

// c = 8 x a coefficient, q = the table's step
MI355_HD int jpeg_quant(int c, int q) {
    const int q8 = q * 8, a = c < 0 ? -c : c, r = (a + (q8 >> 1)) / q8;
    return c < 0 ? -r : r;
}

// bits of |v|: the magnitude category of a DC difference or an AC coefficient
MI355_HD int jpeg_category(int v) {
    const unsigned a = (unsigned)(v < 0 ? -v : v);
    return a ? 32 - __builtin_clz(a) : 0;
}

// The entropy coding of one block: zz = 64 coefficients in zigzag order, pred = the DC of the component's previous block in the
// segment (0 for the first), the component's four table rows.  Every code goes to sink.put(bits, length) with its magnitude bits
// appended, 26 bits at most: DC (code of the category, then the difference's low bits, a negative difference minus one);
// per non-zero AC coefficient one ZRL (0xF0) per 16 zeros before it, then (run << 4 | category) and its bits; EOB (0x00) when the
// block ends in zeros, nothing when coefficient 63 is not zero.
template <class Sink>
MI355_HD void jpeg_code_block(const int16_t* zz, int pred, const uint16_t* dcc, const uint8_t* dcl, const uint16_t* acc, const uint8_t* acl, Sink& s) {
    int d = (int)zz[0] - pred;
    int n = jpeg_category(d);
    unsigned m = (unsigned)(d < 0 ? d - 1 : d) & ((1u << n) - 1u);
    s.put(((unsigned)dcc[n] << n) | m, dcl[n] + n);
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        int v = zz[k];
        if (v == 0) { ++run; continue; }
        v = v > 1023 ? 1023 : v < -1023 ? -1023 : v;     // cannot trigger for 8-bit samples (an AC coefficient stays below 1024); keeps the symbol in the table
        for (; run >= 16; run -= 16) s.put(acc[0xF0], acl[0xF0]);
        n = jpeg_category(v);
        m = (unsigned)(v < 0 ? v - 1 : v) & ((1u << n) - 1u);
        const int sym = run << 4 | n;
        s.put(((unsigned)acc[sym] << n) | m, acl[sym] + n);
        run = 0;
    }
    if (run) s.put(acc[0], acl[0]);
}

// ---- host twin -----------------------------------------------------------------------------------------------------------------------
// component c (0 Y, 1 Cb, 2 Cr) of pixel (x, y) of the padded frame
inline int jpeg_pixel_host(const JpegFrame& f, int c, int x, int y) {
    const uint8_t* p = f.src + (size_t)jpeg_min(y, f.H - 1) * f.pitch + (size_t)jpeg_min(x, f.W - 1) * 3;
    int v[3];
    jpeg_ycc(p[0], p[1], p[2], v[0], v[1], v[2]);
    return v[c];
}
// block j of MCU (mx, my): level-shifted samples -> 64 quantised coefficients in zigzag order
inline void jpeg_block_host(const JpegFrame& f, const JpegTables& t, int mx, int my, int j, int16_t* zz) {
    int blk[64];
    const bool sub = f.bpm == 6;
    const int c = sub ? (j < 4 ? 0 : j - 3) : j;
    for (int r = 0; r < 8; ++r)
        for (int x = 0; x < 8; ++x) {
            int s;
            if (sub && c) {
                const int px = mx * 16 + 2 * x, py = my * 16 + 2 * r;
                s = (jpeg_pixel_host(f, c, px, py) + jpeg_pixel_host(f, c, px + 1, py) + jpeg_pixel_host(f, c, px, py + 1) + jpeg_pixel_host(f, c, px + 1, py + 1) + 2) >> 2;
            } else if (sub) s = jpeg_pixel_host(f, 0, mx * 16 + (j & 1) * 8 + x, my * 16 + (j >> 1) * 8 + r);
            else s = jpeg_pixel_host(f, c, mx * 8 + x, my * 8 + r);
            blk[r * 8 + x] = s - 128;
        }
    for (int pass = 0; pass < 2; ++pass)
        for (int i = 0; i < 8; ++i) {
            const int at = pass ? i : i * 8, step = pass ? 8 : 1;
            int v[8];
            for (int k = 0; k < 8; ++k) v[k] = blk[at + k * step];
            jpeg_fdct_1d(v, pass);
            for (int k = 0; k < 8; ++k) blk[at + k * step] = v[k];
        }
    for (int k = 0; k < 64; ++k) zz[k] = (int16_t)jpeg_quant(blk[t.zigzag[k]], t.q[c ? 1 : 0][k]);
}
inline void jpeg_coefficients_host(const JpegFrame& f, const JpegTables& t, int16_t* coef) {
    for (int my = 0; my < f.mcus_y; ++my)
        for (int mx = 0; mx < f.mcus_x; ++mx)
            for (int j = 0; j < f.bpm; ++j) jpeg_block_host(f, t, mx, my, j, coef + ((size_t)(my * (size_t)f.mcus_x + mx) * f.bpm + j) * 64);
}
struct JpegHostSink {
    uint8_t* p; unsigned long long acc = 0; int nb = 0;
    void put(unsigned code, int len) {
        acc = acc << len | code; nb += len;
        for (; nb >= 8; nb -= 8) { const uint8_t v = (uint8_t)(acc >> (nb - 8)); *p++ = v; if (v == 0xFF) *p++ = 0; }
    }
    void pad() { if (nb) put((1u << (8 - nb)) - 1u, 8 - nb); }
};
// the whole stream of one frame into f.out (jpeg_bound bytes are enough) -> its length.  No scratch: a block is coded as it is made.
inline long long jpeg_encode_host(const JpegFrame& f, const JpegTables& t) {
    uint8_t* o = f.out + jpeg_write_header(t, f, f.out);
    int16_t zz[64];
    for (int my = 0; my < f.mcus_y; ++my) {
        if (my) { *o++ = 0xFF; *o++ = (uint8_t)(0xD0 + ((my - 1) & 7)); }
        JpegHostSink s{o};
        int pred[3] = {0, 0, 0};
        for (int mx = 0; mx < f.mcus_x; ++mx)
            for (int j = 0; j < f.bpm; ++j) {
                const int c = f.bpm == 6 ? (j < 4 ? 0 : j - 3) : j, tc = c ? 1 : 0;
                jpeg_block_host(f, t, mx, my, j, zz);
                jpeg_code_block(zz, pred[c], t.dc_code[tc], t.dc_len[tc], t.ac_code[tc], t.ac_len[tc], s);
                pred[c] = zz[0];
            }
        s.pad();
        o = s.p;
    }
    *o++ = 0xFF; *o++ = 0xD9;
    return (long long)(o - f.out);
}

}  // namespace mi355
