// Evidence frames (include/mi355_yolo.h "render"): the raster rules, stated once for the kernel (render_kernels.hip) and
// its host twin.  Integers only: which pixels a primitive covers, which tiles it can touch, and the mean a mosaic block takes are the
// same numbers on both targets.
//
// A primitive is kRenderWords int32: {type, a, b, c, d, size, colour, 0}; colour = B | G << 8 | R << 16.  A pixel is the point
// (px, py); a rectangle (x0, y0, x1, y1) holds the pixels x0 <= px <= x1, y0 <= py <= y1 (x1 < x0 or y1 < y0: none).
//   MOSAIC  a..d = rectangle, size = B in {4, 8, 16, 32}: a covered pixel takes the rounded mean of the source frame's B x B block
//           that contains it (blocks aligned to the frame's origin, clipped by the frame's right and bottom edge).
//   RECT    a..d = rectangle, size = t: inside the rectangle and not inside the rectangle shrunk by t on every side.
//   FILL    a..d = rectangle.
//   LINE    A = (a, b), B = (c, d), size = t: 4 dist^2 <= t^2, dist = distance from the pixel to the segment (below).
//   DISC    centre (a, b), size = r: (px - a)^2 + (py - b)^2 <= r^2.
//   GLYPH   top-left (a, b), c = character, size = scale: the set bits of a 5 x 7 bitmap, each a scale x scale square.
// Ranges (render_check refuses anything else, so the products below cannot overflow): |coordinate| <= 2^20, frame sides <= 2^14,
// t in 1 .. 255, r in 0 .. 2^20, scale in 1 .. 64.  Differences are then below 2^22, dot products and the cross product below 2^45:
// 64-bit.  The SQUARED cross product would need 90 bits, so the between-case first drops pixels with |cross| > t (|dx| + |dy|) -- they
// are outside, because the segment is no longer than |dx| + |dy| -- and what is left has |cross| <= 2^30, 4 cross^2 <= 2^62.
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

constexpr int kRenderWords = 8;                 // int32 per primitive
constexpr int kRenderTile = 32;                 // pixels per tile side: every mosaic block lies inside one tile
constexpr int kRenderTileRow = kRenderTile * 3; // bytes of a staged tile row
constexpr int kRenderMaxPrims = 16384;          // per frame: 300 boxes x (mosaic + box + label of 11 + 19 limbs + 17 joints) = 14700
constexpr int kRenderMaxCoord = 1 << 20;
constexpr int kRenderMaxSide = 1 << 14;
constexpr int kRenderMeans = 64 + 16 + 4 + 1;   // block means of a tile: B = 4, 8, 16, 32
enum RenderType { RENDER_MOSAIC = 1, RENDER_RECT = 2, RENDER_FILL = 3, RENDER_LINE = 4, RENDER_DISC = 5, RENDER_GLYPH = 6 };

constexpr int kGlyphW = 5, kGlyphH = 7, kGlyphCount = 16;
// rows top to bottom, bit 4 = leftmost column: 0 1 2 3 4 5 6 7 8 9 # . : % - space
constexpr uint8_t kGlyphRows[kGlyphCount][kGlyphH] = {
    {0x0E, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0E}, {0x04, 0x0C, 0x04, 0x04, 0x04, 0x04, 0x0E}, {0x0E, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1F},
    {0x1F, 0x02, 0x04, 0x02, 0x01, 0x11, 0x0E}, {0x02, 0x06, 0x0A, 0x12, 0x1F, 0x02, 0x02}, {0x1F, 0x10, 0x1E, 0x01, 0x01, 0x11, 0x0E},
    {0x06, 0x08, 0x10, 0x1E, 0x11, 0x11, 0x0E}, {0x1F, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08}, {0x0E, 0x11, 0x11, 0x0E, 0x11, 0x11, 0x0E},
    {0x0E, 0x11, 0x11, 0x0F, 0x01, 0x02, 0x0C}, {0x0A, 0x0A, 0x1F, 0x0A, 0x1F, 0x0A, 0x0A}, {0x00, 0x00, 0x00, 0x00, 0x00, 0x0C, 0x0C},
    {0x00, 0x0C, 0x0C, 0x00, 0x0C, 0x0C, 0x00}, {0x18, 0x19, 0x02, 0x04, 0x08, 0x13, 0x03}, {0x00, 0x00, 0x00, 0x1F, 0x00, 0x00, 0x00},
    {0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00}};

// index into kGlyphRows, or -1: the character is not in the font
MI355_HD int render_glyph_index(int ch) {
    if (ch >= '0' && ch <= '9') return ch - '0';
    return ch == '#' ? 10 : ch == '.' ? 11 : ch == ':' ? 12 : ch == '%' ? 13 : ch == '-' ? 14 : ch == ' ' ? 15 : -1;
}
// one row of a glyph (the table above, as a switch: a device function cannot read a host constexpr array by a run-time index)
MI355_HD unsigned render_glyph_row(int gi, int row) {
    unsigned long long lo = 0;                  // 7 rows x 5 bits = 35 bits per glyph, packed from the table at compile time
    switch (gi) {
#define MI355_G(i)                                                                                                                       \
    case i:                                                                                                                              \
        lo = (unsigned long long)kGlyphRows[i][0] | (unsigned long long)kGlyphRows[i][1] << 5 | (unsigned long long)kGlyphRows[i][2] << 10 | \
             (unsigned long long)kGlyphRows[i][3] << 15 | (unsigned long long)kGlyphRows[i][4] << 20 | (unsigned long long)kGlyphRows[i][5] << 25 | \
             (unsigned long long)kGlyphRows[i][6] << 30;                                                                                 \
        break;
        MI355_G(0) MI355_G(1) MI355_G(2) MI355_G(3) MI355_G(4) MI355_G(5) MI355_G(6) MI355_G(7) MI355_G(8) MI355_G(9) MI355_G(10) MI355_G(11)
        MI355_G(12) MI355_G(13) MI355_G(14) MI355_G(15)
#undef MI355_G
    default: break;
    }
    return (unsigned)(lo >> (5 * row)) & 31u;
}

MI355_HD int render_min(int a, int b) { return a < b ? a : b; }
MI355_HD int render_max(int a, int b) { return a > b ? a : b; }

// nullptr, or why the record is refused
inline const char* render_check_prim(const int* p) {
    const int type = p[0], size = p[5];
    if (type < RENDER_MOSAIC || type > RENDER_GLYPH) return "unknown primitive type";
    const int ncoord = type == RENDER_DISC || type == RENDER_GLYPH ? 2 : 4;
    for (int i = 1; i <= ncoord; ++i)
        if (p[i] < -kRenderMaxCoord || p[i] > kRenderMaxCoord) return "a coordinate is outside [-2^20, 2^20]";
    if ((unsigned)p[6] > 0xffffffu) return "colour must be B | G << 8 | R << 16";
    switch (type) {
    case RENDER_MOSAIC: return size == 4 || size == 8 || size == 16 || size == 32 ? nullptr : "a mosaic block must be 4, 8, 16 or 32";
    case RENDER_RECT: case RENDER_LINE: return size >= 1 && size <= 255 ? nullptr : "thickness must be in 1 .. 255";
    case RENDER_DISC: return size >= 0 && size <= kRenderMaxCoord ? nullptr : "radius must be in 0 .. 2^20";
    case RENDER_GLYPH:
        if (render_glyph_index(p[3]) < 0) return "character is not in the built-in font (0-9 # . : % - space)";
        return size >= 1 && size <= 64 ? nullptr : "glyph scale must be in 1 .. 64";
    default: return nullptr;
    }
}

// the primitive's bounding box (may be empty or off-frame); every covered pixel lies inside it
MI355_HD void render_bbox(const int* p, int& x0, int& y0, int& x1, int& y1) {
    switch (p[0]) {
    case RENDER_LINE: {
        const int h = (p[5] + 1) >> 1;
        x0 = render_min(p[1], p[3]) - h; x1 = render_max(p[1], p[3]) + h; y0 = render_min(p[2], p[4]) - h; y1 = render_max(p[2], p[4]) + h;
        break;
    }
    case RENDER_DISC: x0 = p[1] - p[5]; x1 = p[1] + p[5]; y0 = p[2] - p[5]; y1 = p[2] + p[5]; break;
    case RENDER_GLYPH: x0 = p[1]; y0 = p[2]; x1 = p[1] + kGlyphW * p[5] - 1; y1 = p[2] + kGlyphH * p[5] - 1; break;
    default: x0 = p[1]; y0 = p[2]; x1 = p[3]; y1 = p[4]; break;
    }
}

// can the primitive cover a pixel of the pixel rectangle [tx0, tx1] x [ty0, ty1]?  (its bounding box meets it, and for an outline the
// rectangle does not lie wholly in the hollow)
MI355_HD bool render_touches(const int* p, int tx0, int ty0, int tx1, int ty1) {
    int x0, y0, x1, y1;
    render_bbox(p, x0, y0, x1, y1);
    if (x1 < x0 || y1 < y0 || x1 < tx0 || x0 > tx1 || y1 < ty0 || y0 > ty1) return false;
    if (p[0] == RENDER_RECT) {
        const int t = p[5];
        if (tx0 >= x0 + t && tx1 <= x1 - t && ty0 >= y0 + t && ty1 <= y1 - t) return false;
    }
    return true;
}

// does a primitive other than a mosaic cover pixel (px, py)?
MI355_HD bool render_hit(const int* p, int px, int py) {
    switch (p[0]) {
    case RENDER_FILL: return px >= p[1] && px <= p[3] && py >= p[2] && py <= p[4];
    case RENDER_RECT: {
        if (px < p[1] || px > p[3] || py < p[2] || py > p[4]) return false;
        const int t = p[5];
        return !(px >= p[1] + t && px <= p[3] - t && py >= p[2] + t && py <= p[4] - t);
    }
    case RENDER_DISC: {
        const long long dx = px - p[1], dy = py - p[2], r = p[5];
        return dx * dx + dy * dy <= r * r;
    }
    case RENDER_LINE: {
        const long long dx = p[3] - p[1], dy = p[4] - p[2], qx = px - p[1], qy = py - p[2], t = p[5];
        const long long u = qx * dx + qy * dy, len2 = dx * dx + dy * dy;
        if (u <= 0) return 4 * (qx * qx + qy * qy) <= t * t;                       // beyond A (and A = B: a disc)
        if (u >= len2) {                                                           // beyond B
            const long long rx = px - p[3], ry = py - p[4];
            return 4 * (rx * rx + ry * ry) <= t * t;
        }
        long long cr = dx * qy - dy * qx;
        if (cr < 0) cr = -cr;
        const long long l1 = (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy);
        if (cr > t * l1) return false;                                             // farther than t from the line: outside, and cr^2 would not fit
        return 4 * cr * cr <= t * t * len2;
    }
    case RENDER_GLYPH: {
        const int s = p[5], ox = px - p[1], oy = py - p[2];
        if (ox < 0 || oy < 0 || ox >= kGlyphW * s || oy >= kGlyphH * s) return false;
        return (render_glyph_row(render_glyph_index(p[3]), oy / s) >> (kGlyphW - 1 - ox / s)) & 1u;
    }
    default: return false;
    }
}

// index of the mean of the B x B block that holds the tile-local pixel (lx, ly): [B = 4: 64 | 8: 16 | 16: 4 | 32: 1]
MI355_HD int render_mean_index(int B, int lx, int ly) {
    switch (B) {
    case 4: return (ly >> 2) * 8 + (lx >> 2);
    case 8: return 64 + (ly >> 3) * 4 + (lx >> 3);
    case 16: return 80 + (ly >> 4) * 2 + (lx >> 4);
    default: return 84;
    }
}
// block `mi` of a tile of tw x th pixels: its side B, origin (bx, by) inside the tile and how many pixels of it exist
MI355_HD int render_mean_block(int mi, int tw, int th, int& B, int& bx, int& by) {
    int per;
    if (mi < 64) { B = 4; per = 8; } else if (mi < 80) { B = 8; per = 4; mi -= 64; } else if (mi < 84) { B = 16; per = 2; mi -= 80; } else { B = 32; per = 1; mi -= 84; }
    bx = (mi % per) * B; by = (mi / per) * B;
    const int w = render_min(B, tw - bx), h = render_min(B, th - by);
    return w > 0 && h > 0 ? w * h : 0;
}
// rounded integer mean (halves up)
MI355_HD unsigned render_mean(unsigned sum, unsigned n) { return (2u * sum + n) / (2u * n); }

// One primitive on the four pixels (gx .. gx + 3, gy) of a tile whose first pixel is (tx0, ty0).  pass 0 applies mosaics (from `means`,
// the tile's block means of the SOURCE), pass 1 everything else; the caller walks the tile's primitives in ascending index per pass.
MI355_HD void render_apply(const int* p, int pass, int gx, int gy, int tx0, int ty0, const unsigned* means, unsigned px[4]) {
    const bool mosaic = p[0] == RENDER_MOSAIC;
    if (mosaic != (pass == 0)) return;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < 4; ++k) {
        const int x = gx + k;
        if (mosaic) {
            if (x >= p[1] && x <= p[3] && gy >= p[2] && gy <= p[4]) px[k] = means[render_mean_index(p[5], x - tx0, gy - ty0)];
        } else if (render_hit(p, x, gy)) {
            px[k] = (unsigned)p[6];
        }
    }
}

// Host twin of one tile: stile = the staged source tile (rows kRenderTileRow bytes apart, tw x th pixels valid), words = the tile's
// bin mask over the frame's P primitives; the drawn tile is written back into stile.
inline void render_tile_host(uint8_t* stile, int tx0, int ty0, int tw, int th, const int* prims, const unsigned* words, int nwords, bool any_mosaic) {
    unsigned means[kRenderMeans] = {0};
    if (any_mosaic) {
        for (int mi = 0; mi < kRenderMeans; ++mi) {
            int B, bx, by;
            const int n = render_mean_block(mi, tw, th, B, bx, by);
            if (!n) continue;
            unsigned m = 0;
            for (int ch = 0; ch < 3; ++ch) {
                unsigned s = 0;
                for (int y = by; y < render_min(by + B, th); ++y)
                    for (int x = bx; x < render_min(bx + B, tw); ++x) s += stile[y * kRenderTileRow + x * 3 + ch];
                m |= render_mean(s, (unsigned)n) << (8 * ch);
            }
            means[mi] = m;
        }
    }
    for (int ly = 0; ly < th; ++ly)
        for (int lx = 0; lx < tw; lx += 4) {
            unsigned px[4] = {0, 0, 0, 0};
            for (int k = 0; k < 4 && lx + k < tw; ++k) {
                const uint8_t* s = stile + ly * kRenderTileRow + (lx + k) * 3;
                px[k] = (unsigned)s[0] | (unsigned)s[1] << 8 | (unsigned)s[2] << 16;
            }
            for (int pass = any_mosaic ? 0 : 1; pass < 2; ++pass)
                for (int w = 0; w < nwords; ++w)
                    for (unsigned m = words[w]; m; m &= m - 1) {
                        int b = 0;
                        while (!((m >> b) & 1u)) ++b;
                        render_apply(prims + (size_t)(32 * w + b) * kRenderWords, pass, tx0 + lx, ty0 + ly, tx0, ty0, means, px);
                    }
            for (int k = 0; k < 4 && lx + k < tw; ++k) {
                uint8_t* s = stile + ly * kRenderTileRow + (lx + k) * 3;
                s[0] = (uint8_t)px[k]; s[1] = (uint8_t)(px[k] >> 8); s[2] = (uint8_t)(px[k] >> 16);
            }
        }
}

// One frame of a call as the launches read it (device memory; the host twin reads the same struct with host pointers).
struct RenderFrame {
    const uint8_t* src; uint8_t* dst;
    const int* prims;                  // [P][kRenderWords]
    unsigned* bins;                    // [tiles][words]: bit i of a tile's mask = primitive i can touch the tile
    unsigned* flags;                   // [tiles]: bit 0 = some primitive, bit 1 = some mosaic
    int H, W, src_pitch, dst_pitch;
    int P, words, tiles_x, tiles_y;
    int vec, pad_;                     // 1: src, dst and both pitches are multiples of 16 bytes (full-width tiles move as 16-byte vectors)
};

// the whole frame on the host: bins built as the bin launch builds them, tiles drawn by render_tile_host
inline void render_frame_host(const RenderFrame& f) {
    const int words = f.words;
    unsigned* mask = words ? new unsigned[(size_t)words] : nullptr;
    uint8_t stile[kRenderTile * kRenderTileRow];
    for (int ty = 0; ty < f.tiles_y; ++ty)
        for (int tx = 0; tx < f.tiles_x; ++tx) {
            const int x0 = tx * kRenderTile, y0 = ty * kRenderTile, tw = render_min(kRenderTile, f.W - x0), th = render_min(kRenderTile, f.H - y0);
            bool any = false, mosaic = false;
            for (int w = 0; w < words; ++w) mask[w] = 0;
            for (int i = 0; i < f.P; ++i) {
                const int* p = f.prims + (size_t)i * kRenderWords;
                if (!render_touches(p, x0, y0, x0 + tw - 1, y0 + th - 1)) continue;
                mask[i >> 5] |= 1u << (i & 31); any = true; mosaic |= p[0] == RENDER_MOSAIC;
            }
            for (int y = 0; y < th; ++y)
                for (int b = 0; b < tw * 3; ++b) stile[y * kRenderTileRow + b] = f.src[(size_t)(y0 + y) * f.src_pitch + (size_t)x0 * 3 + b];
            if (any) render_tile_host(stile, x0, y0, tw, th, f.prims, mask, words, mosaic);
            for (int y = 0; y < th; ++y)
                for (int b = 0; b < tw * 3; ++b) f.dst[(size_t)(y0 + y) * f.dst_pitch + (size_t)x0 * 3 + b] = stile[y * kRenderTileRow + b];
        }
    delete[] mask;
}

#if defined(__HIPCC__)
// launchers of render_kernels.hip: frames_dev[n] on the device, frames_host the same descriptors for sizing the grids
const char* launch_render(const RenderFrame* frames_dev, const RenderFrame* frames_host, int n, hipStream_t st);
#endif

}  // namespace mi355
