// Merge of the per-entry rows of a tiled predict call (include/mi355_yolo.h): what the kernel (post_kernels.hip) and
// its host twin (engine_tiled.hip) share -- the argument block, the overlap test and the word-by-word shift of a row.  Both translation
// units switch FP contraction off: inter = w * h is rounded to fp32 before the IoU's subtraction reads it.
#pragma once
#include "common.h"
#include "../../include/mi355_yolo.h"

#if defined(__HIPCC__)
#define MI355_HD __host__ __device__ __forceinline__
#else
#define MI355_HD inline
#endif

#pragma clang fp contract(off)       // from here to the end of the including file (both includers state it themselves as well)

namespace mi355 {

constexpr int TILE_ROW_WORDS = (int)(sizeof(mi355_det) / 4);

struct TileMergeArgs {
    const unsigned* rows;          // [sum of entries][max_det][TILE_ROW_WORDS]: the per-entry rows as NMS wrote them
    const int* counts;             // [sum of entries] rows kept per entry
    const int* origins;            // [sum of entries][2] = ox, oy of the entry inside its frame
    const int* entry_off;          // [n_frames + 1] first entry of every frame, or nullptr: frame f owns entries [f * entries, (f + 1) * entries)
    int n_frames, entries;         // entries = the LARGEST entry count of a frame (<= MI355_TILE_MAX_ENTRIES)
    int max_det, nk, kdim;         // nk = keypoint floats of a row (kdim >= 2: float j is an x when j % kdim == 0, a y when j % kdim == 1)
    int metric; float thr;
    unsigned long long* keys;      // scratch [n_frames][key_stride], read and written only when a frame has more than 4096 candidates
    int key_stride;                // power of two >= entries * max_det, or 0 when entries * max_det <= 4096
    unsigned* out_rows;            // [n_frames][max_det][TILE_ROW_WORDS]
    int* out_counts;               // [n_frames]
    int* out_tile_idx;             // [n_frames][max_det], or nullptr
};
const char* launch_tile_merge(const TileMergeArgs& a, hipStream_t st);

struct TileBox { float x1, y1, x2, y2, area; };

MI355_HD bool tile_overlap_gt(const TileBox& i, const TileBox& j, int metric, float thr) {
    const float xx1 = i.x1 > j.x1 ? i.x1 : j.x1, yy1 = i.y1 > j.y1 ? i.y1 : j.y1;
    const float xx2 = i.x2 < j.x2 ? i.x2 : j.x2, yy2 = i.y2 < j.y2 ? i.y2 : j.y2;
    const float dw = xx2 - xx1, dh = yy2 - yy1;
    const float w = dw > 0.f ? dw : 0.f, h = dh > 0.f ? dh : 0.f;
    const float inter = w * h;
    float den;
    if (metric == MI355_TILE_IOS) den = i.area < j.area ? i.area : j.area;
    else { const float s = i.area + j.area; den = s - inter; }
    const float m = inter / den;
    return m > thr;                                       // NaN (0 / 0) compares false
}

// word q of a row of an entry at (ox, oy), as the merged row carries it
MI355_HD unsigned tile_shift_word(unsigned w, int q, float ox, float oy, int nk, int kdim) {
    const float v = __builtin_bit_cast(float, w);
    if (q < 4) return __builtin_bit_cast(unsigned, v + ((q & 1) ? oy : ox));
    const int j = q - 7;
    if (j >= 0 && j < nk && kdim >= 2) {
        const int c = j % kdim;
        if (c == 0) return __builtin_bit_cast(unsigned, v + ox);
        if (c == 1) return __builtin_bit_cast(unsigned, v + oy);
    }
    return w;
}

}  // namespace mi355
