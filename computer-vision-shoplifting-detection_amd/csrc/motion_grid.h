// Motion gate (include/mi355_yolo.h): what the kernel (motion_kernels.hip) and its host twin share -- the camera
// descriptor, the luma sums of one 16-pixel group of a row, and the test that calls a block changed.  Integers only: every figure
// the two produce is the same number.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#ifndef MI355_HD
#if defined(__HIPCC__)
#define MI355_HD __host__ __device__ __forceinline__
#else
#define MI355_HD inline
#endif
#endif

namespace mi355 {

constexpr int kMotionGroup = 16;       // pixels of a row one lane sums at a time: two halves of 8, the smallest block width

// One present camera of a tick, as the launch reads it (device memory; the host twin reads the same struct).
struct MotionCam {
    const uint8_t* src;                // first pixel; rows row_stride bytes apart, bpp bytes per pixel (3: BGR, 1: a Y plane)
    unsigned* cur;                     // [gh][gw] luma sums of this frame
    const unsigned* ref;               // [gh][gw] sums of the last frame that ran the detector, or nullptr: every block is flagged
    uint8_t* flags;                    // [gh][gw] 1 = block changed
    int H, W, row_stride, bpp;
    int gh, gw;
    int strip0;                        // index of this camera's first block-row strip among the launch's work items
    int pad_;
};

// BT.601 luma of cv2's BGR2GRAY in 14-bit fixed point (csrc/gmc_kernels.hip, oracle/gmc_oracle.py)
MI355_HD unsigned motion_luma(unsigned b, unsigned g, unsigned r) { return (1868u * b + 9617u * g + 4899u * r + 8192u) >> 14; }

MI355_HD unsigned motion_byte_sum(unsigned x) {
    const unsigned t = (x & 0x00ff00ffu) + ((x >> 8) & 0x00ff00ffu);
    return (t & 0xffffu) + (t >> 16);
}

// byte k of a little-endian word array (k is a constant after unrolling: a register and a field extract)
MI355_HD unsigned motion_word_byte(const unsigned* w, int k) { return (w[k >> 2] >> ((k & 3) * 8)) & 0xffu; }

// the two half sums of a FULL group held in words: w[0 .. 4 * bpp)
MI355_HD void motion_sums_words(const unsigned* w, int bpp, unsigned& lo, unsigned& hi) {
    if (bpp == 1) {
        lo += motion_byte_sum(w[0]) + motion_byte_sum(w[1]);
        hi += motion_byte_sum(w[2]) + motion_byte_sum(w[3]);
        return;
    }
#pragma unroll
    for (int i = 0; i < kMotionGroup; ++i) {
        const unsigned l = motion_luma(motion_word_byte(w, 3 * i), motion_word_byte(w, 3 * i + 1), motion_word_byte(w, 3 * i + 2));
        if (i < 8) lo += l; else hi += l;
    }
}

// Adds the luma of pixels [0, 8) of the group at p to lo and of pixels [8, 16) to hi; npix (1 .. 16) of them exist.  A full group whose
// address is 16-byte aligned is read with 16-byte loads, a 4-byte aligned one with 4-byte loads, anything else byte by byte: never a
// byte beyond pixel npix - 1.
MI355_HD void motion_group_sums(const uint8_t* p, int bpp, int npix, unsigned& lo, unsigned& hi) {
    const unsigned a = (unsigned)(uintptr_t)p;
    if (npix == kMotionGroup && (a & 3u) == 0) {
        unsigned w[12];
        if ((a & 15u) == 0) {
            struct alignas(16) V16 { unsigned x[4]; };
            const V16* q = (const V16*)p;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                if (j < bpp) { const V16 v = q[j]; w[4 * j] = v.x[0]; w[4 * j + 1] = v.x[1]; w[4 * j + 2] = v.x[2]; w[4 * j + 3] = v.x[3]; }
            }
        } else {
            const unsigned* q = (const unsigned*)p;
#pragma unroll
            for (int j = 0; j < 12; ++j) if (j < 4 * bpp) w[j] = q[j];
        }
        if (bpp == 1) motion_sums_words(w, 1, lo, hi); else motion_sums_words(w, 3, lo, hi);
        return;
    }
    for (int i = 0; i < npix; ++i) {
        const uint8_t* q = p + i * bpp;
        const unsigned l = bpp == 1 ? (unsigned)q[0] : motion_luma(q[0], q[1], q[2]);
        if (i < 8) lo += l; else hi += l;
    }
}

// 16 |S_cur - S_ref| > level_q * P: the block's mean luma moved by more than level_q / 16 (P = its pixels; edge blocks are partial)
MI355_HD unsigned motion_block_changed(unsigned s_cur, unsigned s_ref, unsigned level_q, unsigned pixels) {
    const unsigned d = s_cur > s_ref ? s_cur - s_ref : s_ref - s_cur;
    return 16u * d > level_q * pixels ? 1u : 0u;
}

// launcher of motion_kernels.hip: one wave per (camera, block-row strip); partial[total_strips] receives every strip's changed blocks
const char* launch_motion_grid(const MotionCam* cams_dev, int n_cams, int total_strips, int block, unsigned level_q, unsigned* partial_dev,
                               hipStream_t st);

}  // namespace mi355
