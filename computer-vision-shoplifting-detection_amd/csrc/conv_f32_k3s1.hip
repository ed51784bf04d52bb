// Instances of conv_igemm_f32 for 3x3 convs of stride 1 (device code: conv_f32.h).
#include "conv_f32.h"
#include "conv_f32_inst.h"

namespace mi355 {

KernelFn pick_f32_k3s1(int CT, int WP, int PT) {
    if (PT == 0) {
#define MI355_CASE(ct, wp) if (CT == ct && WP == wp) return &conv_igemm_f32<3, 1, (ct == 5 ? 3 : 4), ct, wp>;
        MI355_CASE(1, 4) MI355_CASE(2, 4) MI355_CASE(3, 4) MI355_CASE(4, 4) MI355_CASE(5, 4)
        MI355_CASE(1, 2) MI355_CASE(2, 2) MI355_CASE(3, 2) MI355_CASE(4, 2) MI355_CASE(5, 2)
        MI355_CASE(1, 1) MI355_CASE(2, 1) MI355_CASE(3, 1) MI355_CASE(4, 1) MI355_CASE(5, 1)
#undef MI355_CASE
        return nullptr;
    }
    // small wave tiles (1 or 2 pixel tiles per wave) for latency-bound launches: a batch-1 map has few pixels, so the
    // planner trades register blocking for more waves
#define MI355_CASE(pt, ct, wp) if (PT == pt && CT == ct && WP == wp) return &conv_igemm_f32<3, 1, pt, ct, wp>;
    MI355_CASE(1, 1, 4) MI355_CASE(1, 2, 4) MI355_CASE(1, 1, 2) MI355_CASE(1, 2, 2) MI355_CASE(1, 1, 1) MI355_CASE(1, 2, 1)
    MI355_CASE(2, 1, 4) MI355_CASE(2, 2, 4) MI355_CASE(2, 1, 2) MI355_CASE(2, 2, 2) MI355_CASE(2, 1, 1) MI355_CASE(2, 2, 1)
    // five pixel tiles per wave (blocks of 80 / 160 / 320 pixels): the 20x20 and 40x40 maps of a 640x640 frame tile exactly
    MI355_CASE(5, 1, 4) MI355_CASE(5, 2, 4) MI355_CASE(5, 3, 4) MI355_CASE(5, 1, 2) MI355_CASE(5, 2, 2) MI355_CASE(5, 3, 2)
    MI355_CASE(5, 1, 1) MI355_CASE(5, 2, 1) MI355_CASE(5, 3, 1)
    // five cout tiles per wave over two / one pixel tiles (blocks of 128 / 64 pixels, all four waves along the pixels): 80 couts in one
    // block along grid.y, the halo tile staged once for all of them
    MI355_CASE(2, 5, 4) MI355_CASE(1, 5, 4)
#undef MI355_CASE
    return nullptr;
}

}  // namespace mi355
