// Drives the HOST objects of csrc/gmc_kernels.hip (mi355_gmc_create(-1), mi355_gmc_multi_create(-1, 3)) through their state transitions
// on synthetic frames -- begin / finish, a skipped camera, a size change, reset, state, destroy -- and checks that the multi-camera object
// gives each camera the warps and the state of a single object of its own.  No HIP call is made, so it runs without a GPU; it is meant
// to be built with the host sanitizers (the Python tests cannot run under them):
//
//   cd computer-vision-shoplifting-detection_amd/csrc
//   hipcc -O1 -g --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined gmc_kernels.hip gmc_host.cpp \
//         ../../tools/gmc_host_drive.cpp -o /tmp/gmc_host_drive && /tmp/gmc_host_drive
#include "../include/mi355_yolo.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } } while (0)

// value noise (a hashed 6-px lattice, bilinear in between) panning 3 px per frame: corners exist, the optical flow has work
static unsigned lattice(int x, int y) {
    unsigned h = (unsigned)x * 374761393u + (unsigned)y * 668265263u;
    h = (h ^ (h >> 13)) * 1274126177u;
    return (h ^ (h >> 16)) & 255u;
}
static std::vector<uint8_t> frame(int h, int w, int t) {
    std::vector<uint8_t> f((size_t)h * w * 3);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const int u = x + 3 * t, v = y + t, gx = u / 6, gy = v / 6, ax = u % 6, ay = v % 6;
            const unsigned top = lattice(gx, gy) * (6 - ax) + lattice(gx + 1, gy) * ax, bot = lattice(gx, gy + 1) * (6 - ax) + lattice(gx + 1, gy + 1) * ax;
            const uint8_t g = (uint8_t)((top * (6 - ay) + bot * ay) / 36);
            for (int c = 0; c < 3; ++c) f[((size_t)y * w + x) * 3 + c] = g;
        }
    return f;
}

struct State {
    int oh = 0, ow = 0, n = 0; std::vector<uint8_t> gray; std::vector<float> pts;
    bool operator==(const State& o) const { return oh == o.oh && ow == o.ow && n == o.n && gray == o.gray && pts == o.pts; }
};
template <class Get>
static State state_of(Get get) {
    State s;
    get(&s.oh, &s.ow, &s.n, nullptr, nullptr, 0);
    s.gray.resize((size_t)s.oh * s.ow); s.pts.resize((size_t)s.n * 2);
    get(nullptr, nullptr, nullptr, s.gray.data(), s.pts.data(), s.n);
    return s;
}

int main() {
    const int N = 3, T = 7;
    int hs[N] = {96, 61, 24}, ws[N] = {128, 83, 40};           // the last one is smaller than the 21 x 21 window after downscaling
    mi355_gmc* one[N] = {};
    mi355_gmc_multi* multi = nullptr;
    for (int i = 0; i < N; ++i) CHECK(mi355_gmc_create(-1, &one[i]) == 0);
    CHECK(mi355_gmc_multi_create(-1, N, &multi) == 0);
    double H1[6], HM[N * 6];
    CHECK(mi355_gmc_track_finish(one[0], H1) == -1 && mi355_gmc_multi_finish(multi, HM) == -1);          // nothing pending
    for (int t = 0; t < T; ++t) {
        if (t == 4) { hs[1] = 70; ws[1] = 90; }                // camera 1 changes its size: its sequence restarts
        if (t == 5) { CHECK(mi355_gmc_track_reset(one[0]) == 0 && mi355_gmc_multi_reset(multi, 0) == 0); }
        std::vector<uint8_t> f[N];
        const uint8_t* ptr[N];
        for (int i = 0; i < N; ++i) {
            const bool absent = (i == 2 && t == 2);            // camera 2 skips a tick: its state stays
            if (!absent) f[i] = frame(hs[i], ws[i], t);
            ptr[i] = absent ? nullptr : f[i].data();
        }
        CHECK(mi355_gmc_multi_begin(multi, ptr, hs, ws, 2) == 0);
        CHECK(mi355_gmc_multi_begin(multi, ptr, hs, ws, 2) == -1);                                       // one tick at a time
        CHECK(mi355_gmc_multi_state(multi, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0) == -1);    // ... and no state while it is pending
        std::memset(HM, 0, sizeof(HM));
        CHECK(mi355_gmc_multi_finish(multi, HM) == 0);
        for (int i = 0; i < N; ++i) {
            if (!ptr[i]) { CHECK(HM[6 * i] == 0.0); continue; }                                         // the absent camera's row is untouched
            CHECK(mi355_gmc_track_begin(one[i], ptr[i], hs[i], ws[i], 2) == 0);
            CHECK(mi355_gmc_track_begin(one[i], ptr[i], hs[i], ws[i], 2) == -1);
            CHECK(mi355_gmc_track_finish(one[i], H1) == 0);
            CHECK(std::memcmp(H1, HM + 6 * i, sizeof(H1)) == 0);
            const bool first = t == 0 || (i == 1 && t == 4) || (i == 0 && t == 5);
            if (first) CHECK(H1[0] == 1 && H1[1] == 0 && H1[2] == 0 && H1[3] == 0 && H1[4] == 1 && H1[5] == 0);
            else if (i == 0) CHECK(H1[2] < -2.0 && H1[2] > -4.0);                                       // the scene moves 3 px per frame, in frame pixels
        }
        for (int i = 0; i < N; ++i) {
            const State a = state_of([&](int* oh, int* ow, int* n, uint8_t* g, float* p, int cap) { return mi355_gmc_track_state(one[i], oh, ow, n, g, p, cap); });
            const State b = state_of([&](int* oh, int* ow, int* n, uint8_t* g, float* p, int cap) { return mi355_gmc_multi_state(multi, i, oh, ow, n, g, p, cap); });
            CHECK(a == b && a.oh == hs[i] / 2 && a.ow == ws[i] / 2);
            if (i == 0) CHECK(a.n > 4);
        }
    }
    // the batched entry point on a host object is the single steps; a pending step refuses it; reset with a step pending drops it
    {
        std::vector<uint8_t> f0 = frame(hs[0], ws[0], T), f1 = frame(hs[0], ws[0], T + 1);
        const uint8_t* two[2] = {f0.data(), f1.data()};
        double HB[12];
        CHECK(mi355_gmc_track_begin(one[0], f0.data(), hs[0], ws[0], 2) == 0);
        CHECK(mi355_gmc_track_batch(one[0], two, 2, hs[0], ws[0], 2, HB) == -1);
        CHECK(mi355_gmc_track_reset(one[0]) == 0);
        int oh = -1;
        CHECK(mi355_gmc_track_state(one[0], &oh, nullptr, nullptr, nullptr, nullptr, 0) == 0 && oh == 0);
        CHECK(mi355_gmc_track_batch(one[0], two, 2, hs[0], ws[0], 2, HB) == 0);
        CHECK(HB[0] == 1 && HB[2] == 0 && HB[6 + 2] < -2.0 && HB[6 + 2] > -4.0);
    }
    CHECK(mi355_gmc_multi_begin(multi, nullptr, hs, ws, 2) == -1);
    for (int i = 0; i < N; ++i) mi355_gmc_destroy(one[i]);
    mi355_gmc_multi_destroy(multi);
    std::printf("gmc host drive ok: %d cameras x %d ticks, multi == single bit for bit\n", N, T);
    return 0;
}
