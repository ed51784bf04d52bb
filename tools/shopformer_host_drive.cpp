// Drives the loader of csrc/shopformer_host.hip (mi355_shopformer_create) over weight images and over damaged copies of them: every
// truncation at a 4-byte boundary of the header and the tensor table and at a few dozen points of the data, and every config word and
// every field of every table entry set to 0, -1 and a huge value.  A damaged image must be refused with MI355_EFORMAT, or pass every
// host-side check and reach the first HIP call; never a crash or an out-of-bounds read.  Without a GPU a whole image ends in the
// "no HIP device" error, which is raised only after every host-side check passed; so the program runs without one, and it is meant
// to be built with the host sanitizers (the Python tests cannot run under them).  The images are not committed; write them first:
//
//   python -c "import sys; sys.path.insert(0, 'tests'); import _shopformer_decoder_numpy as RD; from cvsd_amd import shopformer as SF
//   for n in ('default', 'kp18_t24', 'h32_l4', 'paper', 'default24'):
//       cfg, sd, _ = RD.fixture_model(n)
//       for d in (0, 1): open(f'/tmp/sf_{n}_{d}.img', 'wb').write(SF.image_from_state_dict(sd, cfg, decoder=bool(d)))"
//   cd computer-vision-shoplifting-detection_amd/csrc
//   hipcc -O1 -g --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined shopformer_host.hip shopformer_kernels.hip \
//         shopformer_decoder.hip pose_windows.hip ../../tools/shopformer_host_drive.cpp -o /tmp/shopformer_host_drive
//   /tmp/shopformer_host_drive /tmp/sf_*.img
#include "../include/mi355_yolo.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace mi355 { thread_local std::string g_err; }            // engine_abi.hip's, defined here so that the engine stays out of the link

#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s (%s)\n", __LINE__, #x, mi355::g_err.c_str()); return 1; } } while (0)

static long long g_creates = 0, g_refused = 0;

// -> 0: refused as a bad image; 1: every host-side check passed (no device to go on with, or a handle, destroyed here); -1: anything else
static int create(const uint8_t* p, size_t n) {
    mi355_shopformer* h = nullptr;
    const int rc = mi355_shopformer_create(p, n, 0, &h);
    ++g_creates;
    if (rc == MI355_OK) { mi355_shopformer_destroy(h); return 1; }
    if (h) return -1;
    if (rc == MI355_EFORMAT) { ++g_refused; return 0; }
    return rc == MI355_EHIP && mi355::g_err.rfind("no HIP device", 0) == 0 ? 1 : -1;
}

static int drive(const char* path) {
    std::FILE* f = std::fopen(path, "rb");
    CHECK(f != nullptr);
    std::vector<uint8_t> img;
    uint8_t chunk[65536];
    for (size_t k; (k = std::fread(chunk, 1, sizeof(chunk), f)) > 0;) img.insert(img.end(), chunk, chunk + k);
    std::fclose(f);
    CHECK(img.size() > 24 && create(img.data(), img.size()) == 1);
    uint32_t ncfg, nent;
    std::memcpy(&ncfg, img.data() + 12, 4);
    const size_t table = 16 + 4 * (size_t)ncfg + 4;
    std::memcpy(&nent, img.data() + table - 4, 4);
    const size_t data = (table + 64 * (size_t)nent + 15) / 16 * 16;
    CHECK(data < img.size());
    // truncations, each in an allocation of exactly its size: a read past the cut is a read past the buffer
    std::vector<size_t> cuts;
    for (size_t c = 4; c <= data; c += 4) cuts.push_back(c);
    for (int i = 1; i <= 48; ++i) cuts.push_back(data + (img.size() - data) * i / 49 / 4 * 4);
    cuts.push_back(img.size() - 4); cuts.push_back(img.size() - 1);
    for (size_t c : cuts) {
        std::vector<uint8_t> cut(img.begin(), img.begin() + c);
        CHECK(create(cut.data(), cut.size()) == 0);
    }
    // one field at a time, restored afterwards
    const uint32_t vals[3] = {0u, 0xffffffffu, 0x7fffffffu};
    auto poke = [&](size_t off, size_t width) {
        uint8_t keep[8];
        std::memcpy(keep, img.data() + off, width);
        for (uint32_t v : vals) {
            const uint64_t w = width == 8 ? (v == 0xffffffffu ? ~0ull : v == 0 ? 0ull : 0x7fffffffffffffffull) : v;
            std::memcpy(img.data() + off, &w, width);
            if (create(img.data(), img.size()) < 0) return false;
        }
        std::memcpy(img.data() + off, keep, width);
        return true;
    };
    for (size_t off = 8; off < table; off += 4) CHECK(poke(off, 4));                       // version, word count, config words, entry count
    for (uint32_t e = 0; e < nent; ++e) {
        const size_t r = table + 64 * (size_t)e;
        for (size_t off = 32; off < 48; off += 4) CHECK(poke(r + off, 4));                 // kind, three dims
        CHECK(poke(r + 48, 8) && poke(r + 56, 8));                                         // off, count
    }
    CHECK(create(img.data(), img.size()) == 1);                                            // everything was restored
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: %s image...\n", argv[0]); return 2; }
    mi355_shopformer* h = nullptr;
    CHECK(mi355_shopformer_create(nullptr, 0, 0, &h) == MI355_EINVAL);
    for (int i = 1; i < argc; ++i) if (drive(argv[i])) { std::printf("... in %s\n", argv[i]); return 1; }
    std::printf("shopformer host drive ok: %d images, %lld creates, %lld refused as bad images, none crashed\n", argc - 1, g_creates, g_refused);
    return 0;
}
