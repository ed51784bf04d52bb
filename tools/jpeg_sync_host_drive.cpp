// Stand-alone driver of the host twin of entropy = sync (csrc/jpeg_sync.h, csrc/jpeg_decode_host.cpp) for a sanitizer run
// on the CPU: no HIP, no Python.  It reads a corpus file -- uint32 count, then per stream uint32 length and the bytes, little-endian;
// tests/test_jpeg_sync_cases.py writes one: the case table, truncations, bit flips, refused and corrupt streams -- and runs, on every
// stream the parser takes, mi355_jpeg_decode(-1, ..., MI355_JPEG_ENTROPY_SYNC) and mi355_op_jpeg_sync(-1, ...) with subsequences of 8 and
// of 128 bytes.  Each stream, destination, coefficient and state array lives in a heap block of exactly its size.  The statuses must
// be the sequential routine's (mi355_op_jpeg_decode_coefficients with MI355_JPEG_ENTROPY_HOST), and for a stream that decodes so must
// the coefficients; nothing may crash, hang or touch memory it does not own.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DMI355_JPEG_DECODE_STANDALONE \
//       -I computer-vision-shoplifting-detection_amd/csrc tools/jpeg_sync_host_drive.cpp \
//       computer-vision-shoplifting-detection_amd/csrc/jpeg_decode_host.cpp -o jpeg_sync_host_drive && ./jpeg_sync_host_drive corpus.bin
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../include/mi355_yolo.h"

static uint32_t u32(FILE* f) {
    unsigned char b[4];
    if (std::fread(b, 1, 4, f) != 4) { std::printf("corpus: short read\n"); std::exit(2); }
    return (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24;
}

int main(int argc, char** argv) {
    if (argc != 2) { std::printf("usage: jpeg_sync_host_drive corpus.bin\n"); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
    const uint32_t count = u32(f);
    long decoded = 0, refused = 0, corrupt = 0;
    for (uint32_t i = 0; i < count; ++i) {
        const uint32_t len = u32(f);
        std::unique_ptr<uint8_t[]> exact(new uint8_t[len]);               // exactly the stream: reading exact[len] is out of bounds
        if (len && std::fread(exact.get(), 1, len, f) != len) { std::printf("corpus: short read\n"); return 2; }
        mi355_jpeg_stream_info info;
        mi355_jpeg_stream s{exact.get(), (int64_t)len, 0, 0};
        mi355_jpeg_sync_stats stats;
        if (mi355_jpeg_info(len ? exact.get() : nullptr, len, &info) != MI355_OK) {
            if (len && mi355_op_jpeg_sync(-1, &s, 8, 4, nullptr, nullptr, nullptr, 0, &stats) == MI355_OK) { std::printf("stream %u: the hook takes a refused stream\n", i); return 3; }
            ++refused;
            continue;
        }
        const size_t px = (size_t)info.height * info.width * 3, nc = (size_t)info.blocks * 64;
        std::unique_ptr<uint8_t[]> out(new uint8_t[px]);
        std::unique_ptr<int16_t[]> want(new int16_t[nc]), got(new int16_t[nc]);
        int16_t* wp = want.get();
        int wstatus = -1, status = -1;
        const int rcw = mi355_op_jpeg_decode_coefficients(-1, &s, 1, MI355_JPEG_ENTROPY_HOST, &wp, &wstatus);
        mi355_render_out o{out.get(), info.width * 3, 0};
        const int rc = mi355_jpeg_decode(-1, &s, 1, MI355_JPEG_ENTROPY_SYNC, &o, &status, nullptr, nullptr);
        if (s.entropy_used != MI355_JPEG_ENTROPY_SYNC || (rc == MI355_OK) != (status == 0) || (rcw == MI355_OK) != (wstatus == 0) || status != wstatus) {
            std::printf("stream %u: sync returns %d with status %d, the sequential routine %d with status %d\n", i, rc, status, rcw, wstatus);
            return 3;
        }
        static const int settings[2][2] = {{8, 4}, {128, 256}};
        for (const auto& st : settings) {
            if (mi355_op_jpeg_sync(-1, &s, st[0], st[1], nullptr, nullptr, nullptr, 0, &stats) != MI355_OK || stats.nsub < 1 || stats.nseq < 1) {
                std::printf("stream %u: the hook cannot size its states\n", i);
                return 3;
            }
            std::unique_ptr<mi355_jpeg_sync_state[]> states(new mi355_jpeg_sync_state[(size_t)stats.nsub]);
            int hstatus = -1;
            const int rch = mi355_op_jpeg_sync(-1, &s, st[0], st[1], got.get(), &hstatus, states.get(), stats.nsub, &stats);
            if (rch != MI355_OK || hstatus != wstatus) {
                std::printf("stream %u at (%d, %d): the hook returns %d with status %d, the sequential routine status %d\n", i, st[0], st[1], rch, hstatus, wstatus);
                return 3;
            }
            if (!wstatus && std::memcmp(got.get(), want.get(), nc * 2)) { std::printf("stream %u at (%d, %d): coefficients differ\n", i, st[0], st[1]); return 3; }
        }
        if (rc == MI355_OK) ++decoded; else ++corrupt;
    }
    std::fclose(f);
    std::printf("jpeg_sync_host_drive ok: %u streams, decoded %ld, refused %ld, corrupt %ld\n", count, decoded, refused, corrupt);
    return 0;
}
