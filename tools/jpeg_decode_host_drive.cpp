// Stand-alone driver of the JPEG decoder's host twin (csrc/jpeg_decode.h, csrc/jpeg_decode_host.cpp) for a sanitizer
// run on the CPU: no HIP, no Python.  It reads a corpus file -- uint32 count, then per stream uint32 length and the bytes, little-endian;
// tests/test_jpeg_decode_cases.py writes one: the case table, truncations, bit flips, refused and corrupt streams -- and runs
// mi355_jpeg_info, mi355_jpeg_decode(-1, ...) and mi355_op_jpeg_decode_coefficients(-1, ...) on every stream.  Each stream, each BGR
// destination and each coefficient array lives in a heap block of exactly its size, so a read or a write one byte outside is reported.
// Refused and corrupt streams must come back as errors; nothing may crash, hang or touch memory it does not own.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DMI355_JPEG_DECODE_STANDALONE \
//       -I computer-vision-shoplifting-detection_amd/csrc tools/jpeg_decode_host_drive.cpp \
//       computer-vision-shoplifting-detection_amd/csrc/jpeg_decode_host.cpp -o jpeg_decode_host_drive && ./jpeg_decode_host_drive corpus.bin
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
    if (argc != 2) { std::printf("usage: jpeg_decode_host_drive corpus.bin\n"); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
    const uint32_t count = u32(f);
    long decoded = 0, refused = 0, corrupt = 0;
    unsigned long long sum = 0;
    for (uint32_t i = 0; i < count; ++i) {
        const uint32_t len = u32(f);
        std::unique_ptr<uint8_t[]> data(new uint8_t[len ? len : 1]);
        if (len && std::fread(data.get(), 1, len, f) != len) { std::printf("corpus: short read\n"); return 2; }
        std::unique_ptr<uint8_t[]> exact(new uint8_t[len]);               // exactly the stream: reading data[len] is out of bounds
        std::memcpy(exact.get(), data.get(), len);
        mi355_jpeg_stream_info info;
        if (mi355_jpeg_info(len ? exact.get() : nullptr, len, &info) != MI355_OK) {
            if (!mi355_last_error()[0]) { std::printf("stream %u: refused without a reason\n", i); return 3; }
            ++refused;
            continue;
        }
        const size_t px = (size_t)info.height * info.width * 3;
        std::unique_ptr<uint8_t[]> out(new uint8_t[px]);
        std::unique_ptr<int16_t[]> coef(new int16_t[(size_t)info.blocks * 64]);
        mi355_jpeg_stream s{exact.get(), (int64_t)len, 0, 0};
        mi355_render_out o{out.get(), info.width * 3, 0};
        int status = -1, cstatus = -1;
        const int rc = mi355_jpeg_decode(-1, &s, 1, MI355_JPEG_ENTROPY_AUTO, &o, &status, nullptr, nullptr);
        int16_t* cp = coef.get();
        const int rc2 = mi355_op_jpeg_decode_coefficients(-1, &s, 1, MI355_JPEG_ENTROPY_HOST, &cp, &cstatus);
        if ((rc == MI355_OK) != (status == 0) || (rc2 == MI355_OK) != (cstatus == 0) || status != cstatus || status < 0 || status > 4) {
            std::printf("stream %u: return codes %d / %d and status %d / %d disagree\n", i, rc, rc2, status, cstatus);
            return 3;
        }
        if (rc == MI355_OK) { ++decoded; for (size_t k = 0; k < px; ++k) sum = sum * 1099511628211ull + out[k]; }
        else ++corrupt;
    }
    std::fclose(f);
    std::printf("jpeg_decode_host_drive ok: %u streams, decoded %ld, refused %ld, corrupt %ld, checksum %016llx\n", count, decoded, refused, corrupt, sum);
    return 0;
}
