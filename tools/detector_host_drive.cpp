// Drives the host arithmetic of the detector's mixed-size path (csrc/engine_internal.h: make_geometry, resize_table;
// csrc/engine_multi.hip: multi_check, multi_prepare, multi_image) over edge shapes: 1 x 1 frames, widths that are no multiple of 4,
// frames larger and smaller than imgsz, padded row strides, equal and mixed shapes, host and device frames, and n of 1, chunk,
// chunk + 1 and 2 * chunk + 1.  It asserts that every staging offset plus the frame's bytes lies inside its staging slot, that every
// descriptor points into the slot of its chunk, and that every table offset plus its length lies inside the table block.  No HIP call
// is made and no device is needed; it is meant to be built with the host sanitizers (the Python tests cannot run under them), with
// engine_multi.hip compiled into it and the rest of the engine taken from the built library:
//
//   cd computer-vision-shoplifting-detection_amd/csrc
//   hipcc -O1 -g --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined engine_multi.hip \
//         ../../tools/detector_host_drive.cpp -L.. -lmi355yolo -Wl,-rpath,$PWD/.. -o /tmp/detector_host_drive
//   /tmp/detector_host_drive
#include "../computer-vision-shoplifting-detection_amd/csrc/engine_internal.h"

#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s (%s)\n", __LINE__, #x, mi355_last_error()); return 1; } } while (0)

static long long g_geoms = 0, g_tables = 0, g_calls = 0, g_refused = 0;

static int drive_geometry(int h0, int w0, int imgsz) {
    for (int auto_pad = 0; auto_pad < 2; ++auto_pad) {
        const Geometry g = make_geometry(h0, w0, imgsz, auto_pad != 0);
        ++g_geoms;
        CHECK(g.h0 == h0 && g.w0 == w0 && g.Hr >= 1 && g.Wr >= 1 && g.Hr <= imgsz && g.Wr <= imgsz);
        CHECK(g.top >= 0 && g.left >= 0 && g.top + g.Hr <= g.Hl && g.left + g.Wr <= g.Wl);
        CHECK(g.Hl % 32 == 0 && g.Wl % 32 == 0 && g.Hl <= imgsz && g.Wl <= imgsz);
        if (!auto_pad) CHECK(g.Hl == imgsz && g.Wl == imgsz);
        CHECK(g.resize == (g.Hr != h0 || g.Wr != w0));
        CHECK(!g.identity || (g.Hl == h0 && g.Wl == w0));
        CHECK(g.gain > 0 && g.pad_x >= 0 && g.pad_y >= 0);
    }
    return 0;
}

static int drive_table(int dn, int sn) {
    std::vector<int> t;
    resize_table(dn, sn, t);
    ++g_tables;
    CHECK(t.size() == (size_t)dn * 3);
    for (int d = 0; d < dn; ++d) {
        CHECK(t[d * 3] >= 0 && t[d * 3] <= sn - 1);
        CHECK(t[d * 3 + 1] + t[d * 3 + 2] == 2048 && t[d * 3 + 1] >= 0 && t[d * 3 + 2] >= 0);
        CHECK(t[d * 3 + 2] == 0 || t[d * 3] + 1 <= sn - 1);            // the second tap is read only where it exists
    }
    return 0;
}

struct Shape { int h, w, pad; };                                        // pad: extra bytes per row (0 = dense)

// one call of n frames (shapes taken round robin from `set`) in chunks of `chunk`, host or device frames
static int drive_call(const std::vector<Shape>& set, int n, int chunk, int imgsz, bool on_device, const uint8_t* frame_mem) {
    std::vector<const uint8_t*> frames(n, frame_mem);
    std::vector<int> hs(n), ws(n), rs(n);
    bool any_pad = false;
    for (int i = 0; i < n; ++i) {
        const Shape& s = set[i % set.size()];
        hs[i] = s.h; ws[i] = s.w; rs[i] = s.pad ? s.w * 3 + s.pad : 0; any_pad |= s.pad != 0;
    }
    const MultiFrames mf{frames.data(), hs.data(), ws.data(), any_pad ? rs.data() : nullptr, on_device};
    CHECK(multi_check(mf, n) == MI355_OK);
    const int nb = std::min(n, chunk);
    MultiCall mc;
    multi_prepare(mf, n, nb, imgsz, mc);
    ++g_calls;
    bool same = true;
    for (int i = 1; i < n; ++i) same = same && hs[i] == hs[0] && ws[i] == ws[0];
    CHECK((int)mc.g.size() == n && (int)mc.stage_off.size() == n);
    CHECK(same ? (mc.Hd == mc.g[0].Hl && mc.Wd == mc.g[0].Wl) : (mc.Hd == imgsz && mc.Wd == imgsz));
    for (int i = 0; i < n; ++i) {
        const size_t bytes = (size_t)hs[i] * ws[i] * 3;
        CHECK(mc.g[i].Hl == mc.Hd && mc.g[i].Wl == mc.Wd);
        CHECK(mc.stage_off[i] + bytes <= mc.slot_bytes);                                   // the frame lies inside its staging slot
        CHECK(i % nb == 0 ? mc.stage_off[i] == 0 : mc.stage_off[i] >= mc.stage_off[i - 1] + (size_t)hs[i - 1] * ws[i - 1] * 3);    // behind its neighbour
    }
    const uint8_t* staged = reinterpret_cast<const uint8_t*>(uintptr_t(1) << 40);         // never dereferenced: the image only holds addresses
    MultiImage img;
    multi_image(mf, mc, n, nb, staged, img);
    CHECK(img.geom_off >= (size_t)n * sizeof(LetterboxFrame) && img.tabs_off >= img.geom_off + (size_t)n * 7 * sizeof(float));
    CHECK(img.geom_off % 256 == 0 && img.tabs_off % 256 == 0);
    CHECK(img.tabs_off + img.tab_ints * sizeof(int) <= img.bytes.size());                   // the table block lies inside the image
    const LetterboxFrame* desc = reinterpret_cast<const LetterboxFrame*>(img.bytes.data());
    const float* geom = reinterpret_cast<const float*>(img.bytes.data() + img.geom_off);
    const int* tabs = reinterpret_cast<const int*>(img.bytes.data() + img.tabs_off);
    for (int i = 0; i < n; ++i) {
        const LetterboxFrame& f = desc[i];
        const Geometry& g = mc.g[i];
        CHECK(f.H == hs[i] && f.W == ws[i] && f.Hr == g.Hr && f.Wr == g.Wr && f.top == g.top && f.left == g.left && f.resize == (g.resize ? 1 : 0));
        if (on_device) CHECK(f.src == frames[i] && f.row_stride == (rs[i] ? rs[i] : ws[i] * 3));
        else {
            const size_t at = (size_t)(f.src - staged), slot = (size_t)((i / nb) & 1) * mc.slot_bytes;
            CHECK(f.row_stride == ws[i] * 3 && at >= slot && at + (size_t)hs[i] * ws[i] * 3 <= slot + mc.slot_bytes);   // inside the slot of its chunk
            CHECK(at == slot + mc.stage_off[i]);
        }
        if (f.resize) {
            CHECK(f.xoff >= 0 && (size_t)f.xoff + 3 * (size_t)f.Wr <= img.tab_ints);       // table offset plus length inside the table block
            CHECK(f.yoff >= 0 && (size_t)f.yoff + 3 * (size_t)f.Hr <= img.tab_ints);
            for (int d = 0; d < f.Wr; ++d) CHECK(tabs[f.xoff + d * 3] >= 0 && tabs[f.xoff + d * 3] < f.W);
            for (int d = 0; d < f.Hr; ++d) CHECK(tabs[f.yoff + d * 3] >= 0 && tabs[f.yoff + d * 3] < f.H);
            for (int j = 0; j < i; ++j)                                                    // frames of one shape share one pair of tables
                if (hs[j] == hs[i] && ws[j] == ws[i]) CHECK(desc[j].xoff == f.xoff && desc[j].yoff == f.yoff);
        } else CHECK(f.xoff == 0 && f.yoff == 0);
        CHECK(geom[i * 7 + 0] == (float)g.gain && geom[i * 7 + 5] == (float)ws[i] && geom[i * 7 + 6] == (float)hs[i]);
    }
    MultiImage again;                                                    // the same call builds the same bytes: what multi_upload compares
    multi_image(mf, mc, n, nb, staged, again);
    CHECK(again.bytes == img.bytes);
    return 0;
}

static int drive_refusals(const uint8_t* frame_mem) {
    const uint8_t* two[2] = {frame_mem, frame_mem};
    const uint8_t* hole[2] = {frame_mem, nullptr};
    const int hs[2] = {48, 48}, ws[2] = {80, 80}, zero[2] = {48, 0}, neg[2] = {-1, 80}, tight[2] = {0, 239}, wide[2] = {240, 4096};
    auto refused = [&](const MultiFrames& mf, int n, const char* msg) {
        ++g_refused;
        return multi_check(mf, n) == MI355_EINVAL && std::strcmp(mi355_last_error(), msg) == 0;
    };
    CHECK(refused(MultiFrames{two, hs, ws, nullptr, false}, 0, "n must be positive"));
    CHECK(refused(MultiFrames{nullptr, nullptr, nullptr, nullptr, false}, -3, "n must be positive"));
    CHECK(refused(MultiFrames{nullptr, hs, ws, nullptr, false}, 2, "null argument"));
    CHECK(refused(MultiFrames{two, nullptr, ws, nullptr, true}, 2, "null argument"));
    CHECK(refused(MultiFrames{two, hs, nullptr, nullptr, false}, 2, "null argument"));
    CHECK(refused(MultiFrames{hole, hs, ws, nullptr, false}, 2, "null frame pointer"));
    CHECK(refused(MultiFrames{two, hs, zero, nullptr, false}, 2, "frame height and width must be positive"));
    CHECK(refused(MultiFrames{two, neg, ws, nullptr, true}, 2, "frame height and width must be positive"));
    CHECK(refused(MultiFrames{two, hs, ws, tight, false}, 2, "row_stride_bytes smaller than a row"));
    CHECK(multi_check(MultiFrames{two, hs, ws, wide, false}, 2) == MI355_OK);
    CHECK(multi_check(MultiFrames{hole, hs, ws, nullptr, false}, 1) == MI355_OK);          // only the first n entries are read
    return 0;
}

int main() {
    static const uint8_t frame_mem[16] = {};                             // a non-null frame pointer; none of the driven code reads a frame
    const std::vector<Shape> shapes = {{1, 1, 0}, {1, 7, 0}, {7, 5, 0}, {37, 53, 3}, {48, 80, 0}, {64, 96, 0}, {80, 96, 24}, {96, 128, 0}, {100, 331, 207},
                                       {240, 320, 0}, {640, 640, 0}, {641, 639, 0}, {720, 1280, 0}, {1080, 1920, 128}, {1081, 1921, 1}, {33, 2000, 0}};
    const int sizes[3] = {32, 96, 640};
    for (int imgsz : sizes)
        for (const Shape& s : shapes) {
            if (drive_geometry(s.h, s.w, imgsz)) return 1;
            const Geometry g = make_geometry(s.h, s.w, imgsz, false);
            if (drive_table(g.Wr, s.w) || drive_table(g.Hr, s.h)) return 1;
        }
    for (int dn = 1; dn <= 40; ++dn) for (int sn = 1; sn <= 40; ++sn) if (drive_table(dn, sn)) return 1;
    // equal shapes (one shape at a time) and mixed shapes (windows of the list, and the whole list)
    std::vector<std::vector<Shape>> sets;
    for (const Shape& s : shapes) sets.push_back({s});
    for (size_t i = 0; i + 3 <= shapes.size(); ++i) sets.push_back({shapes[i], shapes[i + 1], shapes[i + 2]});
    sets.push_back(shapes);
    for (int imgsz : sizes)
        for (const auto& set : sets)
            for (int chunk : {1, 2, 4, 5})
                for (int n : {1, chunk, chunk + 1, 2 * chunk + 1})
                    for (int dev = 0; dev < 2; ++dev)
                        if (drive_call(set, n, chunk, imgsz, dev != 0, frame_mem)) { std::printf("... imgsz %d chunk %d n %d device %d\n", imgsz, chunk, n, dev); return 1; }
    if (drive_refusals(frame_mem)) return 1;
    std::printf("detector host drive ok: %lld geometries, %lld resize tables, %lld calls prepared and imaged, %lld refusals, none out of bounds\n",
                g_geoms, g_tables, g_calls, g_refused);
    return 0;
}
