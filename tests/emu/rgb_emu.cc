// lep_rgb.h's wavefront routine (the body of lep_rgb_kernel) stepped through the 64-lane emulation of lep_wave.h on the CPU, unit after
// unit, as a program of its own (tests/test_rgb_emulation.py builds it with AddressSanitizer and UBSan).  Planes and outputs are heap
// blocks of exactly their size -- a plane ends with sample dw - 1 of its row dh - 1, an output with the last pixel of its last row --, so
// a load or a store outside them is seen; outputs start filled with 0xEE and are written out whole.
//   rgb_emu <cases> <out>
// <cases>: int32 count, then per case int32 images and per image int32 width, height, ncomp, convert, h_samp[3], v_samp[3],
// plane_pitch[3], rgb_pitch, y_first, y_end, then per component its (dh - 1) * pitch + dw bytes.  <out>: per case and image the output's
// bytes, (height - 1) * rgb_pitch + width * (ncomp == 1 ? 1 : 3) of them.  An image fill_image refuses ends the program with status 3.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../lepton_amd/csrc/lep_rgb.h"

template <class T>
static bool get(FILE* f, T* v, size_t n = 1) { return fread(v, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t cases = 0;
    if (!get(in, &cases)) return 2;
    long units_run = 0;
    for (int32_t k = 0; k < cases; ++k) {
        int32_t images = 0;
        if (!get(in, &images) || images < 1) return 2;
        std::vector<leprgb::RgbRec> recs((size_t)images);
        std::vector<uint32_t> first((size_t)images + 1, 0u);
        std::vector<uint8_t*> blocks;
        std::vector<uint8_t*> outs;
        std::vector<size_t> sizes;
        for (int32_t i = 0; i < images; ++i) {
            int32_t g[4], hs[3], vs[3], pitch[3], tail[3];
            if (!get(in, g, 4) || !get(in, hs, 3) || !get(in, vs, 3) || !get(in, pitch, 3) || !get(in, tail, 3)) return 2;
            const uint8_t* none[3] = {nullptr, nullptr, nullptr};
            leprgb::RgbRec geo;   // the geometry first: it says how long the planes are
            if (leprgb::fill_image(&geo, g[0], g[1], g[2], hs, vs, g[3], none, pitch, nullptr, tail[0], tail[1], tail[2]) < 0) return 3;
            const uint8_t* planes[3] = {nullptr, nullptr, nullptr};
            for (int c = 0; c < g[2]; ++c) {
                const size_t bytes = (size_t)(geo.dh[c] - 1) * (size_t)pitch[c] + (size_t)geo.dw[c];
                uint8_t* p = static_cast<uint8_t*>(malloc(bytes));
                if (!get(in, p, bytes)) return 2;
                planes[c] = p;
                blocks.push_back(p);
            }
            const size_t bytes = (size_t)(g[1] - 1) * (size_t)tail[0] + (size_t)g[0] * (g[2] == 1 ? 1 : 3);
            uint8_t* rgb = static_cast<uint8_t*>(malloc(bytes));
            memset(rgb, 0xEE, bytes);
            first[(size_t)i + 1] = first[(size_t)i] + (uint32_t)leprgb::fill_image(&recs[(size_t)i], g[0], g[1], g[2], hs, vs, g[3], planes, pitch, rgb, tail[0], tail[1], tail[2]);
            outs.push_back(rgb); sizes.push_back(bytes);
        }
        for (uint32_t unit = 0; unit < first[(size_t)images]; ++unit, ++units_run) leprgb::wave_rgb(recs.data(), first.data(), images, unit);
        for (int32_t i = 0; i < images; ++i) {
            if (fwrite(outs[(size_t)i], 1, sizes[(size_t)i], out) != sizes[(size_t)i]) return 2;
            free(outs[(size_t)i]);
        }
        for (uint8_t* p : blocks) free(p);
    }
    fclose(in);
    if (fclose(out)) return 2;
    printf("ok %ld\n", units_run);
    return 0;
}
