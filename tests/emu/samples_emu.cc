// lep_samples.h's wavefront routines (the bodies of lep_samples_kernel / lep_samples_dc_kernel) stepped through the 64-lane emulation
// of lep_wave.h on the CPU, unit after unit, as a program of its own (tests/test_samples_emulation.py builds it with AddressSanitizer
// and UBSan).  Frames, planes and the tile are heap blocks of exactly their size -- a plane ends with the last sample of its last row --,
// so a load or a store outside them is seen; planes start filled with 0xEE and are written out whole.
//   samples_emu <cases> <out>
// <cases>: int32 count, then per case int32 scale, planes and per plane int32 width_blocks, height_blocks, row_first, row_end, pitch,
// uint16 q[64] (zig-zag order), int16 blocks[width_blocks * height_blocks * 64].  <out>: per case and plane the plane's bytes,
// (height - 1) * pitch + width of them.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../lepton_amd/csrc/lep_samples.h"

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
        int32_t scale = 0, planes = 0;
        if (!get(in, &scale) || !get(in, &planes) || (scale != 1 && scale != 8) || planes < 1) return 2;
        std::vector<lepsamples::PlaneRec> recs((size_t)planes);
        std::vector<uint32_t> first((size_t)planes + 1, 0u);
        std::vector<int16_t*> frames;
        std::vector<uint8_t*> bufs;
        std::vector<size_t> sizes;
        for (int32_t p = 0; p < planes; ++p) {
            int32_t g[5];
            uint16_t q[64];
            if (!get(in, g, 5) || !get(in, q, 64)) return 2;
            const size_t coefs = (size_t)g[0] * (size_t)g[1] * 64;
            int16_t* frame = static_cast<int16_t*>(aligned_alloc(16, coefs * 2));   // (a multiple of 128 bytes, and exactly this long)
            if (!get(in, frame, coefs)) return 2;
            const size_t w = (size_t)g[0] * 8 / (size_t)scale, h = (size_t)g[1] * 8 / (size_t)scale;
            const size_t bytes = (h - 1) * (size_t)g[4] + w;
            uint8_t* plane = static_cast<uint8_t*>(malloc(bytes));
            memset(plane, 0xEE, bytes);
            first[(size_t)p + 1] = first[(size_t)p] + (uint32_t)lepsamples::fill_plane(&recs[(size_t)p], frame, plane, g[0], g[4], g[2], g[3], q, scale);
            frames.push_back(frame); bufs.push_back(plane); sizes.push_back(bytes);
        }
        for (uint32_t unit = 0; unit < first[(size_t)planes]; ++unit, ++units_run) {
            if (scale == 8) { lepsamples::wave_samples_dc(recs.data(), first.data(), planes, unit); continue; }
            uint32_t* tile = static_cast<uint32_t*>(malloc(lepsamples::kTileWords * 4));
            memset(tile, 0x5A, lepsamples::kTileWords * 4);   // what another unit left there
            lepsamples::wave_samples(recs.data(), first.data(), planes, unit, tile);
            free(tile);
        }
        for (int32_t p = 0; p < planes; ++p) {
            if (fwrite(bufs[(size_t)p], 1, sizes[(size_t)p], out) != sizes[(size_t)p]) return 2;
            free(frames[(size_t)p]); free(bufs[(size_t)p]);
        }
    }
    fclose(in);
    if (fclose(out)) return 2;
    printf("ok %ld\n", units_run);
    return 0;
}
