// stage_block_probe.cc -- TEST ONLY: lepbuf::Block (lepton_amd/csrc/lep_block.h), the descriptor block that lep_gpu.hip stages through its
// pinned ring, on parts a test made up: element sizes, counts, alignments, which parts have a source.  tests/test_stage_block.py builds it
// as a library; with -DSTAGE_BLOCK_MAIN it is a program of its own that walks the same rules once (for a run under
// -fsanitize=address,undefined).  Never linked into the product.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../lepton_amd/csrc/lep_block.h"

using namespace lepbuf;

template <size_t N> struct Elem { char b[N]; };

// the element sizes of every descriptor type a workspace of lep_gpu.hip holds (tests/test_stage_block.py WORKSPACES)
#define ELEM_SIZES(X) X(1) X(4) X(8) X(12) X(16) X(20) X(24) X(32) X(36) X(40) X(48) X(168) X(176) X(2208) X(4184) X(4272) X(5552) X(5696)

// One block and one plain Layout from the same parts: part i has count[i] elements of elem[i] bytes at alignment align[i], and is a copy of
// the next count[i] * elem[i] bytes of `src` where sourced[i] is set.  Writes both sets of offsets, then [bytes, padded, upload_bytes] of
// the block and [bytes, padded] of the layout into totals, and pack()'s image into `image` -- which the caller made upload_bytes long
// and not a byte longer.  Returns 0, or -1 for an element size that is not in the list.
extern "C" int emu_stage_block(const uint32_t* elem, const uint64_t* count, const uint32_t* align, const int32_t* sourced, int nparts, const uint8_t* src,
                               uint64_t* off_block, uint64_t* off_layout, uint64_t* totals, uint8_t* image) {
    Block B;
    Layout L;
    for (int i = 0; i < nparts; ++i) {
        const size_t n = (size_t)count[i], a = (size_t)align[i];
        switch (elem[i]) {
#define CASE(N)                                                                                                           \
    case N:                                                                                                               \
        off_block[i] = sourced[i] ? B.add(reinterpret_cast<const Elem<N>*>(src), n, a) : B.add<Elem<N>>(n, a);            \
        off_layout[i] = L.add<Elem<N>>(n, a);                                                                             \
        break;
            ELEM_SIZES(CASE)
#undef CASE
            default: return -1;
        }
        if (sourced[i]) src += n * elem[i];
    }
    totals[0] = B.bytes(); totals[1] = B.padded(); totals[2] = B.upload_bytes(); totals[3] = L.bytes(); totals[4] = L.padded();
    if (image) B.pack(reinterpret_cast<char*>(image));
    return 0;
}

#ifdef STAGE_BLOCK_MAIN
#define CHECK(x) do { if (!(x)) { fprintf(stderr, "stage_block_probe: %s fails (line %d)\n", #x, __LINE__); return 1; } } while (0)
// stdin: one block per line -- nparts, then elem count align sourced per part.  Every block is packed into a heap buffer of exactly
// upload_bytes (the sanitizer sees a byte written behind it) and compared with the parts copied one by one into a zeroed buffer.
int main() {
    int nparts, blocks = 0;
    while (scanf("%d", &nparts) == 1) {
        std::vector<uint32_t> elem((size_t)nparts), align((size_t)nparts);
        std::vector<uint64_t> count((size_t)nparts), ob((size_t)nparts), ol((size_t)nparts);
        std::vector<int32_t> sourced((size_t)nparts);
        size_t src_bytes = 0;
        for (int i = 0; i < nparts; ++i) {
            unsigned long long c;
            CHECK(scanf("%u %llu %u %d", &elem[(size_t)i], &c, &align[(size_t)i], &sourced[(size_t)i]) == 4);
            count[(size_t)i] = c;
            if (sourced[(size_t)i]) src_bytes += (size_t)c * elem[(size_t)i];
        }
        uint8_t* src = (uint8_t*)malloc(src_bytes ? src_bytes : 1);
        for (size_t k = 0; k < src_bytes; ++k) src[k] = (uint8_t)(1 + (k * 131 + (size_t)blocks) % 255);   // never zero: a gap shows
        uint64_t t[5];
        CHECK(emu_stage_block(elem.data(), count.data(), align.data(), sourced.data(), nparts, src, ob.data(), ol.data(), t, nullptr) == 0);
        CHECK(t[0] == t[3] && t[1] == t[4] && t[2] <= t[0]);
        uint8_t* image = (uint8_t*)malloc(t[2] ? (size_t)t[2] : 1);
        uint8_t* want = (uint8_t*)calloc(t[2] ? (size_t)t[2] : 1, 1);
        memset(image, 0xEE, t[2] ? (size_t)t[2] : 1);
        CHECK(emu_stage_block(elem.data(), count.data(), align.data(), sourced.data(), nparts, src, ob.data(), ol.data(), t, t[2] ? image : image + 1) == 0);
        uint64_t last_end = 0;
        const uint8_t* s = src;
        for (int i = 0; i < nparts; ++i) {
            CHECK(ob[(size_t)i] == ol[(size_t)i] && ob[(size_t)i] % align[(size_t)i] == 0);
            const size_t bytes = (size_t)count[(size_t)i] * elem[(size_t)i];
            if (!sourced[(size_t)i]) continue;
            if (bytes) { memcpy(want + ob[(size_t)i], s, bytes); last_end = ob[(size_t)i] + bytes; }
            s += bytes;
        }
        CHECK(t[2] == last_end);
        CHECK(memcmp(image, want, (size_t)t[2]) == 0);
        if (!t[2]) CHECK(image[0] == 0xEE);
        free(src); free(image); free(want);
        ++blocks;
    }
    printf("ok %d\n", blocks);
    return 0;
}
#endif
