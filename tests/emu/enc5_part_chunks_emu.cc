// enc5_part_chunks_emu.cc -- TEST ONLY, a program of its own (tests/test_enc5_part_chunks_emulation.py builds it with g++, with
// AddressSanitizer and UBSan where their runtime exists): the stitched bool writer of lep_enc5.h with its chunks cut at the boundaries
// of gather's parts (part_chunk_cut / wchunk_range_cut / wchunk_link_cuts / wchunk_code_cut, then ONE wchunk_stitch_lane over all
// nparts * c chunks), run part by part the way the GPU launches it: while part p's chunks are ranged, linked and coded, the bins of the
// parts behind it are not there yet (here: poison).
//   enc5_part_chunks lists <trials>     random and adversarial bin lists, cut at random part bounds, against lepdev::BoolCoder<false>
//   enc5_part_chunks frames <file>...   whole segments: count -> emit -> fold -> gather in P parts -> the per-part chunk phases, with one
//                                       and two wavefronts per segment, against the serial coder over the gathered list AND the stream
//                                       the file carries (the oracle's)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#define LEP_DEV inline
#include "../../lepton_amd/csrc/lep_derive.h"
#include "lep_core_coder.h"
using namespace lepdev;
#include "../../lepton_amd/csrc/lep_enc5.h"

static uint64_t rs = 0x2545F4914F6CDD1Dull;
static uint32_t rnd() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return (uint32_t)(rs >> 11); }

// The per-part sequence over `bins` (n of them, B[0..P] the parts' first bins): bytes, length and verdict into out / len / status;
// returns how many chunks the link pass had to redo.  `ck` is a checkpoint table as emit leaves it (only nbins is read).
static int run_part_chunks(const std::vector<uint16_t>& bins, uint32_t n, const uint32_t* B, int P, int c, uint32_t warm, uint32_t cap,
                           std::vector<uint8_t>& out, uint32_t* len, int32_t* status) {
    using namespace lep5;
    SegPlan5 plan;
    memset(&plan, 0, sizeof plan);
    SegDev sd;
    memset(&sd, 0, sizeof sd);
    sd.stream_cap = cap;
    Ckpt5 ck[kMaxParts];
    memset(ck, 0xEE, sizeof ck);
    for (int p = 1; p < P; ++p) ck[p].nbins = B[p];
    plan.nbins = 0xEEEEEEEEu;   // (gather's last part writes it: nothing may ask for it before)
    const int K = P * c;
    std::vector<WChunk5> recs((size_t)K);
    memset(recs.data(), 0xEE, recs.size() * sizeof(WChunk5));
    std::vector<uint16_t> work(bins.size(), 0xA5A5);   // the list as the writer sees it: a part's bins appear when the part is gathered
    int redone = 0;
    for (int p = 0; p < P; ++p) {
        for (uint32_t i = B[p]; i < B[p + 1]; ++i) work[i] = bins[i];
        if (p + 1 == P) plan.nbins = n;
        for (int s = 0; s < c; ++s) wchunk_range_cut(plan, work.data(), &recs[(size_t)(p * c + s)], part_chunk_cut(plan, ck, p, s, P, c), warm);
        wchunk_link_cuts(plan, work.data(), recs.data(), p * c, (p + 1) * c, [&](int j) { return part_chunk_cut(plan, ck, j / c, j % c, P, c); });
        for (int s = 0; s < c; ++s) redone += (p * c + s) > 0 && recs[(size_t)(p * c + s)].q_guess != recs[(size_t)(p * c + s)].q_start;
        for (int s = c - 1; s >= 0; --s) wchunk_code_cut(plan, work.data(), sd, out.data(), &recs[(size_t)(p * c + s)], part_chunk_cut(plan, ck, p, s, P, c));
    }
    wchunk_stitch_lane(plan, sd, out.data(), len, status, recs.data(), K);
    return redone;
}

static int check_lists(int trials) {
    std::vector<uint8_t> a(1 << 17), b(1 << 17);
    int with_redo = 0, without_redo = 0, empty_parts = 0, short_parts = 0, overflows = 0;
    for (int trial = 0; trial < trials; ++trial) {
        const uint32_t n = rnd() % (trial % 7 == 0 ? 40000u : 3000u);
        const int mode = trial % 6;
        std::vector<uint16_t> bins((size_t)n + 256, 0);
        for (uint32_t i = 0; i < n; ++i) {
            uint32_t p, bit;
            if (mode == 0) { p = rnd() % 256; bit = rnd() & 1; }
            else if (mode == 1) { p = 1 + rnd() % 3; bit = (rnd() % 8) != 0; }
            else if (mode == 2) { p = 250 + rnd() % 6; bit = (rnd() % 8) == 0; }
            else if (mode == 3) { p = 128; bit = 1; }
            else if (mode == 4) { p = rnd() % 256; bit = (rnd() % 256) < p ? 0 : 1; }
            else { p = (rnd() & 1) ? 255 : 1; bit = rnd() & 1; }
            bins[i] = (uint16_t)(p | (bit << 8));
        }
        const uint32_t cap = (trial % 50 == 0) ? rnd() % 200 : 1u << 17;
        memset(a.data(), 0xAA, a.size()); memset(b.data(), 0xBB, b.size());
        BoolCoder<false> ref;
        ref.init_stream(a.data(), cap);
        for (uint32_t i = 0; i < n; ++i) ref.put(bins[i] >> 8, bins[i] & 255);
        const uint32_t la = ref.finish();
        const int P = 1 + (int)(rnd() % 8), c = 1 << (rnd() % 6);
        const uint32_t warms[5] = {8, 64, 700, 16384, 1u << 20};
        const uint32_t warm = warms[rnd() % 5];
        // part bounds: sorted random places; every third trial some neighbours made equal (empty parts), every fifth the bounds crowded
        // into a stretch of a few bins (parts far shorter than any warm-up)
        uint32_t B[lep5::kMaxParts + 1];
        B[0] = 0; B[P] = n;
        const uint32_t span = (trial % 5 == 0) ? (n < 40 ? n : 40) : n, from = n > span ? rnd() % (n - span + 1) : 0;
        for (int p = 1; p < P; ++p) B[p] = from + (span ? rnd() % (span + 1) : 0);
        for (int p = 1; p < P; ++p) for (int q = p + 1; q < P; ++q) if (B[q] < B[p]) { const uint32_t t = B[p]; B[p] = B[q]; B[q] = t; }
        if (trial % 3 == 0) for (int p = 1; p < P; ++p) if (rnd() & 1) B[p] = B[p + 1];
        for (int p = 0; p < P; ++p) { empty_parts += B[p] == B[p + 1]; short_parts += B[p + 1] - B[p] > 0 && B[p + 1] - B[p] < 8; }
        uint32_t lb = 0;
        int32_t stt = 0;
        const int redone = run_part_chunks(bins, n, B, P, c, warm, cap, b, &lb, &stt);
        if (P * c > 1) { if (redone) ++with_redo; else ++without_redo; }
        const bool ov = stt == 100;
        overflows += ov;
        if (ref.overflow != ov) { printf("trial %d (n %u P %d c %d warm %u cap %u): verdict %d, serial %d\n", trial, n, P, c, warm, cap, (int)ov, (int)ref.overflow); return 1; }
        if (!ov && (la != lb || memcmp(a.data(), b.data(), la))) { printf("trial %d (n %u P %d c %d warm %u): bytes differ (len %u, serial %u)\n", trial, n, P, c, warm, lb, la); return 1; }
    }
    printf("ok lists %d with_redo %d without_redo %d empty_parts %d short_parts %d overflows %d\n", trials, with_redo, without_redo, empty_parts, short_parts, overflows);
    return 0;
}

// a frame file (written by the test): lep_image_desc up to its pointers | the components' blocks | y0 y1 is_last | length and bytes of
// the stream the oracle makes of the segment
struct FrameFile {
    lep_image_desc d;
    std::vector<std::vector<int16_t>> blocks;
    int32_t seg[3];
    std::vector<uint8_t> want;
    bool read(const char* fn) {
        FILE* f = fopen(fn, "rb");
        if (!f) return false;
        memset(&d, 0, sizeof d);
        bool ok = fread(&d, offsetof(lep_image_desc, blocks), 1, f) == 1 && d.ncomp >= 1 && d.ncomp <= LEP_MAX_COMPONENTS;
        blocks.resize(ok ? (size_t)d.ncomp : 0);
        for (int c = 0; ok && c < d.ncomp; ++c) {
            const size_t nb = (size_t)d.width_blocks[c] * (size_t)d.height_blocks[c];
            blocks[(size_t)c].resize(nb * 64);
            ok = fread(blocks[(size_t)c].data(), 128, nb, f) == nb;
            d.blocks[c] = blocks[(size_t)c].data();
        }
        uint32_t wl = 0;
        ok = ok && fread(seg, 4, 3, f) == 3 && fread(&wl, 4, 1, f) == 1 && wl < (1u << 26);
        if (ok) { want.resize(wl); ok = wl == 0 || fread(want.data(), 1, wl, f) == wl; }
        fclose(f);
        return ok;
    }
};

// encode_segment_v5 of core_emu.cc up to the gather parts, then the per-part chunk phases in place of write_wave; after every gather
// part the chunk phases of that part run on the list as it is then (the later parts' bins still poison)
template <int NW>
static int frame_part_chunks(const FrameFile& ff, int nparts, int c, uint32_t warm, uint32_t cap, int* redone_out) {
    using namespace lep5;
    ImageDev img;
    int rc = derive_image(ff.d, &img, true);
    if (rc) return rc;
    std::vector<NSum> ns(img.ns_total);
    SegDev seg;
    memset(&seg, 0, sizeof seg);
    seg.image = 0; seg.y0 = ff.seg[0]; seg.y1 = ff.seg[1]; seg.is_last = ff.seg[2]; seg.stream_off = 0; seg.stream_cap = cap; seg.slot = 0;
    static Walk5Shared wsh;
    static FoldShared fsh;
    std::vector<uint32_t> counts(kCountWords, 0);
    static SegPlan5 plan;
    {
        Walk5<kCount, NW> w;
        memset(ns.data(), 0, ns.size() * sizeof(NSum));
        w.run(&img, seg, ns.data(), &wsh, &plan, nullptr, nullptr);
        export_counts(w, &wsh, counts.data());
    }
    plan_segment(counts.data(), &plan);
    std::vector<uint8_t> arena(plan.arena_bytes + 64, 0xA5);
    std::vector<uint16_t> binlist(plan.bins_cap + 64, 0xA5A5);
    {
        Walk5<kEmit, NW> w;
        memset(ns.data(), 0, ns.size() * sizeof(NSum));
        rc = w.run(&img, seg, ns.data(), &wsh, &plan, arena.data(), nullptr, 0, 0, nparts);
        if (rc) return rc;
    }
    {
        static BucketShared bsh;
        bucket_wave(&plan, arena.data(), &bsh);
    }
    std::vector<uint32_t> thresh(kThreshWords, kBranchInit);
    for (int ci = 0; ci < 2; ++ci) {
        for (int row = 0; row < kRows; ++row)
            for (int k = 0; k < kClasses; ++k) {
                const int sid = stream_id(ci, row, k);
                if (!plan.cnt[sid]) continue;
                if (row < 63) fold_coef_wave(&plan, arena.data(), 0, 1, sid, &fsh);
                else fold_thresh_wave(&plan, arena.data(), thresh.data(), 0, 1, sid, ci, &fsh);
            }
        fold_sign_wave(&plan, arena.data(), 0, 1, ci, &fsh);
        for (int b = 0; b < 10; ++b) fold_nz_wave(&plan, arena.data(), 0, 1, ci, b, &fsh);
        for (int v = 0; v < 2; ++v) for (int e = 0; e < 8; ++e) fold_edgenz_wave(&plan, arena.data(), 0, 1, ci, v, e, &fsh);
    }
    for (int a = 0; a < 12; ++a) fold_dc_wave(&plan, arena.data(), 0, 1, a, &fsh);
    const Ckpt5* ck = reinterpret_cast<const Ckpt5*>(arena.data() + plan.ckpt_base);
    const int K = nparts * c;
    std::vector<WChunk5> recs((size_t)K);
    memset(recs.data(), 0xEE, recs.size() * sizeof(WChunk5));
    std::vector<uint8_t> out((size_t)cap + 64, 0x5A);
    int redone = 0;
    plan.nbins = 0xEEEEEEEEu;
    for (int part = 0; part < nparts; ++part) {
        Walk5<kGather, NW> w;
        memset(ns.data(), 0, ns.size() * sizeof(NSum));
        rc = w.run(&img, seg, ns.data(), &wsh, &plan, arena.data(), binlist.data(), 0, part, nparts);
        if (rc) return rc;
        if (w.nbins > plan.bins_cap) return 1003;
        if (part + 1 == nparts) plan.nbins = w.nbins;   // (as lep_enc5_walk_kernel does)
        for (int s = 0; s < c; ++s) wchunk_range_cut(plan, binlist.data(), &recs[(size_t)(part * c + s)], part_chunk_cut(plan, ck, part, s, nparts, c), warm);
        wchunk_link_cuts(plan, binlist.data(), recs.data(), part * c, (part + 1) * c, [&](int j) { return part_chunk_cut(plan, ck, j / c, j % c, nparts, c); });
        for (int s = 0; s < c; ++s) redone += (part * c + s) > 0 && recs[(size_t)(part * c + s)].q_guess != recs[(size_t)(part * c + s)].q_start;
        for (int s = 0; s < c; ++s) wchunk_code_cut(plan, binlist.data(), seg, out.data(), &recs[(size_t)(part * c + s)], part_chunk_cut(plan, ck, part, s, nparts, c));
    }
    uint32_t slen = 0;
    int32_t status = 0;
    wchunk_stitch_lane(plan, seg, out.data(), &slen, &status, recs.data(), K);
    // the serial coder over the list gather left
    std::vector<uint8_t> ser((size_t)cap + 64, 0xAA);
    BoolCoder<false> ref;
    ref.init_stream(ser.data(), cap);
    for (uint32_t i = 0; i < plan.nbins; ++i) ref.put(binlist[i] >> 8, binlist[i] & 255);
    const uint32_t la = ref.finish();
    if (ref.overflow != (status == 100)) return 1006;
    if (status != 100) {
        if (la != slen || memcmp(ser.data(), out.data(), la)) return 1007;
        if (slen != ff.want.size() || memcmp(out.data(), ff.want.data(), slen)) return 1008;   // the oracle's stream
    }
    *redone_out += redone;
    return status == 100 ? 100 : status;
}

static int check_frames(int nfiles, char** files) {
    static const int shapes[6][2] = {{8, 1}, {8, 4}, {3, 2}, {1, 8}, {5, 8}, {2, 32}};   // (parts, chunks per part)
    static const uint32_t warms[3] = {lep5::kWarm5, 8, 100};
    int runs = 0, redone = 0, refused = 0;
    for (int i = 0; i < nfiles; ++i) {
        FrameFile ff;
        if (!ff.read(files[i])) { printf("%s: cannot read\n", files[i]); return 1; }
        const uint32_t room = (uint32_t)ff.want.size() + 4096;
        for (int k = 0; k < 6; ++k) {
            const uint32_t warm = warms[(i + k) % 3];
            for (int nw = 1; nw <= 2; ++nw, ++runs) {
                const int rc = nw == 1 ? frame_part_chunks<1>(ff, shapes[k][0], shapes[k][1], warm, room, &redone) : frame_part_chunks<2>(ff, shapes[k][0], shapes[k][1], warm, room, &redone);
                if (rc) { printf("%s: %d parts x %d chunks, %d wavefront(s), warm-up %u: %d\n", files[i], shapes[k][0], shapes[k][1], nw, warm, rc); return 1; }
            }
        }
        // a buffer too small for the stream: the verdict of the serial coder (status 100), whatever the cut
        if (ff.want.size() > 8) {
            const int rc = frame_part_chunks<2>(ff, 8, 4, lep5::kWarm5, (uint32_t)ff.want.size() / 2, &redone);
            if (rc != 100) { printf("%s: half the room: %d, not 100\n", files[i], rc); return 1; }
            ++refused;
        }
    }
    printf("ok frames %d runs %d redone %d refused %d\n", nfiles, runs, redone, refused);
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 3 && !strcmp(argv[1], "lists")) return check_lists(atoi(argv[2]));
    if (argc >= 3 && !strcmp(argv[1], "frames")) return check_frames(argc - 2, argv + 2);
    printf("usage: enc5_part_chunks lists <trials> | frames <file>...\n");
    return 2;
}
