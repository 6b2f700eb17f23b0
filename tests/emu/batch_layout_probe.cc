// batch_layout_probe.cc -- TEST ONLY: the batch pipelines' layout rules and launch order (lepton_amd/csrc/lep_batch_layout.h) on numbers a
// test made up; no file is parsed and no byte of a scan is read.  tests/test_batch_layout.py builds it as a library; with
// -DBATCH_LAYOUT_MAIN it is a program of its own that walks every rule once (for a run under -fsanitize=address,undefined).  Never
// linked into the product.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../lepton_amd/csrc/lep_batch_layout.h"

using namespace lepbatch;

// in, per image: route, scan_len, restarts, mcuv, ref_len, prow_need, nscans, then {scan_len, restarts, ref_len} x nscans.
// out, per image: scan_off, table_off, ref_off, row_off, then {off, table_off, ref_off} x nscans; behind all images: scan_total, rows_total.
// Returns how many numbers were written.
extern "C" int emu_scan_arena(const int64_t* in, int nimg, int verify, int64_t* out) {
    std::vector<ScanArenaImage> imgs((size_t)nimg);
    for (ScanArenaImage& im : imgs) {
        im.route = (Route)in[0]; im.scan_len = (uint32_t)in[1]; im.restarts = (size_t)in[2]; im.mcuv = (int32_t)in[3];
        im.ref_len = (uint32_t)in[4]; im.prow_need = (int32_t)in[5];
        im.scans.resize((size_t)in[6]);
        in += 7;
        for (ScanPlace& sc : im.scans) { sc.scan_len = (uint32_t)in[0]; sc.restarts = (size_t)in[1]; sc.ref_len = (uint32_t)in[2]; in += 3; }
    }
    const ScanArenaTotals t = lay_out_scan_arena(imgs.data(), imgs.size(), verify != 0);
    int64_t* o = out;
    for (const ScanArenaImage& im : imgs) {
        *o++ = (int64_t)im.scan_off; *o++ = (int64_t)im.table_off; *o++ = (int64_t)im.ref_off; *o++ = (int64_t)im.row_off;
        for (const ScanPlace& sc : im.scans) { *o++ = (int64_t)sc.off; *o++ = (int64_t)sc.table_off; *o++ = (int64_t)sc.ref_off; }
    }
    *o++ = (int64_t)t.scan_total; *o++ = (int64_t)t.rows_total;
    return (int)(o - out);
}

extern "C" uint64_t emu_restart_table_bytes(uint64_t n) { return restart_table_bytes((size_t)n); }
extern "C" uint64_t emu_stream_slot_bytes(uint64_t segment_size, uint64_t frame_blocks, int nseg, int progressive) {
    return stream_slot_bytes((size_t)segment_size, (size_t)frame_blocks, nseg, progressive != 0);
}
extern "C" int emu_download_whole(uint64_t extent, uint64_t live) { return download_whole((size_t)extent, (size_t)live) ? 1 : 0; }

// decompress scan arena of one file: out = {off, slot, bound} x ns, then the arena's bytes
extern "C" void emu_recode_slots(const uint32_t* caps, int ns, uint64_t* out) {
    OutputArena a;
    std::vector<RecodeSlot> r((size_t)ns);
    place_recode_segments(caps, ns, &a, r.data());
    for (int q = 0; q < ns; ++q) { out[3 * q] = r[(size_t)q].off; out[3 * q + 1] = r[(size_t)q].slot; out[3 * q + 2] = r[(size_t)q].bound; }
    out[3 * ns] = a.bytes;
}

// the round-trip check's output arena: out = {cap, off, corr_off} x n, then bytes, correction words
extern "C" void emu_verify_arena(const uint32_t* caps, const uint32_t* ref_len, const uint32_t* corr_cap, int n, uint64_t* out) {
    OutputArena a;
    for (int q = 0; q < n; ++q) {
        const uint32_t cap = verify_out_cap(caps[q], ref_len[q]);
        out[3 * q] = cap; out[3 * q + 1] = a.place(cap); out[3 * q + 2] = a.place_corr(corr_cap[q]);
    }
    out[3 * n] = a.bytes; out[3 * n + 1] = a.corr_words;
}

extern "C" int emu_gpu_answer_stands(const uint32_t* slens, const uint32_t* hslot, const uint32_t* hbound, const uint32_t* pad, const uint32_t* attempted, int ns) {
    std::vector<lep_huff_end> ends((size_t)ns);
    for (int q = 0; q < ns; ++q) { memset(&ends[(size_t)q], 0, sizeof(lep_huff_end)); ends[(size_t)q].pad = (uint16_t)pad[q]; ends[(size_t)q].attempted = attempted[q]; }
    return gpu_answer_stands(slens, hslot, hbound, ends.data(), ns) ? 1 : 0;
}

// chunks[n][3] = {lo, hi, nseg}, chunk k in slot k & 1; out[n][6] = {stream, set, beside, ragged, expect_company, prev_slot}
extern "C" void emu_launch_order(const int64_t* chunks, int n, int dec_overlap, int scan_separate, int whole_call, int32_t* out) {
    LaunchOrder order;
    for (int k = 0; k < n; ++k) {
        const LaunchPlace p = order.step(chunks[3 * k], chunks[3 * k + 1], (int)chunks[3 * k + 2], dec_overlap, scan_separate != 0, whole_call != 0, k & 1);
        const int32_t v[6] = {p.stream, p.set, p.beside, p.ragged, p.expect_company, p.prev_slot};
        memcpy(out + 6 * k, v, sizeof v);
    }
}

// byte offsets (from the frame's first byte) of the component pointers of a four-pointer descriptor, -1 = null
extern "C" void emu_point_components(int ncomp, const uint32_t* blocks, int64_t* out) {
    static char frame[1];
    const int16_t* p[4];
    point_components(p, ncomp, frame, [&](int c) { return blocks[c]; });
    for (int c = 0; c < 4; ++c) out[c] = p[c] ? (int64_t)((const char*)p[c] - frame) : -1;
}

#ifdef BATCH_LAYOUT_MAIN
#define CHECK(x) do { if (!(x)) { fprintf(stderr, "batch_layout_probe: %s fails (line %d)\n", #x, __LINE__); return 1; } } while (0)
int main() {
    // A sequential, B progressive (two scans, the second with 3 restart positions), C sequential with a table, D host
    const int64_t in[] = {1, 1000, 0, 10, 1100, 0, 0,   2, 0, 0, 0, 0, 25, 2,  100, 0, 120,  37, 3, 41,   1, 4097, 20, 7, 5000, 0, 0,   0, 0, 0, 0, 0, 0, 0};
    int64_t out[64];
    for (int verify = 0; verify < 2; ++verify) {
        const int m = emu_scan_arena(in, 4, verify, out);
        CHECK(m == 4 * 4 + 2 * 3 + 2);
        CHECK(out[m - 2] == (verify ? 11952 : 5664) && out[m - 1] == 44);
    }
    CHECK(emu_restart_table_bytes(3) == 16 && emu_restart_table_bytes(0) == 0);
    CHECK(emu_stream_slot_bytes(100000, 1200, 4, 1) == 190720 && emu_stream_slot_bytes(1000, 1200, 4, 1) == 77568);
    CHECK(emu_download_whole(4194304, 1048576) == 1 && emu_download_whole(4194304, 1048575) == 0);
    const uint32_t caps[3] = {50000, 10000, 10000};
    uint64_t r[16];
    emu_recode_slots(caps, 3, r);
    CHECK(r[1] == 38192 && r[3] == 38192 && r[9] == 58192);
    const uint32_t vc[2] = {4096, 100}, vr[2] = {120, 41}, vk[2] = {10, 0};
    emu_verify_arena(vc, vr, vk, 2, r);
    CHECK(r[0] == 184 && r[4] == 192 && r[6] == 304 && r[7] == 10);
    const uint32_t slot[3] = {38192, 10000, 10000}, len[3] = {38191, 10000, 9}, pad[3] = {0, 0, 1}, att[3] = {0, 0, 10000};
    CHECK(emu_gpu_answer_stands(len, slot, caps, pad, att, 3) == 1);
    const int64_t chunks[12] = {1, 2, 7000, 10, 10, 7000, 1, 2, 7000, 10, 10, 7000};
    int32_t lo[24];
    emu_launch_order(chunks, 4, -1, 0, 0, lo);
    CHECK(lo[6] == 1 && lo[7] == 1 && lo[8] == 1 && lo[12] == 1 && lo[14] == 0 && lo[18] == 0 && lo[20] == 1);
    const uint32_t blocks[4] = {600, 150, 150, 0};
    int64_t po[4];
    emu_point_components(3, blocks, po);
    CHECK(po[0] == 0 && po[1] == 76800 && po[2] == 96000 && po[3] == -1);
    printf("batch_layout_probe: ok\n");
    return 0;
}
#endif
