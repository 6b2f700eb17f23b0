// prog_cut_host_main.cc -- TEST ONLY: a program of its own (built with AddressSanitizer and UBSan by tests/test_progressive_cut_sanitizers.py)
// around the HOST code of the cut progressive files: parse_jpeg_prepare_gpu_progressive, parse_jpeg_finish_gpu_progressive (jpeg_scan.cc) and
// progressive_plan (jpeg_progressive.cc), fed with the records the emulated window decoder leaves (prog_cut_driver.h).
//   prog_cut_host <file.jpg> <first cut> <stride>
// For every cut jpg[:p] the host parser accepts: the frame, the hand-off rows and the truncation bookkeeping the finish step rebuilds must
// be the host parser's, and the scan writers' plan must take the file with a region that holds the cut scan written whole.
// Prints "ok <accepted> <declined> <kept by the host by rule>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#define LEP_DEV inline
#include "../../lepton_amd/csrc/lep_derive.h"
#include "prog_cut_driver.h"
#include "../../lepton_amd/csrc/jpeg_model.h"
#include "../../lepton_amd/csrc/lep_container.h"

static_assert(sizeof(lep::ProgScanDecodePlan) == sizeof(lephuff::ProgDecScan) && sizeof(lep::ScanDecodeRow) == sizeof(lephuff::HuffDecRow), "the kernels' descriptors mirror the host's");

static int fail(const char* what, long p) { printf("FAILED at cut %ld: %s\n", p, what); return 1; }

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> jpg;
    uint8_t buf[65536];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) jpg.insert(jpg.end(), buf, buf + n);
    fclose(f);
    long accepted = 0, declined = 0, kept = 0;
    for (long p = atol(argv[2]); p + 3 <= (long)jpg.size(); p += atol(argv[3])) {
        // (exactly p bytes on the heap: a read behind the cut is a finding)
        std::vector<uint8_t> cut(jpg.begin(), jpg.begin() + p);
        lep::JpegFile host;
        if (lep::parse_jpeg(cut.data(), cut.size(), true, &host)) continue;
        lep::JpegFile jf;
        lep::ScanDecodePlan plan1;
        bool ok1 = false, ok = false;
        if (lep::parse_jpeg_prepare_gpu(cut.data(), cut.size(), &jf, &plan1, &ok1) || ok1) return fail("not a progressive file", p);
        std::vector<lep::ProgScanDecodePlan> scans;
        int need = 0;
        if (lep::parse_jpeg_prepare_gpu_progressive(&jf, &scans, &need, &ok, true)) return fail("prepare", p);
        if (!ok) {   // what stays with the host by rule: a last scan without a byte of data, a restart interval
            if (jf.rsti > 0 || jf.scan_start.empty() || jf.scan_start.back() >= jf.scan.size()) { ++kept; continue; }
            return fail("not eligible", p);
        }
        std::vector<std::vector<int16_t>> planes((size_t)jf.ncomp);
        for (int c = 0; c < jf.ncomp; ++c) planes[(size_t)c].assign((size_t)jf.comp[c].bc * 64, 0);
        for (auto& sc : scans) for (int c = 0; c < jf.ncomp; ++c) sc.t.blocks[c] = planes[(size_t)c].data();
        std::vector<lep::ScanDecodeRow> rows((size_t)need);
        int32_t taken = 0, none = 0;
        if (emu_prog_cut_decode(reinterpret_cast<const lephuff::ProgDecScan*>(scans.data()), (int)scans.size(), jf.scan.data(), jf.scan.size(), true, false, false,
                                reinterpret_cast<lephuff::HuffDecRow*>(rows.data()), &taken, &none)) return fail("the driver", p);
        if (lep::parse_jpeg_finish_gpu_progressive(&jf, scans, rows.data())) {
            if (!host.cut_block_irregular) return fail("declined a cut whose final block decoded", p);
            ++declined;
            continue;
        }
        ++accepted;
        for (int c = 0; c < jf.ncomp; ++c) {
            if (memcmp(planes[(size_t)c].data(), host.plane[c], planes[(size_t)c].size() * 2)) return fail("frame", p);
            if (jf.max_dpos[c] != host.max_dpos[c] || jf.trunc_bc[c] != host.trunc_bc[c] || jf.trunc_bcv[c] != host.trunc_bcv[c]) return fail("max_dpos / truncation", p);
        }
        if (jf.padbit != host.padbit || jf.scan_count != host.scan_count || jf.max_cmp != host.max_cmp || jf.max_bpos != host.max_bpos || jf.max_sah != host.max_sah)
            return fail("pad bit / scan bookkeeping", p);
        if (jf.rows.size() != host.rows.size()) return fail("number of hand-off rows", p);
        for (size_t i = 0; i < jf.rows.size(); ++i) {
            const lep::Handoff &a = jf.rows[i], &b = host.rows[i];
            if (a.segment_size != b.segment_size || memcmp(a.last_dc, b.last_dc, sizeof a.last_dc) || a.luma_y_start != b.luma_y_start || a.luma_y_end != b.luma_y_end ||
                a.num_overhang_bits != b.num_overhang_bits || a.overhang_byte != b.overhang_byte) return fail("a hand-off row", p);
        }
        lep::ProgPlan wp;
        if (lep::progressive_plan(&host, cut.size(), false, &wp, true) || !wp.gpu_ok || wp.scans.size() != scans.size()) return fail("the scan writers' plan", p);
        for (const auto& sc : wp.scans) if (sc.file_bound < wp.scans.back().out_cap || sc.file_bound < cut.size()) return fail("the file's region", p);
    }
    printf("ok %ld %ld %ld\n", accepted, declined, kept);
    return 0;
}
