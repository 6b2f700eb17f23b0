"""lep_gpu_pack_device's copy routine (lepton_amd/csrc/lep_pack.h copy_run, the body of lep_pack_copy_kernel) stepped lane by lane on the
CPU (tests/emu/pack_copy_emu.cc), as a program of its own built with AddressSanitizer and UBSan: every pair of source and destination
alignments, lengths around the head / dword / tail boundaries and random ones; the destination must hold exactly the run, and no load or
store may leave the aligned dwords that hold bytes of the run (the buffers end there)."""
import os
import subprocess

from conftest import ROOT

MAIN = r"""
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>
extern "C" long emu_pack_copy_run(const uint8_t* run, uint32_t len, int src_shift, int dst_shift);
int main() {
    std::mt19937 rng(17);
    long cases = 0;
    std::vector<uint32_t> lens;
    for (uint32_t k = 0; k <= 300; ++k) lens.push_back(k);
    for (uint32_t k : {4095u, 4096u, 4097u, 65535u, 65537u}) lens.push_back(k);
    for (int k = 0; k < 200; ++k) lens.push_back(rng() % 20000);
    for (uint32_t len : lens) {
        std::vector<uint8_t> run(len + 1);
        for (auto& b : run) b = (uint8_t)rng();
        for (int s = 0; s < 4; ++s)
            for (int d = 0; d < 4; ++d, ++cases) {
                const long bad = emu_pack_copy_run(run.data(), len, s, d);
                if (bad) { printf("len %u src %d dst %d: byte %ld\n", len, s, d, bad - 1); return 1; }
            }
    }
    printf("ok %ld\n", cases);
    return 0;
}
"""


def test_copy_run_lane_by_lane_under_sanitizers(tmp_path):
    main = tmp_path / "main.cc"
    main.write_text(MAIN)
    exe = str(tmp_path / "pack_copy")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-o", exe, str(main), os.path.join(ROOT, "tests", "emu", "pack_copy_emu.cc")]
    if subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-o", str(tmp_path / "probe"), "-"], input="int main() { return 0; }\n",
                      capture_output=True, text=True).returncode != 0:
        cmd = [c for c in cmd if not c.startswith("-fsanitize") and not c.startswith("-fno-sanitize")]   # no sanitizer runtime: the byte checks alone
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout, r.stderr[-3000:])
    assert int(r.stdout.split()[1]) == (301 + 5 + 200) * 16
