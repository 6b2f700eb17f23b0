"""lep_gpu_pack_window_device's device code stepped lane by lane on the CPU (tests/emu/pack_window_emu.cc): window_len, which the
offsets kernel applies to the device's lengths, and copy_run started `skip` bytes into the run, as a program of its own built with
AddressSanitizer and UBSan.  Every source and destination alignment; windows that start and end at every offset mod 4; skip equal to
the length, skip beyond it, take 0, a window that ends behind the run.  The destination must hold exactly the window, and no load or
store may leave the aligned dwords that hold bytes of the WINDOW: the buffers start and end there, the rest of the run is not in them."""
import os
import subprocess

from conftest import ROOT

MAIN = r"""
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>
extern "C" long emu_pack_window_run(const uint8_t* run, uint32_t len, uint32_t skip, uint32_t take, int src_shift, int dst_shift);
int main() {
    std::mt19937 rng(23);
    long cases = 0;
    unsigned len, skip, take;
    while (scanf("%u %u %u", &len, &skip, &take) == 3) {
        std::vector<uint8_t> run(len + 1);
        for (auto& b : run) b = (uint8_t)rng();
        for (int s = 0; s < 4; ++s)
            for (int d = 0; d < 4; ++d, ++cases) {
                const long bad = emu_pack_window_run(run.data(), len, skip, take, s, d);
                if (bad) { printf("len %u skip %u take %u src %d dst %d: %ld\n", len, skip, take, s, d, bad - 1); return 1; }
            }
    }
    printf("ok %ld\n", cases);
    return 0;
}
"""


def windows_of(length):
    """(skip, take) pairs for a run of `length` bytes: starts and ends at every offset mod 4, skip == length, skip > length, take 0,
    windows that end behind the run (by a little, and by all a uint32 holds)"""
    skips = sorted({s for s in (0, 1, 2, 3, 5, length // 2, length - 3, length - 1, length, length + 1, length + 7) if s >= 0})
    out = []
    for s in skips:
        for t in (0, 1, 2, 3, 4, 5, 7, 8, max(length - s, 0), max(length - s - 1, 0), length + 5, 0xFFFFFFFF):
            out.append((s, t))
    return sorted(set(out))


LENGTHS = list(range(0, 41)) + [63, 64, 65, 127, 255, 256, 257, 258, 259, 260, 300, 4097, 70001]


def window_cases():
    return [(n, s, t) for n in LENGTHS for s, t in windows_of(n)]


def test_windowed_copy_lane_by_lane_under_sanitizers(tmp_path):
    main = tmp_path / "main.cc"
    main.write_text(MAIN)
    exe = str(tmp_path / "pack_window")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-o", exe, str(main), os.path.join(ROOT, "tests", "emu", "pack_window_emu.cc")]
    if subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-o", str(tmp_path / "probe"), "-"], input="int main() { return 0; }\n",
                      capture_output=True, text=True).returncode != 0:
        cmd = [c for c in cmd if not c.startswith("-fsanitize") and not c.startswith("-fno-sanitize")]   # no sanitizer runtime: the byte checks alone
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    cases = window_cases()
    assert any(s == n for n, s, t in cases) and any(s > n for n, s, t in cases) and any(t == 0 for n, s, t in cases) and any(s < n < s + t for n, s, t in cases)
    for a in range(4):   # windows that start and end at every offset mod 4
        assert any(s % 4 == a and 0 < t and s + t <= n for n, s, t in cases) and any((s + t) % 4 == a and 0 < t and s + t <= n for n, s, t in cases)
    r = subprocess.run([exe], input="".join("%d %d %d\n" % c for c in cases), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout, r.stderr[-3000:])
    assert int(r.stdout.split()[1]) == len(cases) * 16
