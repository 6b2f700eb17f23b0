"""The host code of the cut progressive files -- parse_jpeg_prepare_gpu_progressive, parse_jpeg_finish_gpu_progressive (jpeg_scan.cc),
progressive_plan (jpeg_progressive.cc) -- as a program of its own (tests/emu/prog_cut_host_main.cc) built with AddressSanitizer and UBSan
and fed with the records the emulated window decoder leaves for the three sweeps of tests/test_progressive_cut_emulation.py: every cut
file is exactly its bytes on the heap, every row array exactly the records asked for.  The program holds frame, hand-off rows and
truncation bookkeeping against the host parser's and fails on a decline the host parser does not call irregular."""
import os
import subprocess

import pytest

from conftest import ROOT, golden

SWEEPS = {"prog_c420_320x240": ("sos+14", 97), "prog_c444_203x149": (700, 61), "prog_gray_120x88": (400, 23)}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("prog_cut_host")
    exe = str(d / "prog_cut_host")
    csrc = os.path.join(ROOT, "lepton_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", exe,
           os.path.join(ROOT, "tests", "emu", "prog_cut_host_main.cc"), os.path.join(csrc, "jpeg_scan.cc"), os.path.join(csrc, "jpeg_progressive.cc")]
    if subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-o", str(d / "probe"), "-"], input="int main() { return 0; }\n",
                      capture_output=True, text=True).returncode != 0:
        cmd = [c for c in cmd if not c.startswith("-fsanitize") and not c.startswith("-fno-sanitize")]   # no sanitizer runtime: the comparisons alone
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.parametrize("name", sorted(SWEEPS))
def test_host_side_of_the_cut_files_under_sanitizers(program, name):
    jpg = golden(name)[0]
    first, stride = SWEEPS[name]
    if first == "sos+14":
        first = jpg.index(b"\xff\xda") + 14
    r = subprocess.run([program, os.path.join(ROOT, "tests", "golden", name + ".jpg"), str(first), str(stride)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout, r.stderr[-3000:])
    accepted, declined, kept = map(int, r.stdout.split()[1:4])
    # the sweeps hold 191, 106 and 91 cuts the parser accepts, none irregular, none the rules keep with the host
    assert (accepted, declined, kept) == ({"prog_c420_320x240": 191, "prog_c444_203x149": 106, "prog_gray_120x88": 91}[name], 0, 0), r.stdout
