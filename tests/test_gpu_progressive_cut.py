"""Progressive files that END INSIDE A SCAN through the batch pipelines of the HIP build, with lep_gpu_cut_progressive on (a codec starts
with it off: they take the host parser on compress and the host re-coder on decompress, as they always have).  The window decoder
(lep_huffprogdec_win.h, LEP_HUFFDEC_EARLY_EOF on the file's last scan) decodes them up to the block that reads the data's last bit, and the
scan writers write every scan whole from the frame, the byte bound cutting the output.

Inputs: the five prog_truncated_* fixtures, every 8th cut of the three sweeps of tests/test_progressive_cut_emulation.py, and four whole
progressive fixtures in the same batch, so that whole and cut files share a launch.  The .lep must be the per-file path's (host parser),
which for the four regular fixtures is the committed, reference-written file; statuses too; both directions must say that the scan kernels
did the Huffman half for every file but the ones whose final block had failed to decode (lep_jpeg_cut_block_irregular), which the kernels
leave to the host parser."""
import os
import sys

import pytest

from conftest import golden
from lepton_amd import abi
from lepton_amd.codec import GpuCodec, LeptonError

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

WHOLE = ["prog_c420_320x240", "prog_c444_203x149", "prog_gray_120x88", "prog_c420_q97_800x600"]


def _inputs():
    import test_progressive_cut_emulation as cuts

    names, jpgs, known = [], [], {}
    for n in cuts.REGULAR + [cuts.IRREGULAR]:
        j, l = golden(n)
        if n in cuts.REGULAR:
            known[len(jpgs)] = l
        names.append(n); jpgs.append(j)
    for n in sorted(cuts.SWEEPS):
        jpg, ps = cuts.sweep_cuts(n)
        for p in ps[::8]:
            names.append("%s[:%d]" % (n, p)); jpgs.append(jpg[:p])
    for n in WHOLE:
        j, l = golden(n)
        known[len(jpgs)] = l
        names.append(n); jpgs.append(j)
    return names, jpgs, known


def test_gpu_cut_progressive_files_take_the_scan_kernels_both_ways():
    import test_progressive_cut_emulation as cuts

    names, jpgs, known = _inputs()
    L = abi.lib()
    codec = GpuCodec(0)
    try:
        # a codec starts with the cut files on the host, as every caller has known them: nothing of the scan kernels for the five fixtures
        five = jpgs[:5]
        _, st0, cs0 = codec.compress_batch(five)
        assert st0 == [0] * 5 and cs0["gpu_huffman_files"] == 0, (st0, cs0)
        assert codec.cut_progressive(True) == 1
        want, want_st, irregular = [], [], 0
        for n, j in zip(names, jpgs):
            try:
                want.append(codec.compress(j)); want_st.append(0)          # per file: host parser + coder kernels
            except LeptonError as e:
                want.append(b""); want_st.append(e.code)                   # a cut the parser refuses keeps lep_compress's code
            rc, irr, _ = cuts.host_parse(j)
            assert (rc != 0) == (want_st[-1] != 0), (n, rc, want_st[-1])
            irregular += 1 if (rc == 0 and irr) else 0
        for i, l in known.items():
            assert want[i] == l, names[i]                                  # ... which for the fixtures is the reference's file
        parsed = sum(1 for s in want_st if s == 0)
        assert irregular == 1 and parsed >= len(jpgs) - 8, (irregular, parsed, len(jpgs))   # prog_truncated_refine_overrun alone; few cuts are refused
        on_gpu = parsed - irregular
        for verify in (False, True):
            chances, timeouts = L.lep_batch_scan_second_chances(), L.lep_jpeg_gpu_scan_wait_timeouts()
            got, st, cs = codec.compress_batch(jpgs, chunk_images=16, verify=verify)
            assert st == want_st, (verify, [(names[i], st[i], want_st[i]) for i in range(len(jpgs)) if st[i] != want_st[i]])
            bad = [names[i] for i in range(len(jpgs)) if want_st[i] == 0 and got[i] != want[i]]
            assert not bad, (verify, bad)
            assert cs["gpu_huffman_files"] == on_gpu, (verify, cs, on_gpu)
            assert cs["redone_files"] == 0, (verify, cs)
            assert (L.lep_batch_scan_second_chances(), L.lep_jpeg_gpu_scan_wait_timeouts()) == (chances, timeouts)
        leps = [w for w, s in zip(want, want_st) if s == 0]
        orig = [j for j, s in zip(jpgs, want_st) if s == 0]
        back, st2, ds = codec.decompress_batch(leps, chunk_images=16)
        assert st2 == [0] * len(leps), st2
        bad = [i for i in range(len(leps)) if back[i] != orig[i]]
        assert not bad, bad
        # every file, the irregular one included: what its final block left in the frame is coefficients like any others to the scan writers
        # (nothing in a .lep says how the block that met the end had decoded) -- never fewer than the compressor's count
        assert ds["gpu_huffman_files"] == len(leps) >= on_gpu, (ds, len(leps), on_gpu)
    finally:
        codec.close()
