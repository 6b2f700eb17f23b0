"""lep_compress_batch's round-trip check saying "no" on the MI355X.  lep_batch_debug_tamper alters ONE byte of a buffer the pipeline owns,
stream-ordered between the kernel that wrote it and the check that reads it; the batches are golden fixtures cut into three chunks, the
altered file in the second (verify_tamper_cases.py, whose STREAM offsets test_verify_tamper_inputs.py holds against the oracle):
  STREAM   the coded stream, in front of the verification decode    -> exit code 41 with verify, the altered byte in the .lep without
  SCRATCH  the decoded-again frame, in front of the frame comparison -> 41
  VSCAN    a baseline file's scan written again, in front of its check   -> the per-file path redoes the file: status 0, the same .lep
  PSCAN    a progressive file's scan written again, in front of its check -> likewise
Every armed case must report the alteration as applied, every other file of the batch keeps status 0 and its bytes, and an unarmed call
right after gives the unarmed results: the hook disarmed itself and the slots carry nothing over."""
import pytest

import verify_tamper_cases as tc
from conftest import golden
from lepton_amd import abi
from lepton_amd.codec import LepFile

pytestmark = pytest.mark.gpu

UNARMED = {}


@pytest.fixture(params=["0", "1"], ids=["one_stream", "overlap"])
def overlap(request, monkeypatch):
    """LEP_BATCH_OVERLAP=1: the second chunk's kernels run on the second compute stream and workspace set"""
    monkeypatch.setenv("LEP_BATCH_OVERLAP", request.param)
    return request.param


@pytest.fixture
def one_stream(monkeypatch):
    monkeypatch.setenv("LEP_BATCH_OVERLAP", "0")
    return "0"


def run(codec, names, verify):
    return codec.compress_batch([golden(n)[0] for n in names], verify=verify, chunk_images=tc.CHUNK_IMAGES)


def unarmed(codec, names, verify, overlap):
    """the batch compressed with nothing armed, once: the reference-written .lep files, and the statistics an armed call is held against"""
    key = (tuple(names), verify, overlap)
    if key not in UNARMED:
        codec.debug_tamper(0, 0, 0, 0)
        got, status, stats = run(codec, names, verify)
        assert codec.debug_tamper_applied() == 0
        assert status == [0] * len(names) and got == [golden(n)[1] for n in names]
        UNARMED[key] = (got, stats)
    return UNARMED[key]


def armed(codec, names, verify, overlap, where, offset, mask, file=tc.TARGET):
    """-> (results, status, stats, applied, (flag word, decode status)) of the armed call; the other files and the call after it are checked here"""
    want, want_stats = unarmed(codec, names, verify, overlap)
    codec.debug_tamper(where, file, offset, mask)
    got, status, stats = run(codec, names, verify)
    applied, seen = codec.debug_tamper_applied(), codec.debug_tamper_seen()
    print("where %d file %d offset %d mask %#x verify %d overlap %s: status %s applied %d flags %#x decode status %d redone %d" %
          (where, file, offset, mask, verify, overlap, status[file] if file < len(status) else None, applied, seen[0], seen[1], stats["redone_files"]))
    for i in range(len(names)):
        if i != file:
            assert status[i] == 0 and got[i] == want[i], (i, names[i], status[i])
    again, status2, stats2 = run(codec, names, verify)          # nothing armed any more
    assert codec.debug_tamper_applied() == applied
    assert status2 == [0] * len(names) and again == want
    assert stats2["redone_files"] == want_stats["redone_files"] and stats2["gpu_verified_scans"] == want_stats["gpu_verified_scans"]
    return got, status, stats, applied, seen


def route(codec, name):
    """how a fixture travels under verify, alone in a batch: (decoded by the GPU scan decoders, scans checked on the GPU, redone per file)"""
    _, status, stats = codec.compress_batch([golden(name)[0]], verify=True)
    assert status == [0]
    return int(stats["gpu_huffman_files"]), int(stats["gpu_verified_scans"]), int(stats["redone_files"])


@pytest.mark.parametrize("name,offset,mask,oracle_rc", tc.STREAM_CASES)
def test_altered_stream_is_refused(gpu_codec, overlap, name, offset, mask, oracle_rc):
    names = tc.batch_names(name)
    got, status, stats, applied, (flags, decode_status) = armed(gpu_codec, names, True, overlap, abi.TAMPER_STREAM, offset, mask)
    assert applied == 1
    assert status[tc.TARGET] == 41 and got[tc.TARGET] is None
    # which signal: the verification decode's status is the oracle's exit code on that stream; where the oracle decodes to the end,
    # into another frame, the frame comparison alone says no
    assert decode_status == oracle_rc
    assert oracle_rc != 0 or flags & 1
    assert stats["redone_files"] == unarmed(gpu_codec, names, True, overlap)[1]["redone_files"]


@pytest.mark.parametrize("name,offset,mask,oracle_rc", tc.STREAM_CASES)
def test_altered_stream_reaches_the_caller_without_verify(gpu_codec, overlap, name, offset, mask, oracle_rc):
    """the control: the alteration is real, and only `verify` stands between it and the caller"""
    names = tc.batch_names(name)
    got, status, _, applied, _ = armed(gpu_codec, names, False, overlap, abi.TAMPER_STREAM, offset, mask)
    assert applied == 1 and status[tc.TARGET] == 0
    good = golden(name)[1]
    a, b = LepFile(good).streams, LepFile(got[tc.TARGET]).streams
    assert len(a) == len(b) == 1 and len(a[0]) == len(b[0])
    assert [(i, x ^ y) for i, (x, y) in enumerate(zip(a[0], b[0])) if x != y] == [(offset, mask)]
    assert len(got[tc.TARGET]) == len(good) and sum(x != y for x, y in zip(good, got[tc.TARGET])) == 1


@pytest.mark.parametrize("end", ["first_byte", "last_byte"])
@pytest.mark.parametrize("name,gpu_decoded", tc.SCRATCH_CASES)
def test_altered_scratch_frame_is_refused(gpu_codec, overlap, name, gpu_decoded, end):
    """the frame comparison at frame byte 0 and at the frame's last byte, on files the GPU scan decoders took and on one the host parser
    took (gray_120x88 was a host-parsed file once; the one-component scan decoder takes it now, so a cut progressive file stands for those)"""
    assert route(gpu_codec, name)[0] == gpu_decoded
    frame_bytes = LepFile(golden(name)[1]).desc.total_blocks() * 128
    offset = 0 if end == "first_byte" else frame_bytes - 1
    got, status, _, applied, (flags, decode_status) = armed(gpu_codec, tc.batch_names(name), True, overlap, abi.TAMPER_SCRATCH, offset, 0x40)
    assert applied == 1
    assert status[tc.TARGET] == 41 and got[tc.TARGET] is None
    assert flags & 1 and decode_status == 0


@pytest.mark.parametrize("name,where", [("c420_160x120", abi.TAMPER_VSCAN), ("prog_c420_320x240", abi.TAMPER_PSCAN)])
def test_altered_scan_check_sends_the_file_through_the_per_file_path(gpu_codec, one_stream, name, where):
    names = tc.batch_names(name)
    gpu_decoded, checked_scans, redone = route(gpu_codec, name)
    assert gpu_decoded == 1 and checked_scans > 0 and redone == 0
    want, want_stats = unarmed(gpu_codec, names, True, one_stream)
    got, status, stats, applied, (flags, decode_status) = armed(gpu_codec, names, True, one_stream, where, 0, 0x01)
    assert applied == 1
    assert flags & 3 == 2 and decode_status == 0
    assert status[tc.TARGET] == 0 and got[tc.TARGET] == want[tc.TARGET]
    assert stats["gpu_verified_scans"] > 0 and stats["gpu_verified_scans"] == want_stats["gpu_verified_scans"]
    assert want_stats["redone_files"] == 0 and stats["redone_files"] == 1


def test_alterations_that_name_nothing_are_not_applied(gpu_codec, one_stream):
    """an offset outside the buffer, a stage the file has no buffer for, a file that is not in the batch: applied 0, the batch as unarmed"""
    frame = {n: LepFile(golden(n)[1]).desc.total_blocks() * 128 for n in ("c420_160x120", "prog_c420_320x240")}
    cases = [("c420_160x120", True, abi.TAMPER_STREAM, 1 << 40, tc.TARGET),
             ("c420_160x120", False, abi.TAMPER_STREAM, 1 << 32, tc.TARGET),
             ("c420_160x120", True, abi.TAMPER_SCRATCH, frame["c420_160x120"], tc.TARGET),
             ("c420_160x120", False, abi.TAMPER_SCRATCH, 0, tc.TARGET),            # no verify: no scratch frame
             ("c420_160x120", True, abi.TAMPER_VSCAN, 1 << 32, tc.TARGET),
             ("c420_160x120", True, abi.TAMPER_PSCAN, 0, tc.TARGET),               # a baseline file has no progressive check scan
             ("prog_c420_320x240", True, abi.TAMPER_VSCAN, 0, tc.TARGET),          # ... and a progressive one no baseline check segment
             ("prog_c420_320x240", True, abi.TAMPER_PSCAN, 1 << 32, tc.TARGET),
             ("c420_160x120", True, abi.TAMPER_STREAM, 0, 12),                     # one past the batch
             ("c420_160x120", True, 5, 0, tc.TARGET), ("c420_160x120", True, abi.TAMPER_STREAM, 0, -1)]
    for name, verify, where, offset, file in cases:
        names = tc.batch_names(name)
        want, want_stats = unarmed(gpu_codec, names, verify, one_stream)
        got, status, stats, applied, seen = armed(gpu_codec, names, verify, one_stream, where, offset, 0xFF, file=file)
        assert applied == 0 and seen == (0, 0), (name, verify, where, offset, file)
        assert status == [0] * len(names) and got == want
        assert stats["redone_files"] == want_stats["redone_files"]
