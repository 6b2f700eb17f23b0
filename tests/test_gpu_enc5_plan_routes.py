"""Routes of the split-phase encoder's writer plan (lep_enc5_plan.h) that no other GPU test takes: a launch whose chunks per segment are
held down by LEP_ENC5_WLANES, one that LEP_ENC5_WLANES leaves fewer than two chunks per segment (the lane-per-segment writer, without
LEP_ENC5_WCHUNKS=0), and a stitched launch whose gather runs in the parts LEP_ENC5_PARTS names while its records stay one part's.  The
golden q30_256x256_4seg in FOUR thread segments (the file's own plan has two: each is halved on an even block row) with LEP_ENC5_MIN=1:
streams are the oracle's, the kernel is the split-phase encoder's, and lep_gpu_debug_wchunks reports the cut tests/test_enc5_plan.py
works out for 4 segments -- K doubles while 4 * 2K <= LEP_ENC5_WLANES: 32 lanes give 8 chunks (not the 4 the issue's table had), 16 give
4, 7 not even 2."""
import os

import pytest

import oracle_binding as ob
from conftest import golden
from lepton_amd import abi
from lepton_amd.codec import GpuCodec, JpegImage

KNOBS = ("LEP_ENC5_MIN", "LEP_ENC5_WCHUNKS", "LEP_ENC5_WLANES", "LEP_ENC5_WMAXSEG", "LEP_ENC5_WSCHED", "LEP_ENC5_PARTS", "LEP_ENC5_WPARTCHUNKS", "LEP_ENC_WAVES")
ROUTES = {"wlanes_32": ({"LEP_ENC5_WLANES": "32"}, (1, 8)), "wlanes_16": ({"LEP_ENC5_WLANES": "16"}, (1, 4)), "wlanes_7": ({"LEP_ENC5_WLANES": "7"}, (0, 0)),
          "parts_3": ({"LEP_ENC5_PARTS": "3"}, (1, 64))}
CASE = {}


def four_segments():
    """once: (image, plan of four segments, the oracle's streams)"""
    if not CASE:
        img = JpegImage(golden("q30_256x256_4seg")[0])
        plan = []
        for s in img.plan():
            mid = (s.luma_y_start + s.luma_y_end) // 2 & ~1
            assert s.luma_y_start < mid < s.luma_y_end
            plan += [abi.Segment(0, s.luma_y_start, mid, 0), abi.Segment(0, mid, s.luma_y_end, s.is_last)]
        assert len(plan) == 4
        CASE["q30"] = (img, plan, ob.oracle_encode(img.desc, plan)[0])
    return CASE["q30"]


@pytest.mark.gpu
@pytest.mark.parametrize("route", list(ROUTES))
def test_gpu_writer_plan_routes(route, monkeypatch):
    img, plan, want = four_segments()
    settings, cut = ROUTES[route]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("LEP_ENC5_MIN", "1")
    for k, v in settings.items():
        monkeypatch.setenv(k, v)
    codec = GpuCodec(0)        # the knobs are read when the codec object is made
    try:
        got = codec.encode([img], [plan])[0]
        kernel = codec._L.lep_gpu_last_kernel_name(codec.handle)
        parts, chunks, recs = codec.debug_wchunks()
        print(route, kernel, (parts, chunks), None if recs is None else recs.shape)
        assert b"enc5" in kernel, kernel
        assert (parts, chunks) == cut
        assert (recs is None) if cut == (0, 0) else recs.shape == (4, cut[1], 16)
        assert got == want
    finally:
        codec.close()
