"""The reference of the writer-list tests (tests/bool_writer_ref.py, a plain serial bool writer in Python) held against
lepdev::BoolCoder<false> (tests/emu/lep_core_coder.h) on every list and every reservation tests/test_gpu_enc5_writer_lists.py uses, and
the writer of lep_enc5.h stepped on the CPU over the same lists in the forms and cuts the GPU test launches (core_emu.cc
emu_write_bins5): its bytes are the reference's, and its records show what those lists make the writer do -- on the constant lists the
link pass runs nearly every chunk's range a second time, on the random ones never; the GPU test asserts the same of the kernels."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bool_writer_ref as bw
from conftest import ROOT


@pytest.fixture(scope="module")
def emu():
    so = os.path.join(ROOT, "tests", "emu", "libcore_emu_boolref.so")
    tmp = "%s.%d" % (so, os.getpid())
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", tmp, os.path.join(ROOT, "tests", "emu", "core_emu.cc")])
    os.replace(tmp, so)
    return C.CDLL(so)


def serial(emu, bins, cap):
    """BoolCoder<false>: (overflow, bytes)"""
    out = (C.c_uint8 * (cap + 8))()
    n, ov = C.c_uint32(), C.c_int()
    a = np.ascontiguousarray(bins, dtype=np.uint16)
    assert emu.emu_bool_writer_list(a.ctypes.data_as(C.c_void_p), len(a), out, cap, C.byref(n), C.byref(ov)) == 0
    return bool(ov.value), bytes(out[:n.value])


def test_python_writer_equals_the_serial_coder_at_every_reservation(emu):
    """every list with room to spare, the lists of CAP_LENGTHS at L0 - 1, L0, L0 + 1, L0 + 2 and 1 byte: the verdict is L0 >= cap, and
    where the serial coder does not overflow its bytes are the Python writer's -- with and without the end rule's zero byte"""
    lists, refs = bw.lists(), bw.references()
    assert len(lists) == len(bw.FAMILIES) * len(bw.LENGTHS) and sum(len(b) for _, b in lists) < 3_000_000
    cases = [(i, bw.ROOMY) for i in range(len(lists))] + bw.cap_cases()
    assert len(cases) == len(lists) + 5 * len(bw.FAMILIES) * len(bw.CAP_LENGTHS)
    overflows = end_rule = 0
    for i, cap in cases:
        stream, l0 = refs[i]
        assert l0 < bw.ROOMY
        ov, got = serial(emu, lists[i][1], cap)
        want_ov, want = bw.expect(stream, l0, cap)
        assert ov == want_ov, (lists[i][0], len(lists[i][1]), cap, l0)
        if not ov:
            assert got == want, (lists[i][0], len(lists[i][1]), cap)
            end_rule += cap != bw.ROOMY and len(stream) == l0 + 1
        overflows += ov
    # (L0 - 1, L0 and 1 overflow -- a stream is never shorter than two bytes; L0 + 1 takes a stream without the zero byte, L0 + 2 one with)
    assert overflows == 3 * len(bw.FAMILIES) * len(bw.CAP_LENGTHS)
    assert end_rule >= 4, end_rule


def run_cut(emu, form, parts, chunks, lists, caps, seed0=0, plan_status=None):
    """emu_write_bins5 over the lists: [(status, length, bytes, records)]"""
    out = []
    K = chunks if form == 1 else parts * chunks
    for i, ((_, b), cap) in enumerate(zip(lists, caps)):
        a = np.ascontiguousarray(b, dtype=np.uint16)
        buf = (C.c_uint8 * (cap + 8))()
        n, st = C.c_uint32(), C.c_int32()
        recs = np.zeros((K, bw.REC_WORDS), dtype=np.uint32)
        pf = (C.c_uint32 * bw.MAX_PARTS)(*bw.part_bounds(len(a), parts, seed0 + i))
        assert emu.emu_write_bins5(form, parts, chunks, a.ctypes.data_as(C.c_void_p), len(a), pf, plan_status[i] if plan_status else 0, buf, cap,
                                   C.byref(n), C.byref(st), recs.ctypes.data_as(C.c_void_p)) == 0
        out.append((st.value, n.value, bytes(buf[:min(n.value, cap)]), recs))
    return out


FORMS = [(1, 1, k) for k in bw.STITCHED_K] + [(2, p, c) for p, c in bw.PART_CUTS] + [(0, p, 1) for p in bw.LANE_PARTS]


@pytest.mark.parametrize("form,parts,chunks", FORMS, ids=["%s_%d_%d" % ("lane stitched part_chunks".split()[f], p, c) for f, p, c in FORMS])
def test_writer_on_the_cpu_equals_the_reference_and_redoes_the_constant_lists(emu, form, parts, chunks):
    lists, refs = bw.lists(), bw.references()
    got = run_cut(emu, form, parts, chunks, lists, [bw.ROOMY] * len(lists), seed0=100 * parts + chunks)
    wrong, early, carries = {}, 0, 0
    for (family, b), (stream, l0), (st, n, data, recs) in zip(lists, refs, got):
        assert st == 0 and n == len(stream) and data == stream, (family, len(b))
        if form:
            w, e, c = bw.chunk_counts(recs)
            wrong.setdefault(family, []).append((len(b), w))
            early += e
            carries += c
    if form:
        print(bw.say_counts(wrong, early, carries))
        for family in bw.FAMILIES:
            if family == "low_always_1":   # (random probabilities, but a bit that never changes: two range runs stay apart as on a constant list)
                continue
            if family in bw.RANDOM or family == "const_0_128":
                assert all(w == 0 for _, w in wrong[family]), (family, wrong[family])
            else:
                assert all(w >= 1 for n, w in wrong[family] if n > 2 * bw.WARM), (family, wrong[family])
