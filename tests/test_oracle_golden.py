"""Pins the CPU oracle (oracle/lepton_oracle.c) and the host container code against the REAL reference:
 * tests/golden/*.lep were produced by the reference binary (tests/golden/make_golden.py);
 * images/{iphone16,gold-legacy}.lep are the reference's own known-answer files
   (test_suite/test_16threads.sh, test_legacy.sh) and must decode to the md5s those scripts expect."""
import hashlib
import os

import pytest

import oracle_binding as ob
from conftest import REF_GOLDEN, golden, golden_cases, ref_cases, ref_golden
from lepton_amd.codec import JpegImage, LepFile


def oracle_compress(jpg):
    img = JpegImage(jpg)
    segs = img.plan()
    streams, _ = ob.oracle_encode(img.desc, segs)
    return img.write_lep(streams)


def oracle_decompress(lep):
    f = LepFile(lep)
    ob.oracle_decode(f.desc, f.segments, f.streams)
    return f.recode()


@pytest.mark.parametrize("name", golden_cases())
def test_oracle_encode_equals_reference_lep(name):
    jpg, lep = golden(name)
    assert oracle_compress(jpg) == lep


@pytest.mark.parametrize("name", golden_cases())
def test_oracle_decode_restores_jpeg(name):
    jpg, lep = golden(name)
    assert oracle_decompress(lep) == jpg


@pytest.mark.parametrize("lep,md5", [("iphone16.lep", "8ea9fcf1b2c24877aa838dd6ac1df413"),
                                     ("gold-legacy.lep", "9ffbfc24d1157d0b1ed7a9b53bef4c23")])
def test_reference_known_answer_lep(lep, md5):
    """the reference's known-answer files, kept in tests/golden/ref (known_<name>)"""
    data = open(os.path.join(REF_GOLDEN, "known_" + lep), "rb").read()
    assert hashlib.md5(oracle_decompress(data)).hexdigest() == md5


@pytest.mark.parametrize("name", [n for n in ref_cases() if n not in ("arithmetic", "badzerorun")][:12])
def test_oracle_equals_reference_binary_on_reference_images(name):
    """the reference's own images (the first twelve it compresses): the oracle writes the bytes its binary wrote with -skipverify
    (tests/golden/ref, tests/golden/make_golden_ref.py)"""
    jpg, lep = ref_golden(name)
    assert oracle_compress(jpg) == lep
