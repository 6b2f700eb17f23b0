"""The split-phase encoder's bool writer kernels on raw bin lists on the MI355X (lep_gpu_debug_write_bins: lep_enc5_write_kernel part by
part, lep_enc5_wchunk_kernel<0..3>, lep_enc5_wchunk_part_kernel<0..2> per part and the stitch) against a plain serial writer in Python
(tests/bool_writer_ref.py, held against lepdev::BoolCoder<false> by tests/test_bool_writer_ref.py).  One launch per form and cut over
all lists, one list per segment -- 11 families x 19 lengths from 1 to 70,000 bins, long and short lanes in one wavefront -- with room
to spare, then the lists of six lengths in reservations of L0 - 1, L0, L0 + 1, L0 + 2 and 1 byte (L0: the stream's length before
the end rule), then with refused segments among the others.  Every launch leaves the arena's bytes outside the reservations alone.

What the lists make the chunked writer do is read from its records and asserted as a lower bound, so that the paths the frames of the
GPU suite never reach did run: on the constant lists other than (0, 128) two range runs never fall into step and the link pass runs
nearly every chunk beyond the warm-up a second time (q_guess != q_start); on the random lists no guess is wrong -- but for
probabilities 1..3 with a bit that is always 1, where the runs stay apart as on a constant list (no claim is made there); many chunks
start before the stream's first byte (t_start < 24) and add their kept bits into the same few bytes.  Stepped on the CPU over
the same lists (tests/test_bool_writer_ref.py prints them; MI355X: the same numbers), per cut in the order of FORMS:
  wrong guesses in the 3 lists over 32,768 bins of const_0_255   K = 2: 1 1 1, 4: 2 2 3, 16: 8 9 12, 64: 32 36 49;
                                                                 (8,1): 3 5 6, (8,4): 21 29 28, (3,4): 6 9 8, (2,32): 41 49 50
  chunks behind the first with t_start < 24                      78, 244, 1275, 5437; 582, 2655, 976, 5396
  chunks with a carry that left their stretch (rec.carry != 0)   0 in every cut: not reached by these lists, perhaps by none"""
import numpy as np
import pytest

import bool_writer_ref as bw

GUARD = 0x5C
GAP = 64
FORMS = [(1, 1, k) for k in bw.STITCHED_K] + [(2, p, c) for p, c in bw.PART_CUTS] + [(0, p, 1) for p in bw.LANE_PARTS]
IDS = ["%s_%d_%d" % ("lane stitched part_chunks".split()[f], p, c) for f, p, c in FORMS]
# chunks behind the first that start before the stream's first byte, per chunked cut: what the CPU twin counts on these lists
EARLY = {(1, 1, 2): 78, (1, 1, 4): 244, (1, 1, 16): 1275, (1, 1, 64): 5437, (2, 8, 1): 582, (2, 8, 4): 2655, (2, 3, 4): 976, (2, 2, 32): 5396}


def reservations(caps):
    """offsets of reservations of `caps` bytes with GAP bytes in front of, between and behind them; the arena's size"""
    off, at = [], GAP
    for c in caps:
        off.append(at)
        at += c + GAP
    return off, at


def outside_is_untouched(arena, offsets, caps):
    own = np.zeros(len(arena), dtype=bool)
    for o, c in zip(offsets, caps):
        own[o:o + c] = True
    return bool((arena[~own] == GUARD).all()) and int((~own).sum()) >= GAP * (len(caps) + 1)


def launch(codec, form, parts, chunks, lists, caps, plan_status=None):
    seed0 = 100 * parts + chunks   # (the part bounds tests/test_bool_writer_ref.py draws)
    pf = [bw.part_bounds(len(b), parts, seed0 + i) for i, b in enumerate(lists)] if form != 1 and parts > 1 else None
    off, size = reservations(caps)
    arena, lens, status, recs = codec.debug_write_bins(form, parts, chunks, lists, off, caps, size, guard=GUARD, plan_status=plan_status, part_first=pf)
    assert outside_is_untouched(arena, off, caps), "bytes outside the reservations changed"
    return [bytes(arena[o:o + c]) for o, c in zip(off, caps)], lens, status, recs


@pytest.mark.gpu
@pytest.mark.parametrize("form,parts,chunks", FORMS, ids=IDS)
def test_gpu_writer_streams_of_bin_lists_equal_the_serial_writer(gpu_codec, form, parts, chunks):
    lists, refs = bw.lists(), bw.references()
    got, lens, status, recs = launch(gpu_codec, form, parts, chunks, [b for _, b in lists], [len(s) + 64 for s, _ in refs])
    wrong, early, carries = {}, 0, 0
    for i, ((family, b), (stream, l0)) in enumerate(zip(lists, refs)):
        assert status[i] == 0 and lens[i] == len(stream), (family, len(b), int(status[i]), int(lens[i]), len(stream))
        assert got[i][:len(stream)] == stream, (family, len(b))
        if form:
            w, e, c = bw.chunk_counts(recs[i])
            wrong.setdefault(family, []).append((len(b), w))
            early += e
            carries += c
    if not form:
        return
    print(IDS[FORMS.index((form, parts, chunks))], bw.say_counts(wrong, early, carries))
    for family in bw.FAMILIES:
        if family == "low_always_1":
            continue
        if family in bw.RANDOM or family == "const_0_128":
            assert all(w == 0 for _, w in wrong[family]), (family, wrong[family])
        else:   # the redo branch of the link pass ran for every long list
            assert all(w >= 1 for n, w in wrong[family] if n > 2 * bw.WARM), (family, wrong[family])
    assert early >= EARLY[(form, parts, chunks)], early   # (16,643 over the eight cuts)


@pytest.mark.gpu
@pytest.mark.parametrize("form,parts,chunks", FORMS, ids=IDS)
def test_gpu_writer_reports_a_reservation_too_small_and_stays_inside_it(gpu_codec, form, parts, chunks):
    """status 100 exactly where L0 >= cap; at L0 + 1 and L0 + 2 the end rule decides the length"""
    lists, refs, cases = bw.lists(), bw.references(), bw.cap_cases()
    got, lens, status, _ = launch(gpu_codec, form, parts, chunks, [lists[i][1] for i, _ in cases], [cap for _, cap in cases])
    overflows = with_zero = 0
    for k, (i, cap) in enumerate(cases):
        stream, l0 = refs[i]
        overflow, want = bw.expect(stream, l0, cap)
        assert (status[k] == 100) == overflow and status[k] in (0, 100), (lists[i][0], len(lists[i][1]), cap, l0, int(status[k]))
        if not overflow:
            assert lens[k] == len(want) and got[k][:len(want)] == want, (lists[i][0], len(lists[i][1]), cap, l0, int(lens[k]))
            with_zero += len(want) == l0 + 1
        overflows += overflow
    assert overflows == 3 * len(cases) // 5 and with_zero >= 4, (overflows, with_zero)


@pytest.mark.gpu
@pytest.mark.parametrize("form,parts,chunks", FORMS, ids=IDS)
def test_gpu_writer_passes_on_a_refused_segment_s_code(gpu_codec, form, parts, chunks):
    """segments the walks refused (plan status 6) among the others: they keep their code and nothing of theirs is written, the others
    are the serial writer's"""
    lists, refs = bw.lists(), bw.references()
    pick = [i for i, (_, b) in enumerate(lists) if len(b) in (5, 129, bw.WARM + 1)]
    refused = set(range(2, len(pick), 5))
    caps = [len(refs[i][0]) + 64 for i in pick]
    got, lens, status, _ = launch(gpu_codec, form, parts, chunks, [lists[i][1] for i in pick], caps, plan_status=[6 if k in refused else 0 for k in range(len(pick))])
    for k, i in enumerate(pick):
        if k in refused:
            assert status[k] == 6 and got[k] == bytes([GUARD]) * caps[k], (k, int(status[k]))
        else:
            assert status[k] == 0 and lens[k] == len(refs[i][0]) and got[k][:lens[k]] == refs[i][0], (k, int(status[k]))


@pytest.mark.gpu
def test_gpu_writer_entry_refuses_what_it_cannot_lay_out_and_a_set_in_a_decode_session(gpu_codec):
    from conftest import golden
    from lepton_amd.codec import LepFile, LeptonError

    lists = [bw.bin_list("uniform", 200, 1), bw.bin_list("uniform", 300, 2)]
    bad = [dict(offsets=[0, 100], caps=[200, 200], arena_bytes=1000),      # reservations that overlap
           dict(offsets=[0, 500], caps=[200, 600], arena_bytes=1000),      # ... that end behind the arena
           dict(offsets=[0, 500], caps=[200, 200], arena_bytes=1000, form=2, parts=3, chunks=4, part_first=[[0, 150, 100], [0, 10, 20]]),   # part bounds not ascending
           dict(offsets=[0, 500], caps=[200, 200], arena_bytes=1000, form=2, parts=2, chunks=4, part_first=[[0, 201], [0, 10]])]            # ... behind the list
    for kw in bad:
        kw = dict(dict(form=1, parts=1, chunks=4), **kw)
        with pytest.raises(LeptonError) as e:
            gpu_codec.debug_write_bins(kw.pop("form"), kw.pop("parts"), kw.pop("chunks"), lists, **kw)
        assert e.value.code == 1 and "out of range" in gpu_codec.last_error()
    session = gpu_codec.decode_rows([LepFile(golden("q30_256x256_4seg")[1])], 1)
    try:
        next(session)
        with pytest.raises(LeptonError) as e:
            gpu_codec.debug_write_bins(1, 1, 4, lists, [0, 500], [200, 400], 1000)
        assert e.value.code == 1 and "decode session" in gpu_codec.last_error()
    finally:
        session.close()
    arena, lens, status, _ = gpu_codec.debug_write_bins(1, 1, 4, lists, [0, 500], [200, 400], 1000, guard=GUARD)
    assert list(status) == [0, 0] and [bytes(arena[o:o + n]) for o, n in zip([0, 500], lens)] == [bw.bool_write(b)[0] for b in lists]
