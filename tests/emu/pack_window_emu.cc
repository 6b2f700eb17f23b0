// lep_pack.h's windowed copy (the body of lep_pack_window_copy_kernel behind window_len, which lep_pack_window_offsets_kernel applies)
// stepped lane by lane on the CPU: one run of `len` bytes, of which the window [skip, min(len, skip + take)) is copied.  The source buffer
// ends at the last aligned dword that holds a byte of the WINDOW -- the run's bytes behind it are not there -- and starts at the first
// such dword; the destination likewise, so that a sanitizer build (tests/test_pack_window_emulation.py) sees any load or store outside.
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "../../lepton_amd/csrc/lep_pack.h"

// src_shift / dst_shift (0..3): alignment of the RUN's first byte in the source and of the window's first byte in the destination.
// Returns 0 when dst holds exactly the window between untouched 0xEE bytes and *wlen is its length, otherwise 1 + the offset of the
// first wrong byte (or -1: the clipped length is wrong).
extern "C" long emu_pack_window_run(const uint8_t* run, uint32_t len, uint32_t skip, uint32_t take, int src_shift, int dst_shift) {
    const uint32_t w = leppack::window_len(len, skip, take);
    const uint32_t want = len <= skip ? 0u : ((uint64_t)skip + take < len ? take : len - skip);
    if (w != want) return -1;
    // the window's first byte stands at address (src_shift + skip) mod 4 of an aligned buffer that holds the window's dwords only
    const size_t lead = ((size_t)src_shift + skip) & 3u;
    const size_t sbytes = (lead + w + 3) & ~(size_t)3, dbytes = ((size_t)dst_shift + w + 3) & ~(size_t)3;
    uint8_t* sbuf = static_cast<uint8_t*>(malloc(sbytes ? sbytes : 4));   // (malloc: 16-byte aligned, and exactly this long)
    uint8_t* dbuf = static_cast<uint8_t*>(malloc(dbytes + 16));
    memset(sbuf, 0x55, sbytes ? sbytes : 4);
    memset(dbuf, 0xEE, dbytes + 16);
    uint8_t* win = sbuf + lead;                 // where the window's first byte stands
    uint8_t* d = dbuf + 16 + dst_shift;
    if (w) memcpy(win, run + skip, w);
    // (the kernel's source is src + src_off + skip: the window's first byte, at the alignment the run's start and the skip leave)
    for (uint32_t lane = 0; lane < 64; ++lane) leppack::copy_run(win, d, w, lane);
    long bad = 0;
    for (size_t i = 0; i < dbytes + 16 && !bad; ++i) {
        const bool in = i >= 16 + (size_t)dst_shift && i < 16 + (size_t)dst_shift + w;
        if (dbuf[i] != (in ? run[skip + (i - 16 - dst_shift)] : 0xEE)) bad = 1 + (long)i;
    }
    free(sbuf); free(dbuf);
    return bad;
}
