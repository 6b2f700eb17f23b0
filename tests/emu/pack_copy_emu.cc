// lep_pack.h's copy routine (the body of lep_pack_copy_kernel) stepped lane by lane on the CPU: one run, 64 lanes one after the other.
// The source stands at the very end of a buffer whose size is a multiple of four and the destination likewise, so that a sanitizer build
// (tests/test_pack_emulation.py) sees any load or store outside the aligned dwords that hold bytes of the run.
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "../../lepton_amd/csrc/lep_pack.h"

// src_shift / dst_shift (0..3): alignment of the run's first byte in source and destination.  Returns 0 when dst holds exactly the run
// between untouched 0xEE bytes, otherwise 1 + the offset of the first wrong byte.
extern "C" long emu_pack_copy_run(const uint8_t* run, uint32_t len, int src_shift, int dst_shift) {
    const size_t sbytes = ((size_t)src_shift + len + 3) & ~(size_t)3, dbytes = ((size_t)dst_shift + len + 3) & ~(size_t)3;
    uint8_t* sbuf = static_cast<uint8_t*>(malloc(sbytes + 16));   // (malloc: 16-byte aligned, and exactly this long)
    uint8_t* dbuf = static_cast<uint8_t*>(malloc(dbytes + 16));
    memset(sbuf, 0x55, sbytes + 16);
    memset(dbuf, 0xEE, dbytes + 16);
    uint8_t* s = sbuf + 16 + src_shift;
    uint8_t* d = dbuf + 16 + dst_shift;
    if (len) memcpy(s, run, len);
    for (uint32_t lane = 0; lane < 64; ++lane) leppack::copy_run(s, d, len, lane);
    long bad = 0;
    for (size_t i = 0; i < dbytes + 16 && !bad; ++i) {
        const bool in = i >= 16 + (size_t)dst_shift && i < 16 + (size_t)dst_shift + len;
        if (dbuf[i] != (in ? run[i - 16 - dst_shift] : 0xEE)) bad = 1 + (long)i;
    }
    free(sbuf); free(dbuf);
    return bad;
}
