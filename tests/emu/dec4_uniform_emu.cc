// dec4_uniform_emu.cc -- TEST ONLY: dec_rows_emu.cc (core_emu.cc and the resumable decoder's driver) built with the v4 decoder's
// uniform-test / lane-select switches as the caller's -D flags set them, and an entry point that says which forms this build holds
// (lep_dec4.h LEP_DEC4_UNIFORM_TESTS, LEP_DEC4_LANE_SELECTS), so that a test knows it ran the build it meant to.
#include "dec_rows_emu.cc"

// bit 0: uniform tests, bit 1: lane selects, bit 2: word per lane, bit 3: refill groups, bit 4: the second regrouped pass as asked for,
// bit 5: ... as in force (it needs the lane selects); bits 8..: LEP_DEC4_SCALAR
extern "C" int emu_dec4_uniform_knobs() {
    return LEP_DEC4_UNIFORM_TESTS | (LEP_DEC4_LANE_SELECTS << 1) | (LEP_DEC4_WORD_PER_LANE << 2) | (LEP_DEC4_REFILL_GROUPS << 3) |
           (LEP_DEC4_WORD_PER_LANE_2 << 4) | ((LEP_DEC4_WPL2 ? 1 : 0) << 5) | (LEP_DEC4_SCALAR << 8);
}
