// dec4_update_emu.cc -- TEST ONLY: dec_rows_emu.cc (core_emu.cc and the resumable decoder's driver) plus entry points to the pieces of the
// owners' one-word-per-lane update (lep_dec4.h adapt_words, lep_wave.h wave_gather), so that they can be held against bupd_t and a plain
// index loop on their own, 64 lanes at a time.
#include "dec_rows_emu.cc"

// adapt_words on 64 words: lanes with use[l] adapt words[l] by obs[l], the others keep theirs
extern "C" void emu_dec4_adapt_words(uint32_t* words, const int32_t* use, const int32_t* obs) {
    static lep4::Dec4Shared sh;
    for (uint32_t d = 0; d < 512; ++d) sh.inv24[d] = lep4::inv24_of(d);
    lep4::Dec4Wave w;
    w.sh = &sh;
    w.adapt_words(words, use, obs);
}
extern "C" uint32_t emu_dec4_bupd_t(uint32_t word, uint32_t obs) {
    static uint32_t inv[512];
    if (!inv[2]) for (uint32_t d = 0; d < 512; ++d) inv[d] = lep4::inv24_of(d);
    return lep4::bupd_t(word, obs, inv);
}
extern "C" void emu_wave_gather(const uint32_t* v, const int32_t* src, uint32_t* out) { lepwave::wave_gather(v, src, out); }
// word slot[l] of the group in lane src[l] (groups: 64 x 4 words)
extern "C" void emu_dec4_regroup(const uint32_t* groups, const int32_t* src, const int32_t* slot, uint32_t* out) {
    lep3::U4 G[64];
    for (int l = 0; l < 64; ++l) G[l] = lep3::U4{groups[4 * l], groups[4 * l + 1], groups[4 * l + 2], groups[4 * l + 3]};
    lep4::Dec4Wave::regroup(G, src, slot, out);
}
extern "C" int emu_dec4_knobs() { return LEP_DEC4_WORD_PER_LANE | (LEP_DEC4_REFILL_GROUPS << 1) | (LEP_DEC4_SCALAR << 8); }
