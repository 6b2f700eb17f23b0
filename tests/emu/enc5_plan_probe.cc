// enc5_plan_probe.cc -- TEST ONLY: lep_enc5_plan.h (the encoder's knobs, enc_choice, the split-phase writer's plan) behind a C entry for
// tests/test_enc5_plan.py, which builds it as a library.  The knobs come from "NAME=value" strings that stand in THIS process's
// environment while enc5_options_from_env reads it, as lep_gpu_create has it read; every LEP_ENC* variable the process had is taken
// out for that long and put back.  Never linked into the product.
#include <cstdint>
#include <string>
#include <utility>
#include <vector>
#include "../../lepton_amd/csrc/lep_enc5_plan.h"

extern char** environ;

static std::vector<std::pair<std::string, std::string>> take_knobs() {   // every LEP_ENC* variable, out of the environment
    std::vector<std::pair<std::string, std::string>> had;
    for (char** e = environ; *e; ++e) {
        const char* eq = strchr(*e, '=');
        if (eq && !strncmp(*e, "LEP_ENC", 7)) had.emplace_back(std::string(*e, (size_t)(eq - *e)), std::string(eq + 1));
    }
    for (const auto& kv : had) unsetenv(kv.first.c_str());
    return had;
}
static lep5::Enc5Options options_of(const char* const* settings, int nset) {
    const auto had = take_knobs();
    for (int i = 0; i < nset; ++i) {
        const std::string s(settings[i]);
        setenv(s.substr(0, s.find('=')).c_str(), s.substr(s.find('=') + 1).c_str(), 1);
    }
    lep5::Enc5Options o;
    lep5::enc5_options_from_env(&o);
    take_knobs();
    for (const auto& kv : had) setenv(kv.first.c_str(), kv.second.c_str(), 1);
    return o;
}

// out[11] = {split_phase, waves, form, gather_parts, chunks, records, groups, lane_groups, report_parts, report_chunks, name says
// "beside gather"}; degraded: the plan the launch takes when the records cannot be had
extern "C" void emu_enc5_plan(const char* const* settings, int nset, int nseg, int degraded, int32_t* out) {
    const lep5::Enc5Options o = options_of(settings, nset);
    const lep5::EncChoice c = lep5::enc_choice(nseg, o);
    const lep5::Enc5WriterPlan W = degraded ? lep5::enc5_lane_plan(nseg, o) : lep5::enc5_writer_plan(nseg, o);
    const int32_t v[11] = {c.split_phase, c.waves, W.form, W.gather_parts, W.chunks, W.records, W.groups, W.lane_groups, W.report_parts, W.chunks,
                           strstr(W.name, "beside gather") != nullptr};
    memcpy(out, v, sizeof v);
}
// the knobs as parsed: out[8] = {enc5_wsched, enc5_wpartchunks, enc5_waves, enc_waves, enc_pair_max, enc5_parts, enc5_parts_given, enc5_scratch_max}
extern "C" void emu_enc5_knobs(const char* const* settings, int nset, uint64_t* out) {
    const lep5::Enc5Options o = options_of(settings, nset);
    const uint64_t v[8] = {(uint64_t)o.enc5_wsched, (uint64_t)o.enc5_wpartchunks, (uint64_t)o.enc5_waves, (uint64_t)o.enc_waves, (uint64_t)(int64_t)o.enc_pair_max,
                           (uint64_t)(int64_t)o.enc5_parts, (uint64_t)o.enc5_parts_given, (uint64_t)o.enc5_scratch_max};
    memcpy(out, v, sizeof v);
}
