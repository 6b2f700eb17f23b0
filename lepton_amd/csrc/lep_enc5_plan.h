// lep_enc5_plan.h -- which encoder an encode launch takes and how the split-phase encoder (lep_enc5.h) schedules its bool writer: the knobs,
// the choice, the writer's plan.  Host code only, no HIP; the launch code (lep_gpu.hip: launch<false>, launch_enc5, launch_enc5_writer)
// allocates and launches what these functions say and decides nothing; tests/test_enc5_plan.py holds them to numbers worked out by hand.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include "../../include/lepton_mi355x.h"

namespace lep5 {
constexpr int kMaxParts = 8;   // parts gather and write may run in (lep_enc5.h: a Ckpt5 per segment and part)

struct Enc5Options {         // the codec object's encoder knobs: enc5_options_from_env reads them when the object is created
    int enc5_min = 8;        // launches of at least this many segments take the split-phase encoder (lep_enc5.h); LEP_ENC5_MIN (0 = never).  64 until
                             // round 4: with the stitched writer a single 4K image (8 segments) takes 109 ms through it against 301 ms through the
                             // two-wavefront single-kernel encoder (profiles/r05k_latency_stitched_writer_ab.json)
    int enc5_waves = 2;      // LEP_ENC5_WAVES: wavefronts per segment in the split-phase walks (1 | 2)
    int enc5_parts = 8;      // LEP_ENC5_PARTS: gather / write in this many parts (1..8), a part written while the next is gathered
                             // (MI355X, 1024 x 4K: 1 part 569 ms per launch, 4 parts 481, 8 parts 475)
    long enc5_wlanes = 131072;  // LEP_ENC5_WLANES: chunk lanes a launch of the stitched writer may have (segments x chunks per segment)
    int enc5_wmaxseg = 4096;    // LEP_ENC5_WMAXSEG: launches of more segments take the writer enc5_wsched names (up to it: stitched behind gather)
    int enc5_wchunks = 64;   // LEP_ENC5_WCHUNKS: the stitched writer for launches that leave lanes free: up to this many chunks per segment (power of
                             // two; 0 = always the lane-per-segment writer beside gather)
    bool enc5_parts_given = false;   // LEP_ENC5_PARTS was set: it holds for every launch (else: one part where the writer runs behind gather)
    int enc5_wsched = 1;     // LEP_ENC5_WSCHED: the writer of launches of more than enc5_wmaxseg segments (LEP_ENC5_WMAXSEG=0: of every launch) --
                             // 0 | lane: lane per segment beside gather; 1 | after: stitched behind the last gather part, chunks as below
                             // that size; 2 | beside: stitched, every part's chunks ranged / linked / coded beside the next part's gather
                             // (MI355X, 1024 x 4K, profiles/r23_*: lane 434 ms per launch; after 423, with gather in one part 403;
                             // beside 420 at 8 parts x 4 chunks, 402 at 2 parts x 8 -- gather loses more to parts and to company than the writer's tail costs)
    int enc5_wpartchunks = 4;   // LEP_ENC5_WPARTCHUNKS: chunks per part and segment of the `beside` schedule (a power of two, 1 .. 32)
    int enc5_gather_wgs = 0; // LEP_ENC5_GATHER_WGS: resident gather workgroups per CU held to this (through the LDS a launch asks for)
    int enc5_fold_apart = 0; // LEP_ENC5_FOLD_APART: the fold launches one after the other, a launch per kind of chain (for the profiler)
    size_t enc5_scratch_max = ~(size_t)0;   // LEP_ENC5_SCRATCH_MAX (bytes): a launch that needs more takes the single-kernel encoder (tests: the out-of-memory path)
    int enc_waves = 0;       // register-budget build of the single-kernel encoder, as the decoder's (LEP_ENC_WAVES = 4 | 8; 2 = the two-wavefronts-per-segment kernel)
    int enc_pair_max = 1280; // launches of up to this many segments take the two-wave encoder: its 128-thread workgroups are resident 6 per
                             // CU (1536 on the chip), one pass; measured (profiles/r02d_latency_sweep.json, 4K images): 1 .. 128 images
                             // 300-343 ms against 450-496 ms for one wavefront per segment, 256 images 650 against 510.  LEP_ENC_PAIR_MAX
};

inline void enc5_options_from_env(Enc5Options* o) {
    if (const char* e = getenv("LEP_ENC_WAVES")) o->enc_waves = atoi(e) == 4 ? 4 : (atoi(e) == 8 ? 8 : (atoi(e) == 2 ? 2 : 0));
    if (const char* e = getenv("LEP_ENC_PAIR_MAX")) o->enc_pair_max = atoi(e);
    if (const char* e = getenv("LEP_ENC5_MIN")) o->enc5_min = atoi(e);
    if (const char* e = getenv("LEP_ENC5_WAVES")) o->enc5_waves = atoi(e) == 1 ? 1 : 2;
    if (const char* e = getenv("LEP_ENC5_FOLD_APART")) o->enc5_fold_apart = atoi(e);
    if (const char* e = getenv("LEP_ENC5_GATHER_WGS")) o->enc5_gather_wgs = atoi(e);
    if (const char* e = getenv("LEP_ENC5_PARTS")) { o->enc5_parts = atoi(e); o->enc5_parts_given = true; }
    if (const char* e = getenv("LEP_ENC5_WCHUNKS")) o->enc5_wchunks = atoi(e);
    if (const char* e = getenv("LEP_ENC5_WLANES")) o->enc5_wlanes = atol(e);
    if (const char* e = getenv("LEP_ENC5_WMAXSEG")) o->enc5_wmaxseg = atoi(e);
    if (const char* e = getenv("LEP_ENC5_WSCHED")) o->enc5_wsched = !strcmp(e, "lane") ? 0 : !strcmp(e, "after") ? 1 : !strcmp(e, "beside") ? 2 : std::min(std::max(atoi(e), 0), 2);
    if (const char* e = getenv("LEP_ENC5_WPARTCHUNKS")) { const int c = atoi(e); o->enc5_wpartchunks = 1; while (o->enc5_wpartchunks * 2 <= std::min(c, 32)) o->enc5_wpartchunks *= 2; }
    if (const char* e = getenv("LEP_ENC5_SCRATCH_MAX")) o->enc5_scratch_max = (size_t)strtoull(e, nullptr, 10);
}

// Which encoder takes a launch.  waves: the single-kernel form, which also stands behind the split-phase encoder when its scratch cannot
// be had -- 2: lep_encode_v3x2_kernel (few segments: two wavefronts per segment, producer / bool coder, half the serial chain), 4 | 8:
// lep_encode_v3_kernel<4 | 8> (like the decoder: a launch that cannot fill 8 wavefronts per SIMD takes the 4-wave build, 128 VGPRs, no spills)
struct EncChoice { bool split_phase; int waves; };
inline EncChoice enc_choice(int nseg, const Enc5Options& o) {
    const int waves = o.enc_waves ? o.enc_waves : nseg > 4608 ? 8 : (nseg <= o.enc_pair_max ? 2 : 4);
    return {o.enc5_min > 0 && !o.enc_waves && nseg >= o.enc5_min, waves};   // (LEP_ENC_WAVES asks for one of the single-kernel forms)
}

struct Enc5WriterPlan {      // everything launch_enc5_writer needs of one of the writer's three forms
    int form, gather_parts;   // LEP_DEBUG_WRITE_LANE | _STITCHED | _PART_CHUNKS; gather's parts: the lane and part-chunk writers follow it part by part
    int chunks;               // per segment (stitched) or per part and segment (part chunks); 0: the lane writer
    int records;              // WChunk5 per segment: what the chunked forms need of W_ENC5_WCHUNKS, and the stitch kernel's K
    int groups, lane_groups;  // grids: a lane per segment, a lane per chunk (of the launch / of a part)
    int report_parts;         // with chunks, what lep_gpu_debug_wchunks says of the launch: (1, K) behind gather whatever gather's parts, (0, 0) for the lane writer
    const char* name;         // lep_gpu_last_kernel_name
};
inline Enc5WriterPlan enc5_writer_form(int form, int nseg, int parts, int chunks) {
    const bool lane = form == LEP_DEBUG_WRITE_LANE, cut = form == LEP_DEBUG_WRITE_PART_CHUNKS;
    Enc5WriterPlan W;
    W.form = form; W.gather_parts = parts; W.chunks = lane ? 0 : chunks; W.records = cut ? parts * chunks : W.chunks;
    W.groups = (nseg + 63) / 64; W.lane_groups = (int)(((long)nseg * W.chunks + 63) / 64); W.report_parts = lane ? 0 : (cut ? parts : 1);
    W.name = cut ? "lep_enc5 (count | emit | fold | gather | write: part chunks beside gather)" : "lep_enc5 (count | emit | fold | gather | write)";
    return W;
}
// The lane-per-segment writer: gather and write in parts (tile ranges of every segment) -- the writer is 128 wavefronts that take the
// same time whatever the batch, part k is written (second stream) while part k + 1 is gathered.  What a launch degrades to when there
// is no room for a chunked plan's records: in enc5_parts parts, not in the one part a stitched plan had.
inline Enc5WriterPlan enc5_lane_plan(int nseg, const Enc5Options& o) {
    return enc5_writer_form(LEP_DEBUG_WRITE_LANE, nseg, std::min(std::max(o.enc5_parts, 1), kMaxParts), 0);
}
// The writer's schedule.  A launch that leaves the chip's lanes free takes the stitched writer behind gather: K chunks per segment (a
// power of two up to 64), as many as keep the launch under enc5_wlanes chunk lanes.  Round 4 capped the lanes at 4096 (K = 2 at 256
// images: two chains of 1.15 M bins per segment, 118 ms of writer on 64 wavefronts); round 6 measured the cap away (profiles/r6o_*:
// 256 images 253 -> 148 ms per launch with K = 32, 128 images 159 -> 107, 512 images -- which had kept the lane-per-segment writer
// -- 308 -> 260).  From 4097 segments on enc5_wsched says which (profiles/r23_*).
inline Enc5WriterPlan enc5_writer_plan(int nseg, const Enc5Options& o) {
    const Enc5WriterPlan lane = enc5_lane_plan(nseg, o);
    const int wsched = nseg <= o.enc5_wmaxseg ? 1 : o.enc5_wsched;
    int K = 0;
    if (o.enc5_wchunks >= 2 && wsched == 1) { K = 1; while (K * 2 <= o.enc5_wchunks && (long)nseg * K * 2 <= o.enc5_wlanes) K *= 2; }
    // Parts exist for a writer that runs beside gather.  Behind gather there is nothing to hide, and gather in parts is the slower one
    // (1024 x 4K, nothing beside it: 8 parts 133 ms, one part 115 -- every part steps through the segment's tiles to its first and ends on
    // its slowest segment; 512 images 231 against 220 ms per launch, 256 images 142 against 137): a launch that writes behind gather
    // gathers in ONE part unless LEP_ENC5_PARTS names a number.
    if (K >= 2) return enc5_writer_form(LEP_DEBUG_WRITE_STITCHED, nseg, o.enc5_parts_given ? lane.gather_parts : 1, K);
    // `beside`: c chunks per part, cut at the parts' boundaries -- part p's range / link / code go out on the second stream when part p
    // is gathered and run beside the gather of part p + 1; behind the last part only that part's phases and the stitch are left
    if (wsched == 2 && o.enc5_wpartchunks >= 1) return enc5_writer_form(LEP_DEBUG_WRITE_PART_CHUNKS, nseg, lane.gather_parts, o.enc5_wpartchunks);
    return lane;
}

}  // namespace lep5
