// lep_gpu.hip -- layer 1 of the C ABI: HIP kernels for gfx950 and the runtime object that launches them.
// One wavefront per (image, thread segment) work item; per-segment adaptive model resident in HBM
// (2.9 MB each, hot tables first), coefficient frames read/written in place in the reference's
// AlignedBlock layout, streams written to / read from one device arena.  No CPU fallback: every entry
// point returns LEP_GPU_ERROR if HIP reports a failure.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/lepton_mi355x.h"
#include "lep_buffers.h"

#define LEP_DEV __device__ __forceinline__
#include "lep_core.h"
#include "lep_enc3.h"
#include "lep_dec4.h"
#include "lep_enc5.h"
#include "lep_enc5_plan.h"
#include "lep_huff.h"
#include "lep_huffdec.h"
#include "lep_huffdec_simt.h"
#include "lep_huff_simt.h"
#include "lep_huffprog.h"
#include "lep_huffprog_simt.h"
#include "lep_huffprogdec.h"
#include "lep_huffprogdec_win.h"
#include "lep_huffprogdec_rst.h"
#include "lep_scan_decode_plan.h"
#include "lep_pack.h"
#include "lep_rgb.h"
#include "lep_samples.h"

using namespace lepdev;

namespace {

// the encoder uses the dense model layout (kModelBranches words), the decoder the group-aligned one (lep3::kModelWords);
// segments are spaced by the larger so that one arena serves both
constexpr size_t kModelStride = lep3::kModelWords > kModelBranches ? lep3::kModelWords : kModelBranches;

template <uint32_t WORDS = kModelBranches>
__device__ void reset_segment_state(uint32_t* model, NSum* ns, int ns_count, int lane) {
    // model reset = Branch::identity() everywhere (model.hh:114-125); 16-byte coalesced stores
    uint4* m4 = reinterpret_cast<uint4*>(model);
    const uint4 init = make_uint4(kBranchInit, kBranchInit, kBranchInit, kBranchInit);
    for (uint32_t i = lane; i < WORDS / 4; i += 64) m4[i] = init;
    uint32_t* n32 = reinterpret_cast<uint32_t*>(ns);
    const uint32_t words = (uint32_t)ns_count * (sizeof(NSum) / 4);
    for (uint32_t i = lane; i < words; i += 64) n32[i] = 0;
}

// The encoder (lep_enc3.h): lane-parallel context / bin-list phases, one model round trip per block, bool coder as uniform
// vector code; 64 VGPRs -> 8 wavefronts per SIMD.  (Earlier generations -- single-lane, exec-masked lane 0, scalar-unit
// serial part -- live on as CPU cross-checks under tests/emu/retired/.)
template <int WAVES>
__global__ __launch_bounds__(64, WAVES) void lep_encode_v3_kernel(const ImageDev* __restrict__ images, const SegDev* __restrict__ segs,
                                                              uint32_t* models, NSum* ns_area, const uint64_t* ns_offsets,
                                                              uint8_t* streams, uint32_t* stream_len, int32_t* status, uint32_t* bins) {
    __shared__ lep3::Enc3Shared sh;
    const int s = blockIdx.x, lane = threadIdx.x;
    const SegDev seg = segs[s];
    const ImageDev* img = images + seg.image;
    uint32_t* model = models + (size_t)s * kModelStride;
    NSum* ns = ns_area + ns_offsets[s];
    reset_segment_state(model, ns, img->ns_total, lane);
    __syncthreads();
    lep3::Enc3Wave w;
    int rc = w.run(img, seg, model, ns, &sh, streams + seg.stream_off, seg.stream_cap);
    uint32_t n = rc ? 0 : w.bc.finish();
    if (lane != 0) return;
    if (!rc && w.bc.overflow) rc = LEP_BUFFER_TOO_SMALL;
    stream_len[seg.slot] = n;
    status[seg.slot] = rc;
    bins[seg.slot] = w.nbins;
}

// Two wavefronts per thread segment (lep_enc3.h, Enc3Pipe): wavefront 0 produces resolved bin-list chunks, wavefront 1
// runs the bool coder one chunk behind.  For launches that cannot fill the chip with one wavefront per segment (a single
// image is 8 segments): the segment's serial chain is about half as long.
__global__ __launch_bounds__(128, 2) void lep_encode_v3x2_kernel(const ImageDev* __restrict__ images, const SegDev* __restrict__ segs,
                                                                 uint32_t* models, NSum* ns_area, const uint64_t* ns_offsets,
                                                                 uint8_t* streams, uint32_t* stream_len, int32_t* status, uint32_t* bins) {
    __shared__ lep3::Enc3Shared sh;
    __shared__ lep3::Enc3Pipe pipe;
    const int s = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const SegDev seg = segs[s];
    const ImageDev* img = images + seg.image;
    uint32_t* model = models + (size_t)s * kModelStride;
    NSum* ns = ns_area + ns_offsets[s];
    if (wave == 0) reset_segment_state(model, ns, img->ns_total, lane);
    if (threadIdx.x == 0) { pipe.count[0] = 0; pipe.count[1] = 0; }
    __syncthreads();
    lep3::Enc3Wave w;
    if (wave == 0) {
        int rc = w.run(img, seg, model, ns, &sh, streams + seg.stream_off, seg.stream_cap, &pipe);
        if (lane != 0) return;
        if (!rc && pipe.out_overflow) rc = LEP_BUFFER_TOO_SMALL;
        stream_len[seg.slot] = rc ? 0 : pipe.out_len;
        status[seg.slot] = rc;
        bins[seg.slot] = w.nbins;
    } else {
        w.consume(&sh, &pipe, streams + seg.stream_off, seg.stream_cap);
    }
}

#ifdef LEP_PROF
__device__ unsigned long long g_prof4[8192][32];   // private accumulators per wave (no atomic contention)
#endif

// exhaustive check of the float-reciprocal / table-reciprocal Branch probabilities against integer division (all 255 x 255 count pairs)
__global__ void lep_selftest_kernel(uint32_t* mismatches) {
    __shared__ uint32_t inv24[512];
    for (uint32_t d = threadIdx.x; d < 512; d += blockDim.x) inv24[d] = lep4::inv24_of(d);
    __syncthreads();
    const uint32_t f = blockIdx.x + 1, t = threadIdx.x + 1;
    if (t > 255) return;
    for (uint32_t obs = 0; obs < 2; ++obs) {   // v4 decoder's table-reciprocal update (lep_dec4.h)
        const uint32_t w = f | (t << 8) | (((f << 8) / (f + t)) << 16);
        if (lep4::bupd_t(w, obs, inv24) != branch_update(w, (int)obs)) atomicAdd(mismatches, 1u);
    }
    if (lep3::prob_of(f, t) != (f << 8) / (f + t)) atomicAdd(mismatches, 1u);
    if (lep5::prob16(f | (t << 8)) != (f << 8) / (f + t)) atomicAdd(mismatches, 1u);   // the fold kernels' form (lep_enc5.h)
    for (int obs = 0; obs < 2; ++obs) {
        const uint32_t w = f | (t << 8) | (((f << 8) / (f + t)) << 16);
        if (lep3::bupd(w, obs) != branch_update(w, obs)) atomicAdd(mismatches, 1u);
    }
    {   // lep4::div_by against the hardware's expansion of `/`: 65025 divisors (quantiser x ICOS column), numerators at their multiples
        const int32_t d = (int32_t)((f * 257u + t) * (f & 1 ? 8192u : (t & 1 ? 2260u : 1u)));
        if (d >= 2) {
            const lep4::DivBy m = lep4::DivBy::of((uint32_t)d);
            const int32_t k = (int32_t)(0x7fffffff / d);
            for (int32_t n : {0, 1, -1, d, d - 1, -d, -d + 1, k * d, k * d - 1, -(k * d), 0x7fffffff, (int32_t)0x80000000, (int32_t)(f * 0x01000193u ^ t * 0x9e3779b9u)})
                if (lep4::div_by(n, m.mul, m.shift) != n / d) atomicAdd(mismatches, 1u);
        }
    }
}

// v4 decoder: serial part as uniform vector code, multi-bin interior windows, one merged edge round (lep_dec4.h).
// WAVES = waves per SIMD the register allocation is held to.
template <int WAVES, int SCMASK = LEP_DEC4_SCALAR>
__global__ __launch_bounds__(64, WAVES) void lep_decode_v4_kernel(const ImageDev* __restrict__ images, const SegDev* __restrict__ segs,
                                                           uint32_t* models, NSum* ns_area, const uint64_t* ns_offsets,
                                                           uint8_t* streams, uint32_t* stream_len, int32_t* status, uint32_t* bins) {
    __shared__ lep4::Dec4Shared sh;
    const int s = blockIdx.x, lane = threadIdx.x;
    const SegDev seg = segs[s];
    const ImageDev* img = images + seg.image;
    uint32_t* model = models + (size_t)s * kModelStride;
    NSum* ns = ns_area + ns_offsets[s];
    reset_segment_state<lep3::kModelWords>(model, ns, img->ns_total, lane);
    __syncthreads();
    lep4::Dec4WaveT<SCMASK> w;
#ifdef LEP_PROF
    w.prof_begin(&g_prof4[s & 8191][0]);
#endif
    int rc = w.run(img, seg, model, ns, &sh, streams + seg.stream_off, stream_len[seg.slot]);
#ifdef LEP_PROF
    w.prof_end();
#endif
    if (lane != 0) return;
    status[seg.slot] = rc;
    bins[seg.slot] = w.nbins;
}

// The same decoder one band of MCU rows per launch (Dec4WaveT::run_rows; lep_gpu_decode_rows_*): a segment takes up where its record
// (recs[slot], lds_save[slot]) says the launch before left it; models and rings are reset on a segment's first band only, and a
// segment that is finished or has failed returns at once.
constexpr int kRowsLdsWords = lep3::kSignWords + lep3::kResDcWords;
template <int WAVES, int SCMASK = LEP_DEC4_SCALAR>
__global__ __launch_bounds__(64, WAVES) void lep_decode_v4_rows_kernel(const ImageDev* __restrict__ images, const SegDev* __restrict__ segs,
                                                                uint32_t* models, NSum* ns_area, const uint64_t* ns_offsets,
                                                                const uint8_t* streams, const uint32_t* stream_len, lep4::Dec4Resume* recs,
                                                                uint32_t* lds_save, int band_mcu_rows) {
    __shared__ lep4::Dec4Shared sh;
    const int s = blockIdx.x, lane = threadIdx.x;
    const SegDev seg = segs[s];
    lep4::Dec4Resume* rec = recs + seg.slot;
    const int state = rec->state;
    if (state != lep4::kRowsFresh && state != lep4::kRowsRunning) return;
    const ImageDev* img = images + seg.image;
    uint32_t* model = models + (size_t)s * kModelStride;
    NSum* ns = ns_area + ns_offsets[s];
    if (state == lep4::kRowsFresh) {
        reset_segment_state<lep3::kModelWords>(model, ns, img->ns_total, lane);
        __syncthreads();
    }
    lep4::Dec4WaveT<SCMASK> w;
#ifdef LEP_PROF
    w.prof_begin(&g_prof4[s & 8191][0]);
#endif
    w.run_rows(img, seg, model, ns, &sh, streams + seg.stream_off, stream_len[seg.slot], rec, lds_save + (size_t)seg.slot * kRowsLdsWords, band_mcu_rows);
}


// ---- the split-phase encoder (lep_enc5.h) -------------------------------------------------------------------------------------
// walk: one or two wavefronts per segment (count / emit / gather share the code; NW = 2: lep_enc5.h Walk5); LDS: two transposed
// coefficient tiles, the tile's entry payloads and ranks, the stream cursors
template <int MODE, int NW>
__global__ __launch_bounds__(64 * NW) void lep_enc5_walk_kernel(const ImageDev* __restrict__ images, const SegDev* __restrict__ segs, NSum* ns_all,
                                                         const uint64_t* __restrict__ ns_off, lep5::SegPlan5* plans, uint8_t* arena, uint16_t* bins,
                                                         uint32_t* counts, int part, int nparts) {
    lep5::Walk5Shared* sh = reinterpret_cast<lep5::Walk5Shared*>(lep5::lep5_lds);   // dynamic LDS (walk_lds_bytes(MODE) at launch)
    const int s = blockIdx.x;
    const SegDev seg = segs[s];
    lep5::SegPlan5* P = plans + s;
    if (MODE == lep5::kGather && P->status) return;
    lep5::Walk5<MODE, NW> w;
    const int rc = w.run(images + seg.image, seg, ns_all + ns_off[s], sh, P, arena, bins, (int)(threadIdx.x >> 6), part, nparts);
    if (threadIdx.x >= 64) return;
    if (MODE == lep5::kCount) lep5::export_counts(w, sh, counts + (size_t)s * lep5::kCountWords);
    if (threadIdx.x == 0) {
        if (MODE == lep5::kEmit) P->status = rc;
        if (MODE == lep5::kGather && part + 1 == nparts) P->nbins = w.nbins;
    }
}
// the stitched writer (lep_enc5.h "write, stitched"): PHASE 0 range (lane = chunk), 1 link (lane = segment), 2 code (lane = chunk),
// 3 stitch (lane = segment); K chunks per segment
template <int PHASE>
__global__ __launch_bounds__(64) void lep_enc5_wchunk_kernel(const lep5::SegPlan5* __restrict__ plans, const uint16_t* __restrict__ bins, const SegDev* __restrict__ segs,
                                                         int nseg, int K, lep5::WChunk5* recs, uint8_t* streams, uint32_t* stream_len, int32_t* status, uint32_t* nbins_out) {
    const int id = (int)(blockIdx.x * 64 + threadIdx.x);
    if (PHASE == 0 || PHASE == 2) {
        const int seg = id / K, k = id - seg * K;
        if (seg >= nseg) return;
        if (PHASE == 2) __builtin_amdgcn_s_setprio(3);
        if (PHASE == 0) lep5::wchunk_range_lane(plans[seg], bins, recs + (size_t)seg * K + k, k, K);
        else lep5::wchunk_code_lane(plans[seg], bins, segs[seg], streams, recs + (size_t)seg * K + k, k, K);
    } else {
        if (id >= nseg) return;
        if (PHASE == 1) { status[segs[id].slot] = 0; nbins_out[segs[id].slot] = plans[id].nbins; lep5::wchunk_link_lane(plans[id], bins, recs + (size_t)id * K, K); }
        else lep5::wchunk_stitch_lane(plans[id], segs[id], streams, stream_len, status, recs + (size_t)id * K, K);
    }
}
// ... with the chunks cut at the boundaries of gather's parts (lep5::part_chunk_cut): the three phases of ONE part's c chunks, launched
// when that part is gathered and run beside the gather of the next -- PHASE 0 range and 2 code (lane = one of the part's chunks),
// 1 link (lane = segment; goes on from the part before).  Stitch is the kernel above over all nparts * c chunks.
template <int PHASE>
__global__ __launch_bounds__(64) void lep_enc5_wchunk_part_kernel(const lep5::SegPlan5* __restrict__ plans, const uint16_t* __restrict__ bins, const SegDev* __restrict__ segs,
                                                              int nseg, int nparts, int c, int part, lep5::WChunk5* recs, uint8_t* streams, const uint8_t* __restrict__ arena,
                                                              int32_t* status, uint32_t* nbins_out) {
    __builtin_amdgcn_s_setprio(3);   // (beside the next part's gather, like the lane-per-segment writer)
    const int id = (int)(blockIdx.x * 64 + threadIdx.x);
    const int seg = PHASE == 1 ? id : id / c, s = PHASE == 1 ? 0 : id - seg * c;
    if (seg >= nseg) return;
    const lep5::SegPlan5& P = plans[seg];
    const lep5::Ckpt5* ck = reinterpret_cast<const lep5::Ckpt5*>(arena + P.arena_off + P.ckpt_base);
    lep5::WChunk5* r = recs + (size_t)seg * (size_t)(nparts * c);
    if (PHASE == 0) lep5::wchunk_range_cut(P, bins, r + part * c + s, lep5::part_chunk_cut(P, ck, part, s, nparts, c));
    else if (PHASE == 2) lep5::wchunk_code_cut(P, bins, segs[seg], streams, r + part * c + s, lep5::part_chunk_cut(P, ck, part, s, nparts, c));
    else {
        if (part == 0) status[segs[seg].slot] = 0;
        if (part + 1 == nparts) nbins_out[segs[seg].slot] = P.nbins;
        lep5::wchunk_link_cuts(P, bins, r, part * c, (part + 1) * c, [&](int j) { return lep5::part_chunk_cut(P, ck, j / c, j % c, nparts, c); });
    }
}
// counts -> per-segment layout (one thread per segment), then the prefix over the segments (one wavefront)
__global__ void lep_enc5_plan_kernel(const uint32_t* __restrict__ counts, lep5::SegPlan5* plans, int nseg) {
    const int s = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (s < nseg) lep5::plan_segment(counts + (size_t)s * lep5::kCountWords, plans + s);
}
__global__ __launch_bounds__(64) void lep_enc5_offsets_kernel(lep5::SegPlan5* plans, int nseg, uint64_t* totals) {
    uint64_t a = 0, b = 0;
    for (int s0 = 0; s0 < nseg; s0 += 64) {
        const int s = s0 + (int)threadIdx.x;
        const uint32_t ab = s < nseg ? plans[s].arena_bytes : 0u, bc = s < nseg ? plans[s].bins_cap : 0u;
        int oa, ob;
        const int va = (int)(ab >> 8), vb = (int)(bc >> 7);   // (both are multiples of 256 / 128: the scan runs on 32-bit values)
        const int ta = lepwave::wave_excl_scan(&va, &oa), tb = lepwave::wave_excl_scan(&vb, &ob);
        if (s < nseg) { plans[s].arena_off = a + ((uint64_t)(uint32_t)oa << 8); plans[s].bins_off = b + ((uint64_t)(uint32_t)ob << 7); }
        a += (uint64_t)(uint32_t)ta << 8; b += (uint64_t)(uint32_t)tb << 7;
    }
    if (threadIdx.x == 0) { totals[0] = a; totals[1] = b; }
}
__global__ void lep_enc5_fill_kernel(uint4* p, size_t n16, uint32_t v) {
    const uint4 x = make_uint4(v, v, v, v);
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x) p[i] = x;
}
// bucket: the sparse records of a segment -> one stream per chain (one wavefront per segment)
__global__ __launch_bounds__(64) void lep_enc5_bucket_kernel(const lep5::SegPlan5* __restrict__ plans, uint8_t* arena) {
    __shared__ lep5::BucketShared sh;
    lep5::bucket_wave(plans + blockIdx.x, arena, &sh);
}
// fold, coefficient chains: block = (64 consecutive segments, stream); 18 KB of LDS
struct Fold5CoefShared { uint16_t slice[lep5::kCoefSlice * 64]; };   // 18 KB: eight wavefronts per CU
__global__ __launch_bounds__(64) void lep_enc5_fold_coef_kernel(const lep5::SegPlan5* __restrict__ plans, uint8_t* arena, int nseg, int groups) {
    __shared__ Fold5CoefShared shc;
    const int grp = (int)blockIdx.x % groups, job = (int)blockIdx.x / groups;   // job = ci * 630 + row * 10 + k, rows 0..62
    const int ci = job / 630, row = (job % 630) / 10, k = job % 10;
    const int sid = lep5::stream_id(ci, row, k), seg = grp * 64 + (int)threadIdx.x;
    const bool work = seg < nseg && !plans[seg].status && plans[seg].cnt[sid] != 0;
    if (!__ballot(work)) return;
    lep5::fold_coef_wave(plans, arena, grp * 64, nseg, sid, reinterpret_cast<lep5::FoldShared*>(&shc));
}
// fold, the other chains, by the LDS their Branches take (a kernel's resident wavefronts are what its largest job leaves room for):
//   small  sign chains (long dependent chains: first), threshold chains (Branches in HBM), edge non-zero counts     12 KB
//   big    DC chains, 7x7 non-zero counts                                                                          25 KB
struct Fold5SmallShared { uint16_t slice[lep5::kEdgeNzSlice * 64]; };
__global__ __launch_bounds__(64) void lep_enc5_fold_small_kernel(const lep5::SegPlan5* __restrict__ plans, uint8_t* arena, uint32_t* thresh_models, int nseg, int groups, int job0) {
    __shared__ Fold5SmallShared shs;
    lep5::FoldShared* sh = reinterpret_cast<lep5::FoldShared*>(&shs);
    const int grp = (int)blockIdx.x % groups;
    int job = (int)blockIdx.x / groups + job0;
    const int seg0 = grp * 64;
    if (job < 2) { lep5::fold_sign_wave(plans, arena, seg0, nseg, job, sh); return; }
    job -= 2;
    if (job < 12) { const int ci = job / 6, lt = 2 + job % 6; lep5::fold_thresh_wave(plans, arena, thresh_models, seg0, nseg, lep5::stream_id(ci, 63, lt), ci, sh); return; }
    job -= 12;
    lep5::fold_edgenz_wave(plans, arena, seg0, nseg, job / 16, (job / 8) & 1, job & 7, sh);   // 32 jobs
}
constexpr int kFold5SmallJobs = 2 + 12 + 32;
__global__ __launch_bounds__(64) void lep_enc5_fold_big_kernel(const lep5::SegPlan5* __restrict__ plans, uint8_t* arena, int nseg, int groups, int job0) {
    __shared__ lep5::FoldShared sh;
    const int grp = (int)blockIdx.x % groups;
    int job = (int)blockIdx.x / groups + job0;
    const int seg0 = grp * 64;
    if (job < 12) { lep5::fold_dc_wave(plans, arena, seg0, nseg, job, &sh); return; }
    job -= 12;
    lep5::fold_nz_wave(plans, arena, seg0, nseg, job / 10, job % 10, &sh);   // 20 jobs
}
constexpr int kFold5BigJobs = 12 + 20;
// write: lane = segment
__global__ __launch_bounds__(64) void lep_enc5_write_kernel(const lep5::SegPlan5* __restrict__ plans, const uint16_t* __restrict__ bins, const SegDev* __restrict__ segs,
                                                          int nseg, uint8_t* streams, uint32_t* stream_len, int32_t* status, uint32_t* nbins_out, uint8_t* arena,
                                                          int part, int nparts) {
    __builtin_amdgcn_s_setprio(3);   // (128 wavefronts that run beside the next part's gather: one long dependency chain each)
    const int seg0 = (int)blockIdx.x * 64, seg = seg0 + (int)threadIdx.x;
    if (seg < nseg) {
        if (part == 0) status[segs[seg].slot] = 0;
        if (part + 1 == nparts) nbins_out[segs[seg].slot] = plans[seg].nbins;
    }
    lep5::write_wave(plans, bins, segs, seg0, nseg, streams, stream_len, status, arena, part, nparts);
}

// JPEG Huffman re-encode of decoded frames: one wavefront per thread segment (lep_huff.h)
__global__ __launch_bounds__(64, 8) void lep_huffman_encode_kernel(const lephuff::HuffImage* __restrict__ images,
                                                                   const lephuff::HuffSegment* __restrict__ segs, uint8_t* out,
                                                                   uint32_t* out_len, lephuff::HuffEnd* ends) {
    __shared__ lephuff::HuffShared sh;
    const int s = blockIdx.x;
    const lephuff::HuffSegment seg = segs[s];
    if (seg.pad & lephuff::kHuffSegSimt) return;   // the lane-per-unit kernels below own this segment
    if (seg.pad & lephuff::kHuffSegRefuse) {       // a truncated file's segment nobody on the GPU takes: said so, the host re-coder's
        if (threadIdx.x == 0) {
            out_len[s] = 0;
            if (ends) { lephuff::HuffEnd e; memset(&e, 0, sizeof e); e.pad = lephuff::kHuffEndRefused; ends[s] = e; }
        }
        return;
    }
    lephuff::HuffWave w;
    const uint32_t n = w.run(images + seg.image, seg, &sh, out);
    if (threadIdx.x == 0) out_len[s] = n;
    if (ends) w.export_end(ends + s);
}
// (the bit buffers are cleared by a kernel of our own: hipMemsetAsync of 2.5 GB held the calling thread until everything queued
// on the stream in front of it had run -- the decode kernel of the chunk, 1.1 s -- measured with LEP_BATCH_TRACE)
__global__ __launch_bounds__(256) void lep_zero_kernel(uint4* p, size_t n16) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x) p[i] = uint4{0u, 0u, 0u, 0u};
}
// byte runs that lie apart moved back to back (lep_pack.h): offsets, then one wavefront per run
__global__ __launch_bounds__(leppack::kScanLanes) void lep_pack_offsets_kernel(const uint32_t* __restrict__ len, int n, uint64_t* __restrict__ dst_off) {
    leppack::offsets([len](int i) { return len[i]; }, n, dst_off);
}
__global__ __launch_bounds__(64) void lep_pack_copy_kernel(const uint8_t* __restrict__ src, const uint64_t* __restrict__ src_off, const uint32_t* __restrict__ len,
                                                           int n, uint8_t* __restrict__ dst, uint64_t dst_cap, const uint64_t* __restrict__ dst_off) {
    if (dst_off[n] > dst_cap) return;
    const int i = (int)blockIdx.x;
    leppack::copy_run(src + src_off[i], dst + dst_off[i], len[i], threadIdx.x & 63u);
}
// coefficient frames -> 8-bit sample planes (lep_samples.h): four wavefronts per workgroup, each with a unit and an LDS tile of its own
__global__ __launch_bounds__(64 * lepsamples::kWavesPerGroup) void lep_samples_kernel(const lepsamples::PlaneRec* __restrict__ recs, const uint32_t* __restrict__ first, int nplanes) {
    __shared__ uint32_t tiles[lepsamples::kWavesPerGroup][lepsamples::kTileWords];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t unit = blockIdx.x * (uint32_t)lepsamples::kWavesPerGroup + (uint32_t)wave;
    if (unit >= first[nplanes]) return;
    lepsamples::wave_samples(recs, first, nplanes, unit, tiles[wave]);
}
__global__ __launch_bounds__(64 * lepsamples::kWavesPerGroup) void lep_samples_dc_kernel(const lepsamples::PlaneRec* __restrict__ recs, const uint32_t* __restrict__ first, int nplanes) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t unit = blockIdx.x * (uint32_t)lepsamples::kWavesPerGroup + (uint32_t)wave;
    if (unit >= first[nplanes]) return;
    lepsamples::wave_samples_dc(recs, first, nplanes, unit);
}
// sample planes -> pixels (lep_rgb.h): four wavefronts per workgroup, each with a unit of its own
__global__ __launch_bounds__(64 * leprgb::kWavesPerGroup) void lep_rgb_kernel(const leprgb::RgbRec* __restrict__ recs, const uint32_t* __restrict__ first, int nimg) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t unit = blockIdx.x * (uint32_t)leprgb::kWavesPerGroup + (uint32_t)wave;
    if (unit >= first[nimg]) return;
    leprgb::wave_rgb(recs, first, nimg, unit);
}
// ... with a window per run (lep_gpu_pack_window_device): the clipped lengths are made here, from the device's lengths, summed, and left in wlen
__global__ __launch_bounds__(leppack::kScanLanes) void lep_pack_window_offsets_kernel(const uint32_t* __restrict__ len, const uint32_t* __restrict__ skip,
                                                                                      const uint32_t* __restrict__ take, int n, uint32_t* __restrict__ wlen,
                                                                                      uint64_t* __restrict__ dst_off) {
    leppack::offsets([=](int i) { const uint32_t w = leppack::window_len(len[i], skip[i], take[i]); wlen[i] = w; return w; }, n, dst_off);
}
__global__ __launch_bounds__(64) void lep_pack_window_copy_kernel(const uint8_t* __restrict__ src, const uint64_t* __restrict__ src_off, const uint32_t* __restrict__ skip,
                                                                  const uint32_t* __restrict__ wlen, int n, uint8_t* __restrict__ dst, uint64_t dst_cap,
                                                                  const uint64_t* __restrict__ dst_off) {
    if (dst_off[n] > dst_cap) return;
    const int i = (int)blockIdx.x;
    leppack::copy_run(src + src_off[i] + skip[i], dst + dst_off[i], wlen[i], threadIdx.x & 63u);
}
// ... with one lane per run of MCUs (lep_huff_simt.h): count / place / code / stuff
template <bool WRITE>
__global__ __launch_bounds__(64) void lep_huffman_simt_encode_units_kernel(const lephuff::HuffImage* __restrict__ images, const lephuff::HuffSegment* __restrict__ segs,
                                                                           lephuff::SimtEncSeg* es, const lephuff::SimtEncWave* __restrict__ waves,
                                                                           uint32_t* unit_bits, uint8_t* scratch) {
    __shared__ lephuff::SimtEncShared sh;
    const lephuff::SimtEncWave w = waves[blockIdx.x];
    lephuff::simt_enc_units<WRITE>(images, segs, es + w.eseg, &sh, unit_bits, scratch, w.first_unit);
}
__global__ __launch_bounds__(64) void lep_huffman_simt_encode_place_kernel(const lephuff::HuffImage* __restrict__ images, const lephuff::HuffSegment* __restrict__ segs,
                                                                           lephuff::SimtEncSeg* es, uint32_t* unit_bits, uint32_t* unit_plain) {
    lephuff::simt_enc_place(images, segs, es + blockIdx.x, unit_bits, unit_plain);
}
__global__ __launch_bounds__(64) void lep_huffman_simt_encode_stuff_kernel(const lephuff::HuffImage* __restrict__ images, const lephuff::HuffSegment* __restrict__ segs,
                                                                           const lephuff::SimtEncSeg* __restrict__ es, uint8_t* scratch, uint8_t* out, uint32_t* out_len,
                                                                           lephuff::HuffEnd* ends) {
    lephuff::simt_enc_stuff(images, segs, es[blockIdx.x], scratch, out, out_len, ends);
}

// progressive files: one wavefront per (image, scan) (lep_huffprog.h)
__global__ __launch_bounds__(64, 8) void lep_huffman_progressive_encode_kernel(const lephuff::ProgImage* __restrict__ images,
                                                                               const lephuff::ProgScan* __restrict__ scans, uint8_t* out,
                                                                               uint32_t* corr, uint32_t* out_len) {
    __shared__ lephuff::ProgShared sh;
    const lephuff::ProgScan* sc = scans + blockIdx.x;
    if (sc->pad & (lephuff::kProgScanSimt | lephuff::kProgScanSeq)) return;   // the lane-per-unit kernels below / the sequential scan encoders own this scan
    lephuff::ProgWave w;
    const uint32_t n = w.run_scan(images + sc->image, sc, &sh, out, corr);
    if (threadIdx.x == 0) out_len[blockIdx.x] = n;
}
// scans of sequential frames, written by the sequential scan encoders as segments of their own: their byte counts to the scans' places, with
// the progressive writers' mark (bit 31) on a scan that outgrew its slot
__global__ void lep_huffprog_seq_lens_kernel(const uint32_t* __restrict__ which, const uint32_t* __restrict__ cap, const uint32_t* __restrict__ lens,
                                             const lephuff::HuffEnd* __restrict__ ends, int n, uint32_t* out_len) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    const bool over = ends[i].attempted > cap[i] || (ends[i].pad & (lephuff::kHuffEndCut | lephuff::kHuffEndRefused)) != 0;
    out_len[which[i]] = lens[i] | (over ? 0x80000000u : 0u);
}
// ... with one lane per run of blocks (lep_huffprog_simt.h): count / place / code / stuff, scans with and without a restart interval alike
template <bool WRITE>
__global__ __launch_bounds__(64) void lep_huffprog_simt_units_kernel(const lephuff::ProgImage* __restrict__ images, const lephuff::ProgScan* __restrict__ scans,
                                                                     const lephuff::ProgSimtScan* __restrict__ ps, const lephuff::ProgSimtWave* __restrict__ waves,
                                                                     uint32_t* unit_words, size_t units, uint8_t* scratch) {
    __shared__ lephuff::ProgSimtShared sh;
    const lephuff::ProgSimtWave w = waves[blockIdx.x];
    lephuff::ProgSimtUnits U;
    U.set(unit_words, units);
    lephuff::prog_simt_units<WRITE>(images, scans, ps + w.pscan, &sh, U, scratch, w.first_unit);
}
__global__ __launch_bounds__(64) void lep_huffprog_simt_place_kernel(const lephuff::ProgScan* __restrict__ scans, lephuff::ProgSimtScan* ps, uint32_t* unit_words, size_t units) {
    lephuff::ProgSimtUnits U;
    U.set(unit_words, units);
    lephuff::prog_simt_place(scans, ps + blockIdx.x, U);
}
// the bit buffers are cleared as far as the scans reach (pass 2 knows; the buffers are sized by what a scan MAY need, ten times that), and the
// marker maps behind them (an eighth of the buffer; workgroups count on through them)
__global__ __launch_bounds__(256) void lep_huffprog_simt_zero_kernel(const lephuff::ProgSimtScan* __restrict__ ps, uint8_t* scratch, uint32_t chunk16) {
    const lephuff::ProgSimtScan s = ps[blockIdx.x];
    const uint32_t need16 = (uint32_t)std::min<uint64_t>(((uint64_t)s.total_bits + 7) / 8 / 16 + 2, s.buf_bytes / 16), map16 = s.map_bytes / 16;
    uint4* p = reinterpret_cast<uint4*>(scratch + s.buf_off);
    const uint32_t i0 = blockIdx.y * chunk16, i1 = i0 + chunk16 < need16 + map16 ? i0 + chunk16 : need16 + map16;
    for (uint32_t i = i0 + threadIdx.x; i < i1; i += blockDim.x) p[i < need16 ? i : s.buf_bytes / 16 + (i - need16)] = uint4{0u, 0u, 0u, 0u};
}
__global__ void lep_huffprog_simt_assign_kernel(const lephuff::ProgSimtRegion* __restrict__ regions, int nregion, lephuff::ProgSimtScan* ps) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < nregion) lephuff::prog_simt_assign(regions[i], ps);
}
__global__ __launch_bounds__(64) void lep_huffprog_simt_stuff_kernel(const lephuff::ProgImage* __restrict__ images, const lephuff::ProgScan* __restrict__ scans,
                                                                     const lephuff::ProgSimtScan* __restrict__ ps, uint8_t* scratch, uint8_t* out, uint32_t* out_len) {
    lephuff::prog_simt_stuff(images, scans, ps[blockIdx.x], scratch, out, out_len);
}

// progressive files, encode direction: one wavefront per (image, scan) of one dependency level (lep_huffprogdec.h)
__global__ __launch_bounds__(64, 8) void lep_huffman_progressive_decode_kernel(const lephuff::ProgDecScan* __restrict__ scans, lephuff::HuffDecRow* rows) {
    __shared__ lephuff::HuffDecShared sh;
    lephuff::ProgDecWave w;
    w.run_scan<false>(scans + blockIdx.x, &sh, rows);
}
// the same two launches with the window of speculative codes (lep_huffprogdec_win.h) for the scans it takes (ProgDecScan.pad)
__global__ __launch_bounds__(64, 2) void lep_huffprogdec_win_kernel(const lephuff::ProgDecScan* __restrict__ scans, lephuff::HuffDecRow* rows) {
    __shared__ lephuff::ProgWinShared ws;
    __shared__ lephuff::HuffDecShared sh;
    const lephuff::ProgDecScan* sc = scans + blockIdx.x;
    if (sc->pad & lephuff::kProgDecWin) { lephuff::ProgWinWave w; w.run_scan_win<false>(sc, &ws, rows); }
    else { lephuff::ProgDecWave w; w.run_scan<false>(sc, &sh, rows); }
}
__global__ __launch_bounds__(64, 2) void lep_huffprogdec_win_pipelined_kernel(const lephuff::ProgDecScan* __restrict__ scans, lephuff::HuffDecRow* rows,
                                                                            const lephuff::ProgDeps* __restrict__ deps, uint32_t* progress, uint32_t* ticket) {
    __shared__ lephuff::ProgWinShared ws;
    __shared__ lephuff::HuffDecShared sh;
    uint32_t t = 0;
    if (threadIdx.x == 0) t = atomicAdd(ticket, 1u);
    const int k = __builtin_amdgcn_readfirstlane((int)t);
    const lephuff::ProgDecScan* sc = scans + k;
    // (the scans of a file run side by side, two or three wavefronts to a SIMD, and each is one chain bound by its own instruction
    // issue: the long ones -- luma AC scans, the file's critical path -- are served first)
    if (sc->to != 0) { if (sc->cmp[0] == 0) __builtin_amdgcn_s_setprio(3); else __builtin_amdgcn_s_setprio(1); }
    if (sc->pad & lephuff::kProgDecWin) { lephuff::ProgWinWave w; w.run_scan_win<true>(sc, &ws, rows, deps + k, progress, k); }
    else { lephuff::ProgDecWave w; w.run_scan<true>(sc, &sh, rows, deps + k, progress, k); }
}
// scans with restart intervals whose marker positions lie behind their slot (lep_huffprogdec_rst.h): one wavefront per PIECE -- a run of
// consecutive intervals -- of the scans of one dependency level; then one wavefront per scan makes its final record of what the pieces left.
// (The window form's registers and LDS: 8 KB of tables and ring per wavefront.  Unlike that form's launches these are thousands of
// wavefronts per file: four to a SIMD.)
__global__ __launch_bounds__(64, 4) void lep_huffprogdec_rst_kernel(const lephuff::ProgDecScan* __restrict__ scans, const lephuff::ProgRstScan* __restrict__ plans, int nscan,
                                                                   lephuff::ProgRstOut* outs, lephuff::HuffDecRow* rows) {
    __shared__ lephuff::ProgWinShared ws;
    // the piece's scan: the last one of the launch whose first piece is not behind it
    const uint32_t piece = plans[0].piece0 + blockIdx.x;
    int lo = 0, hi = nscan - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (plans[mid].piece0 <= piece) lo = mid; else hi = mid - 1;
    }
    const lephuff::ProgRstScan pl = plans[lo];
    const uint32_t first = (piece - pl.piece0) * pl.ipp;
    if (piece - pl.piece0 >= pl.npieces || first >= pl.nint) return;
    lephuff::ProgRstWave w;
    w.run_piece(scans + lo, &ws, rows, pl.nint, first, pl.nint - first < pl.ipp ? pl.nint - first : pl.ipp, outs + piece);
}
__global__ __launch_bounds__(64) void lep_huffprogdec_rst_reduce_kernel(const lephuff::ProgDecScan* __restrict__ scans, const lephuff::ProgRstScan* __restrict__ plans,
                                                                       const lephuff::ProgRstOut* outs, lephuff::HuffDecRow* rows) {
    lephuff::prog_rst_reduce(scans + blockIdx.x, plans + blockIdx.x, outs, rows);
}
// ... all levels in ONE launch: a scan waits, MCU row by MCU row, for the scans of its file it follows (lep_huffprogdec.h ProgDeps)
// (128 VGPRs: at 64 the waiting code's spills trip a register-pair alignment check in this compiler's backend; a launch of this
// kind is small, what it needs is a short chain)
// A workgroup does not take the scan of its own index: it draws a ticket when it STARTS and takes that scan.  A scan only waits for
// scans of a lower index (prog_scan_deps), i.e. for tickets drawn before its own -- workgroups that are running or done, whatever
// order the hardware starts workgroups in.  (Round 3 relied on index-order dispatch, which holds on this chip but is nobody's
// promise: ADVICE round 3.)
__global__ __launch_bounds__(64, 4) void lep_huffman_progressive_pipelined_kernel(const lephuff::ProgDecScan* __restrict__ scans, lephuff::HuffDecRow* rows,
                                                                                 const lephuff::ProgDeps* __restrict__ deps, uint32_t* progress, uint32_t* ticket) {
    __shared__ lephuff::HuffDecShared sh;
    uint32_t t = 0;
    if (threadIdx.x == 0) t = atomicAdd(ticket, 1u);
    const int k = __builtin_amdgcn_readfirstlane((int)t);
    lephuff::ProgDecWave w;
    w.run_scan<true>(scans + k, &sh, rows, deps + k, progress, k);
}

// JPEG Huffman scan decode: one wavefront per image (lep_huffdec.h)
// <= 64 VGPRs and 4.5 KB of LDS: one of these waves fits on a SIMD beside seven coder waves, and it runs at raised priority
// there (it is one long dependency chain per image; the coder waves around it are the throughput work)
__global__ __launch_bounds__(64, 8) void lep_huffman_decode_kernel(const lephuff::HuffDecImage* __restrict__ images, lephuff::HuffDecRow* rows) {
    __shared__ lephuff::HuffDecShared sh;
    __builtin_amdgcn_s_setprio(3);
    lephuff::HuffDecWave w;
    w.run(images + blockIdx.x, &sh, rows);
}

// One lane per subsequence (lep_huffdec_simt.h): guess / settle / place / write; a wavefront's 64 lanes are 64 consecutive
// subsequences of one image, whose tables the wavefront keeps in LDS.
__global__ __launch_bounds__(64) void lep_huffman_simt_settle_kernel(const lephuff::HuffDecImage* __restrict__ images, lephuff::SimtImage* si, const lephuff::SimtWave* waves,
                                                                     const lephuff::SimtSub* in, lephuff::SimtSub* out, int settle, lephuff::SimtSlots* slots) {
    __shared__ lephuff::SimtShared sh;
    // (the lanes' slot columns of blind images with more than four blocks per MCU: dynamic, so that a launch without such an image
    // asks for no more LDS than it ever did -- the launch code puts those images' wavefronts into launches of their own, with
    // sizeof(SimtColumns) of it)
    extern __shared__ __attribute__((aligned(16))) unsigned char simt_columns[];
    const lephuff::SimtWave w = waves[blockIdx.x];
    lephuff::simt_guess_or_settle(images + w.image, &sh, si + w.image, in + si[w.image].first, out + si[w.image].first, w.first_sub, settle, slots,
                                  reinterpret_cast<lephuff::SimtColumns*>(simt_columns));
}
__global__ __launch_bounds__(64) void lep_huffman_simt_place_kernel(const lephuff::HuffDecImage* __restrict__ images, lephuff::SimtImage* si, const lephuff::SimtSub* sub,
                                                                    lephuff::SimtPlace* place, int passes, lephuff::HuffDecRow* rows, const lephuff::SimtSlots* slots) {
    const int i = (int)blockIdx.x;
    lephuff::simt_place(images + i, si + i, sub + si[i].first, place + si[i].first, passes, rows, slots);
}
__global__ __launch_bounds__(64) void lep_huffman_simt_write_kernel(const lephuff::HuffDecImage* __restrict__ images, lephuff::SimtImage* si, const lephuff::SimtWave* waves,
                                                                    const lephuff::SimtSub* sub, const lephuff::SimtPlace* place, lephuff::HuffDecRow* rows) {
    __shared__ lephuff::SimtShared sh;
    __shared__ lephuff::SimtTile tile;
    const lephuff::SimtWave w = waves[blockIdx.x];
    lephuff::simt_write(images + w.image, &sh, &tile, si + w.image, sub + si[w.image].first, place + si[w.image].first, rows, w.first_sub);
}
__global__ void lep_huffman_simt_finish_kernel(const lephuff::HuffDecImage* __restrict__ images, int nimg, lephuff::HuffDecRow* rows, const lephuff::SimtImage* si) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < nimg) lephuff::simt_finish(images + i, si + i, rows);
}

}  // namespace

// ------------------------------------------------------------------------------------------------
struct lep_gpu {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    bool released = false;   // device side already given back (by lep_gpu_destroy or by the exit handler)
    lep5::Enc5Options opt;   // the encoder knobs (lep_enc5_plan.h: defaults, environment, what was measured)
    hipStream_t stream2 = nullptr, stream3 = nullptr;   // the split-phase encoder folds its long chains beside its many short ones
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_join3 = nullptr;
    int huffprog_pipeline = 1;          // LEP_HUFFPROG_PIPELINE=0: progressive scan decode level by level, whatever the launch size
    int huffprog_split = 0;             // LEP_HUFFPROG_SPLIT=1: level-by-level launches split by kind of scan (measurement aid)
    int huffprogdec_rst = 1;            // LEP_HUFFPROGDEC_RST=0: scans with restart intervals decoded by lep_huffprogdec.h whatever their descriptors carry
    uint32_t huffprogdec_rst_floor = lephuff::kRstPieceFloor;   // LEP_HUFFPROGDEC_RST_FLOOR: bytes of scan per piece (measurements)
    int huffprogdec_win = 1;            // LEP_HUFFPROGDEC_WIN=0: progressive scans decoded by lep_huffprogdec.h's uniform vector code only
    int huffprog_simt = 1;              // LEP_HUFFPROG_SIMT=0: every progressive scan's bytes from the wavefront-per-scan kernel (lep_huffprog.h)
    int huffprog_simt_rst = 1;          // LEP_HUFFPROG_SIMT_RST=0: scans with a restart interval from the wavefront-per-scan kernel
    uint32_t huffprog_forms[4] = {0, 0, 0, 0};   // the last progressive write's scans by form: lane, lane with intervals, wavefront, sequential
    int cut_progressive = 0;            // lep_gpu_cut_progressive / LEP_CUT_PROGRESSIVE=1: the batch calls take progressive files that end inside a scan on the scan kernels
    int stream_pack = 1;                // LEP_STREAM_PACK=0: lep_decompress_batch_stream fetches a band's bytes with one copy per segment, not packed (lep_pack.h)
    int huffenc_simt = 1;               // LEP_HUFFENC_SIMT=0: every segment's scan bytes from the wavefront-per-segment kernel (lep_huff.h)
    int simt_sub_bits = 0;              // LEP_HUFFDEC_SIMT_BITS: bits per subsequence of the lane-per-subsequence scan decoder (0 = from the launch's size)
    int huffprog_pipeline_max = 16384;  // LEP_HUFFPROG_PIPELINE_MAX: scans per launch up to which the levels go out as one pipelined launch (measured to 10240:
                                        // 1024 4K files, 798 -> 938 MB/s; a workgroup takes the scan of the ticket it draws when it starts, so a scan's predecessors are always running or done)
    hipEvent_t ev_part[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int wchunks_parts = 0, wchunks_per_part = 0;   // the stitched writer's cut in the most recent encode launch (0: it used none) and that launch's
    std::vector<uint32_t> wchunks_slots;           // segments in launch order, as the caller counts them (lep_gpu_debug_wchunks)
    hipEvent_t ev_stage[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // stage boundaries of the last split-phase launch
    int nstage = 0;
    int dec_company = 0;     // lep_gpu_expect_company: decode launches will overlap with their neighbours on another stream
    int dec_waves = 0;       // register-budget build of the decoder: 0 = by batch size (8 waves per SIMD / 64 VGPRs once a launch can
                             // fill them, else 4 / 128 VGPRs, no spills); LEP_DEC_WAVES = 4 | 8 forces one
    std::string err;
    const char* last_kernel = "";   // name of the kernel the most recent launch used
    char simt_name[112] = "";       // ... of the lane-per-subsequence scan decoder: with the lanes and the subsequence length of that launch
    // Device memory the object owns (round 4): every large grow-only workspace below is a virtual address range of its own (hipMemAddressReserve)
    // into which physical chunks of 512 MB (hipMemCreate) are mapped as it grows -- growing maps more chunks behind what is there, nothing
    // is freed and taken again.  A workspace that is given back (lep_gpu_trim) is unmapped and its chunks go to the object's POOL, from
    // which the next workspace that grows takes them: memory moves between the encoder's scratch, the decoder's models and the rings
    // without passing through the driver.  Why that matters (MI355X, scripts/proto/vmm_costs.hip, profiles/r05m_*): the driver CLEARS
    // what it hands out -- hipMalloc of 96 GB takes 2.9 - 4.1 s, hipMemCreate the same per byte -- while unmapping 96 GB of chunks takes
    // 19 ms and mapping them again 14 ms.  Round 3's "2x cliff" after a trim was the next launch paying ~40 ms per GB for ~140 GB again.
    // Only lep_gpu_release_memory (and an allocation that fails elsewhere) hands the pool to the driver.  LEP_VMM=0: plain hipMalloc /
    // hipFree as before (A/B).  A workspace's range and chunks are the buffer's own (lep_buffers.h, DevBuf::v).
    struct Vmm {
        bool on = false;
        size_t chunk = (size_t)512 << 20;   // (64 MB chunks cost the encoder 2 %: 470 -> 480 ms, more page-table fragments; 512 MB: as one hipMalloc -- profiles/r05q_*)
        hipMemAllocationProp prop;
        hipMemAccessDesc access;
        std::vector<hipMemGenericAllocationHandle_t> pool;   // chunks of workspaces that were given back (lep_gpu_trim): unmapped, still ours --
                                                             // the next workspace that grows, of whatever kind, maps them again
        size_t mapped_total = 0, creates = 0, releases = 0;
    } vmm;
    // Every device workspace of the object, once: release_device_side, lep_gpu_trim and release_idle_caches walk ws[].  A name with _1
    // behind it is one of a pair (W_X + k): one per arena set, or two used in turn.
    enum Ws {
        // -- what lep_gpu_trim gives back: all of it is re-acquired by the next launch that needs it.  release_idle_caches takes the same,
        //    bar the models and summaries of the arena set a launch is being set up in.
        // split-phase encoder scratch: ONE set (a 4K image takes ~140 MB of it), shared by the two arena sets -- a split-phase launch
        // waits for the one before it (ev_enc5_done), which fills the chip on its own anyway
        W_ENC5_ENTRIES,             // the chains' entry streams, records, places
        W_ENC5_BINLIST,             // the segments' bin lists
        // grow-only device workspace of a coder launch (models, neighbour summaries; descriptors: W_META).  There are two sets so that two
        // launches may be in flight at once on different streams (lep_gpu_use_arena: the next chunk's coder kernel starts in the
        // wave slots that the long segments of the current one leave free); everything else uses set 0.
        W_MODELS, W_MODELS_1,
        W_NS, W_NS_1,
        W_TRIMMED,                  // -- what stays through a trim: from here on
        W_META = W_TRIMMED, W_META_1,   // ImageDev[] | SegDev[] | ns_offsets[] | bins[]
        W_ROWS, W_ROWS_1,           // a decode session's records: Dec4Resume[] | the segments' LDS-resident Branches (one per arena set)
        W_ENC5_PLANS,               // SegPlan5[] | counts | totals
        W_ENC5_WCHUNKS,             // the stitched writer's records, one per (segment, chunk)
        // host-variant staging
        W_BLOCKS, W_STREAMS, W_LENS,
        // HuffImage[] | HuffSegment[], one per arena set: the batch compressor's round-trip check writes the scans of chunk k and of chunk k + 1 on two
        // streams (lep_gpu_use_arena picks the set), and a short chunk k + 1 reaches its scan encoder before a long chunk k does -- with one buffer its
        // descriptors replaced the ones chunk k's kernels were still to read (a memory fault in tests/test_gpu_parity.py::*overlapped_launches, once,
        // round 6: the scans of sequential frames in several scans come through here a second time per chunk)
        W_HUFF, W_HUFF_1,
        W_HUFFENC, W_HUFFENC_1,     // lep_huff_simt.h: segment / wave descriptors, unit bit counts, bit buffers (one per arena set, like W_HUFF)
        W_HUFFPROG, W_HUFFPROG_1,   // ProgImage[] | ProgScan[], one per turn (two launches on two streams)
        W_HUFFPROGSIMT, W_HUFFPROGSIMT_1,   // lep_huffprog_simt.h: descriptors, unit arrays, bit buffers (one per turn)
        W_HUFFSEQ, W_HUFFSEQ_1,     // scans of sequential frames in a progressive launch: which / caps / byte counts / end states (one per turn)
        W_HUFFPROGDEC,              // ProgDecScan[]
        W_HUFFPROGRST,              // files with scans of lep_huffprogdec_rst.h: ProgDecScan[], ProgRstScan[], ProgRstOut[]
        W_HUFFDEC,                  // HuffDecImage[]
        W_HUFFPAR,                  // the lane-per-subsequence scan decoder's records (SimtImage | SimtWave | SimtSub x 2 | SimtPlace)
        W_PACK, W_PACK_1,           // lep_gpu_pack_device: the runs' source offsets (one per arena set, like W_HUFF)
        W_SAMPLES, W_SAMPLES_1,     // lep_gpu_samples_device: PlaneRec[] | first[] (one per arena set)
        W_RGB, W_RGB_1,             // lep_gpu_rgb_device: RgbRec[] | first[] (one per arena set)
        W_COUNT
    };
    lepbuf::DevBuf<> ws[W_COUNT];
    int cur = 0;                    // the arena set of the launches being set up (lep_gpu_use_arena)
    // a decode session per arena set (lep_gpu_decode_rows_begin .. _end): the launch it advances band by band
    struct RowsSession {
        bool open = false;
        int nseg = 0, waves = 4;
        hipStream_t st = nullptr;
        const ImageDev* d_img = nullptr; const SegDev* d_seg = nullptr; const uint64_t* d_nsoff = nullptr;
        uint32_t* d_models = nullptr; NSum* d_ns = nullptr;
        const uint8_t* d_streams = nullptr; const uint32_t* d_stream_len = nullptr;
        std::vector<lep4::Dec4Resume> h_recs;
    } rows[2];
    hipEvent_t ev_enc5_done = nullptr;
    uint32_t* d_bins = nullptr;
    std::vector<uint32_t> h_bins;
    struct Staging { void* host = nullptr; size_t cap = 0; hipEvent_t ev = nullptr; bool used = false; };
    Staging staging[16];                // pinned ring of staged descriptor blocks (stage()): a slot per block, at most five blocks per call (a
    int staging_next = 0;               // progressive write or decode that holds every kind of scan); nothing on a launch path waits for its stream
    std::vector<void*> staging_retired;
    int huffprog_turn = 0;   // the two sets are used in turn: at most two launches are ever in flight (lep_batch.hip queues chunk k+1 before it fetches chunk k)
};

#define HIPCHK(g, call)                                                                        \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) {                                                                \
            (g)->err = std::string(#call) + ": " + hipGetErrorString(e_);                      \
            return LEP_GPU_ERROR;                                                              \
        }                                                                                      \
    } while (0)

// ---- workspaces ------------------------------------------------------------------------------------------------------------------
static void vmm_init(lep_gpu* g) {
    g->vmm.on = false;
    if (const char* e = getenv("LEP_VMM")) if (atoi(e) == 0) return;
    int ok = 0;
    if (hipDeviceGetAttribute(&ok, hipDeviceAttributeVirtualMemoryManagementSupported, g->device) != hipSuccess || !ok) { (void)hipGetLastError(); return; }
    memset(&g->vmm.prop, 0, sizeof g->vmm.prop);
    g->vmm.prop.type = hipMemAllocationTypePinned;
    g->vmm.prop.location.type = hipMemLocationTypeDevice;
    g->vmm.prop.location.id = g->device;
    size_t gran = 0;
    if (hipMemGetAllocationGranularity(&gran, &g->vmm.prop, hipMemAllocationGranularityRecommended) != hipSuccess || !gran) { (void)hipGetLastError(); return; }
    if (const char* e = getenv("LEP_VMM_CHUNK_MB")) if (atoi(e) > 0) g->vmm.chunk = (size_t)atoi(e) << 20;
    g->vmm.chunk = ((g->vmm.chunk + gran - 1) / gran) * gran;
    g->vmm.access.location = g->vmm.prop.location;
    g->vmm.access.flags = hipMemAccessFlagsProtReadWrite;
    g->vmm.on = true;
}
typedef lepbuf::DevBuf<> Workspace;
// gives a workspace's range back: its chunks unmapped and pooled (or released to the driver), the address range kept for the next time it grows
static void vmm_unmap(lep_gpu* g, Workspace& w, bool to_driver = false) {
    lepbuf::VRange& b = w.v;
    if (b.mapped) (void)hipMemUnmap(b.va, b.mapped);
    for (hipMemGenericAllocationHandle_t h : b.chunks) {
        if (to_driver) { (void)hipMemRelease(h); ++g->vmm.releases; }
        else g->vmm.pool.push_back(h);
    }
    g->vmm.mapped_total -= b.mapped;
    b.chunks.clear(); b.mapped = 0;
    w.set(nullptr, 0);
}
static void vmm_drain_pool(lep_gpu* g) {
    for (hipMemGenericAllocationHandle_t h : g->vmm.pool) { (void)hipMemRelease(h); ++g->vmm.releases; }
    g->vmm.pool.clear();
}
static void dev_release(lep_gpu* g, Workspace& w) {
    if (w.v.va) vmm_unmap(g, w);
    else (void)w.release();
}
static void vmm_destroy(lep_gpu* g) {
    for (Workspace& w : g->ws) {
        if (!w.v.va) continue;
        vmm_unmap(g, w, true);
        (void)hipMemAddressFree(w.v.va, w.v.reserved);
        w.v = lepbuf::VRange();
    }
    vmm_drain_pool(g);
}
// before an allocation failure is reported: the cached memory no launch that is being set up depends on -- the split-phase
// encoder's scratch (its launches take the single-kernel encoder when they cannot have it) and the other arena set's models
static bool session_holds(const lep_gpu* g, int w) {   // the models and rings of an arena set with an open decode session
    for (int k = 0; k < 2; ++k)
        if (g->rows[k].open && (w == lep_gpu::W_MODELS + k || w == lep_gpu::W_NS + k)) return true;
    return false;
}
static void release_idle_caches(lep_gpu* g) {
    (void)hipDeviceSynchronize();
    for (int w = 0; w < lep_gpu::W_TRIMMED; ++w)
        if (w != lep_gpu::W_MODELS + g->cur && w != lep_gpu::W_NS + g->cur && !session_holds(g, w)) dev_release(g, g->ws[w]);
}
static int vmm_ensure(lep_gpu* g, Workspace& w, size_t need, bool may_release) {
    lep_gpu::Vmm& V = g->vmm;
    lepbuf::VRange& b = w.v;
    const size_t want = ((need + V.chunk - 1) / V.chunk) * V.chunk;
    if (want > b.reserved) {   // a longer address range (what the workspace held is not kept: every launch fills it anew)
        // The old range is unmapped and freed here, and launches do not wait for their streams any more (stage() ring; lep_batch.hip
        // queues chunk k + 1 while chunk k's kernels run): a kernel still in flight would lose its mapping under its feet.  hipFree
        // used to synchronise implicitly; this path has to ask.  Rare: growth inside the reservation maps behind.
        if (b.mapped) (void)hipDeviceSynchronize();
        vmm_unmap(g, w);
        if (b.va) (void)hipMemAddressFree(b.va, b.reserved);
        b.va = nullptr; b.reserved = 0;
        size_t res = want + want / 2;
        res = ((std::max(res, (size_t)256 << 20) + V.chunk - 1) / V.chunk) * V.chunk;
        void* va = nullptr;
        HIPCHK(g, hipMemAddressReserve(&va, res, 0, nullptr, 0));
        b.va = (char*)va; b.reserved = res;
    }
    const size_t old = b.mapped;
    while (b.mapped < want) {
        hipMemGenericAllocationHandle_t h;
        if (!V.pool.empty()) { h = V.pool.back(); V.pool.pop_back(); --V.creates; }
        else if (hipMemCreate(&h, V.chunk, &V.prop, 0) != hipSuccess) {
            (void)hipGetLastError();
            if (may_release) { may_release = false; release_idle_caches(g); if (!V.pool.empty()) continue; }   // the idle workspaces' chunks are in the pool now
            {   // no room: what this call mapped is given back, the workspace stays as it was
                while (b.mapped > old) { b.mapped -= V.chunk; (void)hipMemUnmap(b.va + b.mapped, V.chunk); V.pool.push_back(b.chunks.back()); b.chunks.pop_back(); V.mapped_total -= V.chunk; }
                g->err = "hipMemCreate: out of device memory";
                return LEP_GPU_ERROR;
            }
        }
        ++V.creates;
        if (hipMemMap(b.va + b.mapped, V.chunk, 0, h, 0) != hipSuccess) { (void)hipGetLastError(); (void)hipMemRelease(h); g->err = "hipMemMap failed"; return LEP_GPU_ERROR; }
        b.chunks.push_back(h); b.mapped += V.chunk; V.mapped_total += V.chunk;
    }
    if (b.mapped > old) HIPCHK(g, hipMemSetAccess(b.va + old, b.mapped - old, &V.access, 1));
    w.set(b.va, b.mapped);
    return 0;
}
static int ensure(lep_gpu* g, Workspace& w, size_t need, bool may_release = true) {
    if (w.cap >= need) return 0;
    // the large workspaces (models, rings, scratch: GBs) are owned address ranges with pooled chunks; descriptors and other small ones
    // (a chunk would be mostly slack) stay plain allocations
    if (g->vmm.on && (need >= ((size_t)32 << 20) || w.v.va)) {
        if (!w.v.va) HIPCHK(g, w.release());   // a plain buffer that turns virtual
        return vmm_ensure(g, w, need, may_release);
    }
    hipError_t e = w.ensure(need, need / 8);   // (the head room is a convenience: without it before giving up)
    if (e != hipSuccess && may_release) {
        (void)hipGetLastError();
        release_idle_caches(g);
        e = w.ensure(need);
    }
    if (e != hipSuccess) { g->err = std::string("hipMalloc: ") + hipGetErrorString(e); return LEP_GPU_ERROR; }
    return 0;
}

#include "lep_derive.h"


// The bool writer of a split-phase launch, as its plan (lep_enc5_plan.h) says: the kernels of one of the three forms on `wst`, in the
// encoder's order.  ready(p), p < gather_parts: part p's bins get to `binlist` and `wst` is put behind them; ready(gather_parts): every
// part's kernels are queued (launch_enc5 marks the stage there).  Also what lep_gpu_debug_write_bins runs on a test's lists.
template <class Ready>
static int launch_enc5_writer(const lep5::Enc5WriterPlan& W, const lep5::SegPlan5* plans, const uint16_t* binlist, const SegDev* segs, int nseg, lep5::WChunk5* recs,
                              uint8_t* arena, uint8_t* streams, uint32_t* stream_len, int32_t* status, uint32_t* bins, hipStream_t wst, Ready&& ready) {
#define LEP_WCHUNK(PHASE, GRID) hipLaunchKernelGGL((lep_enc5_wchunk_kernel<PHASE>), dim3(GRID), dim3(64), 0, wst, plans, binlist, segs, nseg, W.records, recs, streams, stream_len, status, bins)
#define LEP_WPART(PHASE, GRID) hipLaunchKernelGGL((lep_enc5_wchunk_part_kernel<PHASE>), dim3(GRID), dim3(64), 0, wst, plans, binlist, segs, nseg, \
                                                  W.gather_parts, W.chunks, part, recs, streams, (const uint8_t*)arena, status, bins)
    for (int part = 0; part < W.gather_parts; ++part) {
        if (int rc = ready(part)) return rc;
        if (W.form == LEP_DEBUG_WRITE_LANE)
            hipLaunchKernelGGL(lep_enc5_write_kernel, dim3(W.groups), dim3(64), 0, wst, plans, binlist, segs, nseg, streams, stream_len, status, bins, arena, part, W.gather_parts);
        if (W.form == LEP_DEBUG_WRITE_PART_CHUNKS) { LEP_WPART(0, W.lane_groups); LEP_WPART(1, W.groups); LEP_WPART(2, W.lane_groups); }
    }
    if (int rc = ready(W.gather_parts)) return rc;
    if (W.form == LEP_DEBUG_WRITE_STITCHED) { LEP_WCHUNK(0, W.lane_groups); LEP_WCHUNK(1, W.groups); LEP_WCHUNK(2, W.lane_groups); }
    if (W.form != LEP_DEBUG_WRITE_LANE) LEP_WCHUNK(3, W.groups);   // stitch: over all of a segment's records
#undef LEP_WPART
#undef LEP_WCHUNK
    return 0;
}

// The split-phase encoder (lep_enc5.h): count -> plan -> emit -> fold -> gather -> write.  One host synchronisation in the
// middle: the arena sizes come out of the count pass.  Stage boundaries are recorded as events (lep_gpu_last_stage_ms).
constexpr int kEnc5NoMemory = -1000;   // launch_enc5: the scratch could not be allocated (nothing has been written for the caller yet)
static int launch_enc5(lep_gpu* g, const ImageDev* d_img, const SegDev* d_seg, const uint64_t* d_nsoff, int nseg, uint8_t* d_streams,
                       uint32_t* d_stream_len, int32_t* d_status, hipStream_t st) {
    Workspace &models = g->ws[lep_gpu::W_MODELS + g->cur], &ns = g->ws[lep_gpu::W_NS + g->cur];
    Workspace &ws_plans = g->ws[lep_gpu::W_ENC5_PLANS], &ws_entries = g->ws[lep_gpu::W_ENC5_ENTRIES], &ws_binlist = g->ws[lep_gpu::W_ENC5_BINLIST], &wchunks = g->ws[lep_gpu::W_ENC5_WCHUNKS];
    if (!g->stream2) {
        HIPCHK(g, hipEventCreateWithFlags(&g->ev_enc5_done, hipEventDisableTiming));
        for (auto& e : g->ev_part) HIPCHK(g, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        HIPCHK(g, hipStreamCreateWithFlags(&g->stream2, hipStreamNonBlocking));
        HIPCHK(g, hipStreamCreateWithFlags(&g->stream3, hipStreamNonBlocking));
        HIPCHK(g, hipEventCreateWithFlags(&g->ev_fork, hipEventDisableTiming));
        HIPCHK(g, hipEventCreateWithFlags(&g->ev_join, hipEventDisableTiming));
        HIPCHK(g, hipEventCreateWithFlags(&g->ev_join3, hipEventDisableTiming));
        for (auto& e : g->ev_stage) HIPCHK(g, hipEventCreate(&e));
    }
    lepbuf::Layout L;
    L.add<lep5::SegPlan5>((size_t)nseg);
    const size_t o_counts = L.add<uint32_t>((size_t)nseg * lep5::kCountWords), o_tot = L.add<uint64_t>(2);
    HIPCHK(g, hipStreamWaitEvent(st, g->ev_enc5_done, 0));   // (the scratch is the previous split-phase launch's until its writer is done)
    if (int rc = ensure(g, ws_plans, L.padded())) return rc;
    lep5::SegPlan5* plans = ws_plans.at<lep5::SegPlan5>(0);
    uint32_t* counts = ws_plans.at<uint32_t>(o_counts);
    uint64_t* d_tot = ws_plans.at<uint64_t>(o_tot);
    const int groups = (nseg + 63) / 64;
    g->nstage = 0;
    HIPCHK(g, hipEventRecord(g->ev_stage[0], st));
    const bool two = g->opt.enc5_waves == 2;
    lep5::Enc5WriterPlan W = lep5::enc5_writer_plan(nseg, g->opt);
    int nparts = lep5::enc5_lane_plan(nseg, g->opt).gather_parts;   // (what count is told; emit and gather: the plan's, settled below, once the records are there)
    auto walk =[&](int mode, uint8_t* entries, uint16_t* binlist, int part = 0) {
        size_t lds = lep5::walk_lds_bytes(mode);
        if (mode == lep5::kGather && g->opt.enc5_gather_wgs > 0) lds = std::max(lds, (size_t)(160 * 1024 / g->opt.enc5_gather_wgs) & ~(size_t)255);   // (measurement aid: fewer resident workgroups)
#define LEP_WALK(MODE, NW) hipLaunchKernelGGL((lep_enc5_walk_kernel<MODE, NW>), dim3(nseg), dim3(64 * NW), lds, st, d_img, d_seg, (NSum*)ns.p, d_nsoff, plans, entries, binlist, counts, part, nparts)
        if (mode == lep5::kCount) { if (two) LEP_WALK(lep5::kCount, 2); else LEP_WALK(lep5::kCount, 1); }
        else if (mode == lep5::kEmit) { if (two) LEP_WALK(lep5::kEmit, 2); else LEP_WALK(lep5::kEmit, 1); }
        else { if (two) LEP_WALK(lep5::kGather, 2); else LEP_WALK(lep5::kGather, 1); }
#undef LEP_WALK
    };
    walk(lep5::kCount, nullptr, nullptr);
    hipLaunchKernelGGL(lep_enc5_plan_kernel, dim3(groups), dim3(64), 0, st, (const uint32_t*)counts, plans, nseg);
    hipLaunchKernelGGL(lep_enc5_offsets_kernel, dim3(1), dim3(64), 0, st, plans, nseg, d_tot);
    // the threshold Branches are the only model state in HBM: 2 MB per segment, reset while the count pass is looked at
    hipLaunchKernelGGL(lep_enc5_fill_kernel, dim3(4096), dim3(256), 0, st, (uint4*)models.p, (size_t)nseg * lep5::kThreshWords / 4, kBranchInit);
    uint64_t tot[2] = {0, 0};
    HIPCHK(g, hipMemcpyAsync(tot, d_tot, sizeof tot, hipMemcpyDeviceToHost, st));
    HIPCHK(g, hipStreamSynchronize(st));
    // no room for the scratch (~140 MB per 4K image): the single-kernel encoder takes the launch -- it needs none
    if ((size_t)tot[0] + (size_t)tot[1] * 2 > g->opt.enc5_scratch_max || ensure(g, ws_entries, (size_t)tot[0] + 256, false) || ensure(g, ws_binlist, (size_t)tot[1] * 2 + 256, false)) {
        (void)hipGetLastError();
        g->err.clear();
        static bool told = false;
        if (!told) { told = true; fprintf(stderr, "lepton-mi355x: no room for the split-phase encoder's scratch (%.1f GB for %d segments): single-kernel encoder\n", ((double)tot[0] + 2.0 * (double)tot[1]) / 1e9, nseg); }
        return kEnc5NoMemory;
    }
    // (no room for a chunked writer's records: the lane-per-segment writer)
    if (W.records && ensure(g, wchunks, (size_t)nseg * W.records * sizeof(lep5::WChunk5) + 256, false)) { (void)hipGetLastError(); g->err.clear(); W = lep5::enc5_lane_plan(nseg, g->opt); }
    nparts = W.gather_parts;
    // (Segment groups on streams of their own -- one group's writer and folds beside the next group's walks -- were measured
    // and dropped: MI355X, 1024 x 4K, profiles/r04l_*: 1 group 784 ms, 2: 875, 4: 1232; launches this large do not share the chip.)
    {
        HIPCHK(g, hipEventRecord(g->ev_stage[1], st));
        walk(lep5::kEmit, (uint8_t*)ws_entries.p, nullptr);
        HIPCHK(g, hipEventRecord(g->ev_stage[2], st));
        hipLaunchKernelGGL(lep_enc5_bucket_kernel, dim3(nseg), dim3(64), 0, st, (const lep5::SegPlan5*)plans, (uint8_t*)ws_entries.p);
        HIPCHK(g, hipEventRecord(g->ev_fork, st));
        HIPCHK(g, hipStreamWaitEvent(g->stream2, g->ev_fork, 0));
        HIPCHK(g, hipStreamWaitEvent(g->stream3, g->ev_fork, 0));
        if (g->opt.enc5_fold_apart) {   // measurement aid (LEP_ENC5_FOLD_APART=1): every kind of chain as a launch of its own, one after the other
            const int small0[4] = {0, 2, 14, 46}, big0[3] = {0, 12, 32};   // sign | threshold | edge counts;  DC | 7x7 counts
            for (int i = 0; i < 3; ++i)
                hipLaunchKernelGGL(lep_enc5_fold_small_kernel, dim3((unsigned)groups * (small0[i + 1] - small0[i])), dim3(64), 0, st, (const lep5::SegPlan5*)plans, (uint8_t*)ws_entries.p,
                                   (uint32_t*)models.p, nseg, groups, small0[i]);
            for (int i = 0; i < 2; ++i)
                hipLaunchKernelGGL(lep_enc5_fold_big_kernel, dim3((unsigned)groups * (big0[i + 1] - big0[i])), dim3(64), 0, st, (const lep5::SegPlan5*)plans, (uint8_t*)ws_entries.p, nseg, groups, big0[i]);
        } else {
        hipLaunchKernelGGL(lep_enc5_fold_small_kernel, dim3((unsigned)groups * kFold5SmallJobs), dim3(64), 0, g->stream2, (const lep5::SegPlan5*)plans, (uint8_t*)ws_entries.p,
                           (uint32_t*)models.p, nseg, groups, 0);
        hipLaunchKernelGGL(lep_enc5_fold_big_kernel, dim3((unsigned)groups * kFold5BigJobs), dim3(64), 0, g->stream3, (const lep5::SegPlan5*)plans, (uint8_t*)ws_entries.p, nseg, groups, 0);
        }
        hipLaunchKernelGGL(lep_enc5_fold_coef_kernel, dim3((unsigned)groups * 1260u), dim3(64), 0, st, (const lep5::SegPlan5*)plans, (uint8_t*)ws_entries.p, nseg, groups);
        HIPCHK(g, hipEventRecord(g->ev_join, g->stream2));
        HIPCHK(g, hipEventRecord(g->ev_join3, g->stream3));
        HIPCHK(g, hipStreamWaitEvent(st, g->ev_join, 0));
        HIPCHK(g, hipStreamWaitEvent(st, g->ev_join3, 0));
        HIPCHK(g, hipEventRecord(g->ev_stage[3], st));
        // behind gather the writer follows it on the launch's stream; beside it, it runs on the second one, behind every part's event
        const hipStream_t wst = W.form == LEP_DEBUG_WRITE_STITCHED ? st : g->stream2;
        auto gathered = [&](int part) -> int {
            if (part == nparts) { HIPCHK(g, hipEventRecord(g->ev_stage[4], st)); return 0; }
            walk(lep5::kGather, (uint8_t*)ws_entries.p, (uint16_t*)ws_binlist.p, part);
            if (wst != st) { HIPCHK(g, hipEventRecord(g->ev_part[part], st)); HIPCHK(g, hipStreamWaitEvent(wst, g->ev_part[part], 0)); }
            return 0;
        };
        if (int rc = launch_enc5_writer(W, plans, (const uint16_t*)ws_binlist.p, d_seg, nseg, (lep5::WChunk5*)wchunks.p, (uint8_t*)ws_entries.p, d_streams, d_stream_len, d_status,
                                        g->d_bins, wst, gathered)) return rc;
        if (wst != st) { HIPCHK(g, hipEventRecord(g->ev_join, wst)); HIPCHK(g, hipStreamWaitEvent(st, g->ev_join, 0)); }
        HIPCHK(g, hipEventRecord(g->ev_stage[5], st));
        g->nstage = 5;
    }
    HIPCHK(g, hipEventRecord(g->ev_enc5_done, st));
    HIPCHK(g, hipGetLastError());
    g->wchunks_parts = W.report_parts; g->wchunks_per_part = W.chunks; g->last_kernel = W.name;
    return 0;
}

// The sizes of the descriptor types that are staged, as tests/test_stage_block.py walks them: a type that changes size stops the build here.
#define LEP_STAGED(T, N) static_assert(sizeof(T) == N, "a staged descriptor changed size: tests/test_stage_block.py WORKSPACES and tests/emu/stage_block_probe.cc ELEM_SIZES name it")
LEP_STAGED(ImageDev, 2208); LEP_STAGED(SegDev, 32); LEP_STAGED(lep_huff_image, 4272); LEP_STAGED(lep_huff_segment, 40); LEP_STAGED(lephuff::SimtEncSeg, 40);
LEP_STAGED(lephuff::SimtEncWave, 8); LEP_STAGED(lepsamples::PlaneRec, 176); LEP_STAGED(leprgb::RgbRec, 112); LEP_STAGED(lep_huffprog_image, 168); LEP_STAGED(lep_huffprog_scan, 4184);
LEP_STAGED(lephuff::ProgSimtScan, 48); LEP_STAGED(lephuff::ProgSimtWave, 8); LEP_STAGED(lephuff::ProgSimtRegion, 24); LEP_STAGED(lep_huffprogdec_scan, 5696);
LEP_STAGED(lephuff::ProgDeps, 16); LEP_STAGED(lephuff::ProgRstScan, 16); LEP_STAGED(lephuff::ProgRstOut, 24); LEP_STAGED(lep_huffdec_image, 5552);
LEP_STAGED(lephuff::SimtImage, 36); LEP_STAGED(lephuff::SimtWave, 8); LEP_STAGED(lephuff::SimtSub, 20); LEP_STAGED(lephuff::SimtPlace, 12); LEP_STAGED(lephuff::SimtSlots, 32);

// The one way descriptors get to the device: a block (lep_block.h: these arrays, at these offsets) into workspace `ws`, ordered on `st`,
// WITHOUT waiting for what is queued on it.  The workspace is ensured for the whole block; the block's image is packed into a pinned
// slot of the codec's own ring (the caller's arrays, and the launch function's vectors, may go away) and goes up from there as ONE
// copy.  A launch function that waited for its stream here -- hipMemcpyAsync from pageable memory, then hipStreamSynchronize -- waited
// for every kernel queued in front of it: in the batch decompressor that was the decode kernel of the chunk being launched (1 s),
// during which the host could have staged the next chunk (kernel trace of round 4: the decoder idle ~0.1 s per chunk).  A slot is
// reused sixteen blocks later -- a call stages at most five -- and its event says when its copy has run.
static int stage(lep_gpu* g, Workspace& ws, const lepbuf::Block& B, hipStream_t st) {
    if (int rc = ensure(g, ws, B.padded())) return rc;
    const size_t n = B.upload_bytes();
    if (!n) return 0;
    lep_gpu::Staging& sl = g->staging[g->staging_next];
    g->staging_next = (g->staging_next + 1) % 16;
    if (sl.used) { HIPCHK(g, hipEventSynchronize(sl.ev)); sl.used = false; }
    if (!sl.ev) HIPCHK(g, hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming));
    if (sl.cap < n) {
        // (a buffer that has become too small is kept until the codec is destroyed: hipHostFree waits for the device, i.e. for the
        // very kernels this function exists not to wait for -- measured: 1.1 s per chunk.  8 MB take the descriptors of a 1024-image launch.)
        if (sl.host) g->staging_retired.push_back(sl.host);
        sl.host = nullptr; sl.cap = 0;
        const size_t want = std::max<size_t>(n + n / 4 + 4096, (size_t)8 << 20);
        HIPCHK(g, hipHostMalloc(&sl.host, want, hipHostMallocDefault));
        sl.cap = want;
    }
    B.pack((char*)sl.host);
    HIPCHK(g, hipMemcpyAsync(ws.p, sl.host, n, hipMemcpyHostToDevice, st));
    HIPCHK(g, hipEventRecord(sl.ev, st));
    sl.used = true;
    return 0;
}

// A decode session (lep_gpu_decode_rows_begin .. _end) owns the arena set it was begun on: its models, rings and descriptors carry a
// half-decoded launch from one advance to the next, so everything else that would set up work in that set is refused until the end.
static int refuse_if_session(lep_gpu* g, const char* what) {
    if (!g->rows[g->cur].open) return 0;
    g->err = std::string(what) + ": arena set " + std::to_string(g->cur) + " belongs to a decode session until lep_gpu_decode_rows_end";
    return LEP_ASSERTION_FAILURE;
}

// The front of a coder launch: descriptors derived, the launch order chosen, models / rings / descriptors ensured in the current arena
// set and the descriptors queued for upload on `st`.
struct LaunchFront { const ImageDev* d_img; const SegDev* d_seg; const uint64_t* d_nsoff; uint32_t* d_models; NSum* d_ns; };
static int launch_front(lep_gpu* g, bool dec, const lep_image_desc* images, int nimg, const lep_segment* segs, int nseg,
                        const uint64_t* stream_offsets, hipStream_t st, LaunchFront* out) {
    std::vector<ImageDev> himg(nimg);
    for (int i = 0; i < nimg; ++i) {
        int rc = derive_image(images[i], &himg[i], !dec);
        if (rc) return rc;
    }
    std::vector<SegDev> hseg(nseg);
    std::vector<uint64_t> hns(nseg);
    uint64_t ns_total = 0;
    for (int s = 0; s < nseg; ++s)
        if (segs[s].image < 0 || segs[s].image >= nimg) return LEP_ASSERTION_FAILURE;
    // Launch order.  Workgroups are observed to go to the 8 XCDs round-robin (block b -> XCD b % 8, MI355X_MICROARCH.md
    // "Workgroup dispatch, XCD placement": a speed matter only, nothing here depends on it), and the caller's order is
    // image-major: with 8 thread segments per image, segment k of EVERY image would land on XCD k -- and photographs are not
    // uniform top to bottom (sky above, detail below: up to 2x the bins per row), so one XCD would be the straggler of every
    // launch.  Segment r of image m is therefore queued for XCD (r + m) % 8 and the queues are interleaved; SegDev.slot
    // carries the caller's index for the results.
    const bool permute = nseg > 8;
    std::vector<int> order(nseg);
    if (permute) {
        std::vector<int> q[8];
        int rank = 0;
        for (int s = 0; s < nseg; ++s) {
            rank = (s > 0 && segs[s].image == segs[s - 1].image) ? rank + 1 : 0;
            q[(rank + segs[s].image) & 7].push_back(s);
        }
        size_t at[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int i = 0; i < nseg;)
            for (int x = 0; x < 8 && i < nseg; ++x)
                if (at[x] < q[x].size()) order[i++] = q[x][at[x]++];
    } else {
        for (int s = 0; s < nseg; ++s) order[s] = s;
    }
    // Longest first.  A launch is over when its longest thread segment is, and the hardware hands workgroups out in launch order as
    // wave slots come free: with the long segments in front, the short ones of a mixed batch (1080p files beside 4K ones: a quarter of
    // the blocks) back-fill behind them -- in this launch when it has more segments than the chip holds wavefronts, and in the NEXT
    // chunk's launch, which the batch decompressor queues on a second stream (lep_batch.hip) -- instead of the other way round.  A
    // stable sort on the block count's size class (quarter octaves) keeps the XCD interleave above among near-equals, and a corpus whose
    // segments are within 1.5x of each other (the eight segments of equal-sized files differ by a block row) is launched exactly as before.
    if (nseg > 8) {
        std::vector<int> cls(nseg);
        int64_t lo = INT64_MAX, hi = 0;
        for (int s = 0; s < nseg; ++s) {
            const ImageDev& im = himg[segs[s].image];
            const int y1 = segs[s].is_last ? im.height[0] : std::min(segs[s].luma_y_end, im.height[0]);
            const int64_t w = std::max<int64_t>(1, (int64_t)std::max(0, y1 - segs[s].luma_y_start) * im.width[0]);
            lo = std::min(lo, w); hi = std::max(hi, w);
            int c = 0;
            for (int64_t v = w; v > 1; v >>= 1) c += 4;                       // 4 * floor(log2 w) ...
            const int64_t base = (int64_t)1 << (c / 4);
            c += w * 4 >= base * 7 ? 3 : (w * 2 >= base * 3 ? 2 : (w * 4 >= base * 5 ? 1 : 0));   // ... + the quarter inside the octave
            cls[s] = c;
        }
        if (hi * 2 > lo * 3) {
            std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cls[a] > cls[b]; });
        }
    }
    if (!dec) g->wchunks_slots.assign((size_t)nseg, 0u);
    for (int i = 0; i < nseg; ++i) {
        const int s = order[i];
        hseg[i].image = segs[s].image; hseg[i].y0 = segs[s].luma_y_start; hseg[i].y1 = segs[s].luma_y_end;
        hseg[i].is_last = segs[s].is_last;
        hseg[i].stream_off = stream_offsets[s];
        uint64_t cap = stream_offsets[s + 1] - stream_offsets[s];
        hseg[i].stream_cap = (uint32_t)(cap > 0xffffffffu ? 0xffffffffu : cap);
        hseg[i].slot = (uint32_t)s;
        if (!dec) g->wchunks_slots[(size_t)i] = (uint32_t)s;
        hns[i] = ns_total;
        ns_total += (uint64_t)himg[segs[s].image].ns_total;
    }
    HIPCHK(g, hipSetDevice(g->device));
    Workspace &models = g->ws[lep_gpu::W_MODELS + g->cur], &ns = g->ws[lep_gpu::W_NS + g->cur];
    if (int rc = ensure(g, models, (size_t)nseg * kModelStride * 4)) return rc;
    if (int rc = ensure(g, ns, (size_t)ns_total * sizeof(NSum) + 16)) return rc;
    lepbuf::Block B;
    const size_t o_img = B.add(himg.data(), (size_t)nimg), o_seg = B.add(hseg.data(), (size_t)nseg), o_ns = B.add(hns.data(), (size_t)nseg), o_bins = B.add<uint32_t>((size_t)nseg);
    Workspace& meta = g->ws[lep_gpu::W_META + g->cur];
    if (int rc = stage(g, meta, B, st)) return rc;
    g->d_bins = meta.at<uint32_t>(o_bins);
    g->h_bins.assign(nseg, 0);
    g->nstage = 0;
    out->d_img = meta.at<const ImageDev>(o_img); out->d_seg = meta.at<const SegDev>(o_seg); out->d_nsoff = meta.at<const uint64_t>(o_ns);
    out->d_models = (uint32_t*)models.p; out->d_ns = (NSum*)ns.p;
    return 0;
}

// waves per SIMD the decoder's register allocation is held to for a launch of nseg segments: more resident waves only pay once the
// batch can fill them (MI355X, 4K corpus: below ~4600 segments the 4-wave build, which does not spill, is faster)
static int decoder_waves(const lep_gpu* g, int nseg) {
    // (a launch that is to share the chip with the launch before or behind it -- lep_gpu_expect_company, the batch decompressor's
    // chunks on two streams -- takes the 64-VGPR build whatever its size: four 128-VGPR wavefronts hold a SIMD's whole register file,
    // and the other launch's wavefronts could not move into the wave slots they leave empty)
    if (g->dec_waves) return g->dec_waves;
    return (nseg > 4608 || (g->dec_company && nseg >= 64)) ? 8 : 4;
}

template <bool DEC>
static int launch(lep_gpu* g, const lep_image_desc* images, int nimg, const lep_segment* segs, int nseg, uint8_t* d_streams,
                  const uint64_t* stream_offsets, uint32_t* d_stream_len, int32_t* d_status, hipStream_t st) {
    if (nseg <= 0) return 0;
    if (int rc = refuse_if_session(g, DEC ? "decode launch" : "encode launch")) return rc;
    LaunchFront F;
    if (int rc = launch_front(g, DEC, images, nimg, segs, nseg, stream_offsets, st, &F)) return rc;
    Workspace &models = g->ws[lep_gpu::W_MODELS + g->cur], &ns = g->ws[lep_gpu::W_NS + g->cur];
    HIPCHK(g, hipEventRecord(g->ev0, st));
    if (DEC) {
#ifdef LEP_PROF
        { void* p = nullptr; if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_prof4)) == hipSuccess) (void)hipMemsetAsync(p, 0, sizeof(g_prof4), st); }
#endif
#define LEP_LAUNCH_DEC4(W)                                                                                                     \
    hipLaunchKernelGGL((lep_decode_v4_kernel<W>), dim3(nseg), dim3(64), 0, st, F.d_img, F.d_seg, (uint32_t*)models.p, (NSum*)ns.p, \
                       F.d_nsoff, d_streams, d_stream_len, d_status, g->d_bins)
        const int waves = decoder_waves(g, nseg);
        if (waves >= 8) { g->last_kernel = "lep_decode_v4_kernel<8>"; LEP_LAUNCH_DEC4(8); }
        else { g->last_kernel = "lep_decode_v4_kernel<4>"; LEP_LAUNCH_DEC4(4); }
#undef LEP_LAUNCH_DEC4
    } else {
#define LEP_LAUNCH_ENC3(KERNEL, THREADS)                                                                                       \
    hipLaunchKernelGGL(KERNEL, dim3(nseg), dim3(THREADS), 0, st, F.d_img, F.d_seg, (uint32_t*)models.p, (NSum*)ns.p, F.d_nsoff, \
                       d_streams, d_stream_len, d_status, g->d_bins)
        const lep5::EncChoice enc = lep5::enc_choice(nseg, g->opt);   // (lep_enc5_plan.h)
        g->wchunks_parts = g->wchunks_per_part = 0;
        const int rc = enc.split_phase ? launch_enc5(g, F.d_img, F.d_seg, F.d_nsoff, nseg, d_streams, d_stream_len, d_status, st) : kEnc5NoMemory;
        if (rc && rc != kEnc5NoMemory) return rc;
        if (!rc) {}
        else if (enc.waves == 2) { g->last_kernel = "lep_encode_v3x2_kernel"; LEP_LAUNCH_ENC3(lep_encode_v3x2_kernel, 128); }
        else if (enc.waves >= 8) { g->last_kernel = "lep_encode_v3_kernel<8>"; LEP_LAUNCH_ENC3((lep_encode_v3_kernel<8>), 64); }
        else { g->last_kernel = "lep_encode_v3_kernel<4>"; LEP_LAUNCH_ENC3((lep_encode_v3_kernel<4>), 64); }
#undef LEP_LAUNCH_ENC3
    }
    HIPCHK(g, hipGetLastError());
    HIPCHK(g, hipEventRecord(g->ev1, st));
    g->timed = true;
    return 0;
}

// The HIP runtime multiplexes a process's streams onto a few hardware queues -- four per device unless GPU_MAX_HW_QUEUES says
// otherwise -- and two streams that share one run their work one after the other.  The batch pipeline keeps seven streams busy (copies
// up, copies down, two coder launches, the scan decoder at raised priority, the split-phase encoder's two side streams): in the kernel
// and copy trace of round 4 (profiles/r05b_*, r05c_*) the encoder's gather and write parts, which overlap in a process with three
// streams, alternated strictly, and a chunk's upload waited for the previous chunk's decode kernel.  Eight queues unless the
// environment already chose; read by the runtime when it initialises, i.e. before this library's first HIP call.
__attribute__((constructor)) static void lep_runtime_defaults() { setenv("GPU_MAX_HW_QUEUES", "8", 0); }

extern "C" {

// Process exit.  The HIP runtime registers its own teardown with atexit() lazily, at the first HIP call -- i.e. AFTER the
// static objects of a host program were constructed, so it runs BEFORE their destructors.  A host that keeps its coder in a
// global (the reference does: g_encoder / g_decoder, jpgcoder.cc:428, 478) would call lep_gpu_destroy on a runtime that is
// already gone and hang in hipStreamSynchronize (seen on MI355X with oracle/_ref/lepton-mi355x: work done in 0.1 s, process
// never ended).  So the library registers its own atexit handler after the first successful create -- later than HIP's,
// hence run earlier -- which releases every live object while the runtime still works; lep_gpu_destroy on such an object
// afterwards only frees the host struct.
static std::mutex g_live_mu;
static std::vector<lep_gpu*> g_live;
static bool g_exit_hook = false;
static void release_device_side(lep_gpu* g);
static void release_all_at_exit() {
    std::lock_guard<std::mutex> lk(g_live_mu);
    for (lep_gpu* g : g_live) release_device_side(g);
    g_live.clear();
}

int lep_gpu_create(int device, lep_gpu** out) {
    lep_gpu* g = new lep_gpu;
    g->device = device;
    if (const char* e = getenv("LEP_DEC_WAVES")) g->dec_waves = atoi(e) == 4 ? 4 : (atoi(e) == 8 ? 8 : 0);
    lep5::enc5_options_from_env(&g->opt);
    if (const char* e = getenv("LEP_HUFFPROG_PIPELINE")) g->huffprog_pipeline = atoi(e);
    if (const char* e = getenv("LEP_HUFFPROG_PIPELINE_MAX")) g->huffprog_pipeline_max = atoi(e);
    if (const char* e = getenv("LEP_HUFFDEC_SIMT_BITS")) g->simt_sub_bits = std::max(0, atoi(e));
    if (const char* e = getenv("LEP_HUFFENC_SIMT")) g->huffenc_simt = atoi(e) != 0;
    if (const char* e = getenv("LEP_STREAM_PACK")) g->stream_pack = atoi(e) != 0;
    if (const char* e = getenv("LEP_CUT_PROGRESSIVE")) g->cut_progressive = atoi(e) != 0;
    if (const char* e = getenv("LEP_HUFFPROG_SIMT")) g->huffprog_simt = atoi(e) != 0;
    if (const char* e = getenv("LEP_HUFFPROG_SIMT_RST")) g->huffprog_simt_rst = atoi(e) != 0;
    if (const char* e = getenv("LEP_HUFFPROGDEC_WIN")) g->huffprogdec_win = atoi(e) != 0;
    if (const char* e = getenv("LEP_HUFFPROGDEC_RST")) g->huffprogdec_rst = atoi(e) != 0;
    if (const char* e = getenv("LEP_HUFFPROGDEC_RST_FLOOR")) g->huffprogdec_rst_floor = (uint32_t)std::max(1, atoi(e));
    if (const char* e = getenv("LEP_HUFFPROG_SPLIT")) g->huffprog_split = atoi(e) != 0;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= device) { delete g; return LEP_GPU_ERROR; }
    if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&g->stream) != hipSuccess ||
        hipEventCreate(&g->ev0) != hipSuccess || hipEventCreate(&g->ev1) != hipSuccess) { delete g; return LEP_GPU_ERROR; }
    vmm_init(g);
    {
        std::lock_guard<std::mutex> lk(g_live_mu);
        g_live.push_back(g);
        if (!g_exit_hook) { g_exit_hook = true; atexit(release_all_at_exit); }
    }
    *out = g;
    return 0;
}

static void release_device_side(lep_gpu* g) {
    if (g->released) return;
    g->released = true;
    (void)hipSetDevice(g->device);
    (void)hipStreamSynchronize(g->stream);
    if (g->ev_enc5_done) (void)hipEventDestroy(g->ev_enc5_done);
    for (auto& e : g->ev_part) if (e) (void)hipEventDestroy(e);
    for (auto& e : g->ev_stage) if (e) (void)hipEventDestroy(e);
    if (g->ev_fork) (void)hipEventDestroy(g->ev_fork);
    if (g->ev_join) (void)hipEventDestroy(g->ev_join);
    if (g->ev_join3) (void)hipEventDestroy(g->ev_join3);
    if (g->stream2) (void)hipStreamDestroy(g->stream2);
    if (g->stream3) (void)hipStreamDestroy(g->stream3);
    for (Workspace& w : g->ws) dev_release(g, w);
    vmm_destroy(g);
    if (g->ev0) (void)hipEventDestroy(g->ev0);
    if (g->ev1) (void)hipEventDestroy(g->ev1);
    if (g->stream) (void)hipStreamDestroy(g->stream);
    for (lep_gpu::Staging& sl : g->staging) { if (sl.host) (void)hipHostFree(sl.host); if (sl.ev) (void)hipEventDestroy(sl.ev); sl = lep_gpu::Staging(); }
    for (void* p : g->staging_retired) (void)hipHostFree(p);
    g->staging_retired.clear();
}

void lep_gpu_destroy(lep_gpu* g) {
    if (!g) return;
    {
        std::lock_guard<std::mutex> lk(g_live_mu);
        for (size_t i = 0; i < g_live.size(); ++i) if (g_live[i] == g) { g_live.erase(g_live.begin() + i); break; }
        release_device_side(g);   // a no-op when the exit handler got there first
    }
    delete g;
}

const char* lep_gpu_last_error(lep_gpu* g) { return g ? g->err.c_str() : "no gpu object"; }

int lep_gpu_encode_device(lep_gpu* g, const lep_image_desc* images, int nimg, const lep_segment* segs, int nseg,
                          uint8_t* d_streams, const uint64_t* stream_offsets, uint32_t* d_stream_len, int32_t* d_status,
                          void* hip_stream) {
    return launch<false>(g, images, nimg, segs, nseg, d_streams, stream_offsets, d_stream_len, d_status,
                         hip_stream ? (hipStream_t)hip_stream : g->stream);
}

int lep_gpu_decode_device(lep_gpu* g, const lep_image_desc* images, int nimg, const lep_segment* segs, int nseg,
                          const uint8_t* d_streams, const uint64_t* stream_offsets, const uint32_t* d_stream_len,
                          int32_t* d_status, void* hip_stream) {
    return launch<true>(g, images, nimg, segs, nseg, const_cast<uint8_t*>(d_streams), stream_offsets,
                        const_cast<uint32_t*>(d_stream_len), d_status, hip_stream ? (hipStream_t)hip_stream : g->stream);
}

// ---- resumable decode: a launch advanced one band of MCU rows at a time (lep_decode_v4_rows_kernel) -----------------------------------
// begin = the front of a decode launch + cleared records; advance = one band on the session's stream, waited for, records copied back;
// end gives the arena set back.  The host only ever reads what a completed launch left behind.
int lep_gpu_decode_rows_begin(lep_gpu* g, const lep_image_desc* images, int nimg, const lep_segment* segs, int nseg,
                              const uint8_t* d_streams, const uint64_t* stream_offsets, const uint32_t* d_stream_len, void* hip_stream) {
    if (!g) return LEP_GPU_ERROR;
    if (int rc = refuse_if_session(g, "lep_gpu_decode_rows_begin")) return rc;
    if (nseg <= 0 || nimg <= 0) { g->err = "lep_gpu_decode_rows_begin: nothing to decode"; return LEP_ASSERTION_FAILURE; }
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : g->stream;
    LaunchFront F;
    if (int rc = launch_front(g, true, images, nimg, segs, nseg, stream_offsets, st, &F)) return rc;
    Workspace& recs = g->ws[lep_gpu::W_ROWS + g->cur];
    lepbuf::Layout L;
    L.add<lep4::Dec4Resume>((size_t)nseg);
    L.add<uint32_t>((size_t)nseg * kRowsLdsWords);
    if (int rc = ensure(g, recs, L.bytes())) return rc;
    HIPCHK(g, hipMemsetAsync(recs.p, 0, L.bytes(), st));   // all zero = fresh
    lep_gpu::RowsSession& R = g->rows[g->cur];
    R.nseg = nseg; R.st = st; R.waves = decoder_waves(g, nseg);
    R.d_img = F.d_img; R.d_seg = F.d_seg; R.d_nsoff = F.d_nsoff; R.d_models = F.d_models; R.d_ns = F.d_ns;
    R.d_streams = d_streams; R.d_stream_len = d_stream_len;
    R.h_recs.assign((size_t)nseg, lep4::Dec4Resume());
    R.open = true;
    return 0;
}

int lep_gpu_decode_rows_advance(lep_gpu* g, int band_mcu_rows, lep_decode_progress* progress, int* running) {
    if (!g) return LEP_GPU_ERROR;
    lep_gpu::RowsSession& R = g->rows[g->cur];
    if (!R.open) { g->err = "lep_gpu_decode_rows_advance: no decode session on arena set " + std::to_string(g->cur); return LEP_ASSERTION_FAILURE; }
    HIPCHK(g, hipSetDevice(g->device));
    Workspace& ws = g->ws[lep_gpu::W_ROWS + g->cur];
    lep4::Dec4Resume* d_recs = ws.at<lep4::Dec4Resume>(0);
    lepbuf::Layout L;
    L.add<lep4::Dec4Resume>((size_t)R.nseg);
    uint32_t* d_lds = ws.at<uint32_t>(L.add<uint32_t>((size_t)R.nseg * kRowsLdsWords));
#define LEP_LAUNCH_ROWS(W)                                                                                                             \
    hipLaunchKernelGGL((lep_decode_v4_rows_kernel<W>), dim3(R.nseg), dim3(64), 0, R.st, R.d_img, R.d_seg, R.d_models, R.d_ns, R.d_nsoff, \
                       R.d_streams, R.d_stream_len, d_recs, d_lds, band_mcu_rows)
    if (R.waves >= 8) { g->last_kernel = "lep_decode_v4_rows_kernel<8>"; LEP_LAUNCH_ROWS(8); }
    else { g->last_kernel = "lep_decode_v4_rows_kernel<4>"; LEP_LAUNCH_ROWS(4); }
#undef LEP_LAUNCH_ROWS
    HIPCHK(g, hipGetLastError());
    HIPCHK(g, hipMemcpyAsync(R.h_recs.data(), d_recs, (size_t)R.nseg * sizeof(lep4::Dec4Resume), hipMemcpyDeviceToHost, R.st));
    HIPCHK(g, hipStreamSynchronize(R.st));
    int still = 0;
    for (int s = 0; s < R.nseg; ++s) {
        const lep4::Dec4Resume& r = R.h_recs[(size_t)s];
        const bool failed = r.state == lep4::kRowsFailed;
        const bool retired = r.state == lep4::kRowsRetired;
        if (r.state != lep4::kRowsFinished && !failed && !retired) ++still;
        if (!progress) continue;
        lep_decode_progress& p = progress[s];
        p.status = r.state == lep4::kRowsFinished ? 0 : (failed ? r.code : (retired ? -2 : -1));
        for (int c = 0; c < LEP_MAX_COMPONENTS; ++c) p.rows_done[c] = c < 3 ? r.rows_done[c] : 0;
        p.fail_component = failed ? r.fail_component : -1; p.fail_y = failed ? r.fail_y : -1; p.fail_x = failed ? r.fail_x : -1;
        p.bins = r.nbins;
    }
    if (running) *running = still;
    return 0;
}

// A segment the caller needs no more rows of: its record's state word becomes kRowsRetired, by a copy in stream order behind the band
// before, and the rows kernel leaves at its entry from then on.  Finished and failed segments keep their state.
int lep_gpu_decode_rows_retire(lep_gpu* g, const int32_t* seg_index, int n) {
    if (!g) return LEP_GPU_ERROR;
    lep_gpu::RowsSession& R = g->rows[g->cur];
    if (!R.open) { g->err = "lep_gpu_decode_rows_retire: no decode session on arena set " + std::to_string(g->cur); return LEP_ASSERTION_FAILURE; }
    if (n < 0 || (n > 0 && !seg_index)) { g->err = "lep_gpu_decode_rows_retire: a list of segment indices"; return LEP_ASSERTION_FAILURE; }
    for (int k = 0; k < n; ++k)
        if (seg_index[k] < 0 || seg_index[k] >= R.nseg) {
            g->err = "lep_gpu_decode_rows_retire: segment index " + std::to_string(seg_index[k]) + " is not one of the session's " + std::to_string(R.nseg);
            return LEP_ASSERTION_FAILURE;
        }
    HIPCHK(g, hipSetDevice(g->device));
    lep4::Dec4Resume* d_recs = g->ws[lep_gpu::W_ROWS + g->cur].at<lep4::Dec4Resume>(0);
    static const int32_t kRetired = lep4::kRowsRetired;
    for (int k = 0; k < n; ++k) {
        lep4::Dec4Resume& r = R.h_recs[(size_t)seg_index[k]];
        if (r.state != lep4::kRowsFresh && r.state != lep4::kRowsRunning) continue;
        HIPCHK(g, hipMemcpyAsync(&d_recs[seg_index[k]].state, &kRetired, sizeof kRetired, hipMemcpyHostToDevice, R.st));
        r.state = lep4::kRowsRetired;
    }
    return 0;
}

int lep_gpu_decode_rows_end(lep_gpu* g) {
    if (!g) return LEP_GPU_ERROR;
    lep_gpu::RowsSession& R = g->rows[g->cur];
    if (!R.open) { g->err = "lep_gpu_decode_rows_end: no decode session on arena set " + std::to_string(g->cur); return LEP_ASSERTION_FAILURE; }
    R.open = false;
    R.h_recs.clear();
    return 0;
}

static_assert(sizeof(lep_huff_image) == sizeof(lephuff::HuffImage) &&sizeof(lep_huff_segment) == sizeof(lephuff::HuffSegment) &&
              sizeof(lep_huff_end) == sizeof(lephuff::HuffEnd) && sizeof(lep_huff_end) == 16, "C ABI mirrors");

int lep_gpu_huffman_encode_device(lep_gpu* g, const lep_huff_image* images, int nimg, const lep_huff_segment* segs, int nseg,
                                  uint8_t* d_out, uint32_t* d_out_len, lep_huff_end* d_ends, void* hip_stream) {
    if (!g) return LEP_GPU_ERROR;
    if (nseg <= 0) return 0;
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : g->stream;
    HIPCHK(g, hipSetDevice(g->device));
    const int set = g->cur & 1;                            // (the arena set the caller chose: two launches on two streams never share descriptors or scratch)
    Workspace &huff = g->ws[lep_gpu::W_HUFF + set], &huffenc = g->ws[lep_gpu::W_HUFFENC + set];
    // which segments the lane-per-unit kernels take, and what they need: lep_huff_simt.h's plan; the wavefront-per-segment kernel keeps the others
    std::vector<lep_huff_segment> sv(segs, segs + nseg);
    lephuff::SimtEncPlan plan;
    lephuff::simt_enc_plan(reinterpret_cast<const lephuff::HuffImage*>(images), nimg, reinterpret_cast<lephuff::HuffSegment*>(sv.data()), nseg, g->huffenc_simt != 0, &plan);
    const auto& es = plan.es; const auto& waves = plan.waves;
    lepbuf::Block D, E;
    const size_t o_img = D.add(images, (size_t)nimg), o_seg = D.add(sv.data(), (size_t)nseg);
    const size_t o_es = E.add(es.data(), es.size()), o_wv = E.add(waves.data(), waves.size()),
                 o_ub = E.add<uint32_t>(plan.nunits * 2),   // (units: bit counts / positions, and the plain prefix sum of scans with restart intervals)
                 o_sc = E.add<uint8_t>(plan.scratch_bytes);
    if (int rc = stage(g, huff, D, st)) return rc;
    if (!es.empty()) {
        if (int rc = stage(g, huffenc, E, st)) return rc;
        hipLaunchKernelGGL(lep_zero_kernel, dim3(8192), dim3(256), 0, st, huffenc.at<uint4>(o_sc), plan.scratch_bytes / 16);   // (buf_bytes are multiples of 16)
    }
    const lephuff::HuffImage* di = huff.at<const lephuff::HuffImage>(o_img);
    const lephuff::HuffSegment* ds = huff.at<const lephuff::HuffSegment>(o_seg);
    HIPCHK(g, hipEventRecord(g->ev0, st));
    if (!es.empty()) {
        lephuff::SimtEncSeg* des = huffenc.at<lephuff::SimtEncSeg>(o_es);
        const lephuff::SimtEncWave* dwv = huffenc.at<const lephuff::SimtEncWave>(o_wv);
        uint32_t* dub = huffenc.at<uint32_t>(o_ub);
        uint8_t* dsc = huffenc.at<uint8_t>(o_sc);
        hipLaunchKernelGGL((lep_huffman_simt_encode_units_kernel<false>), dim3((unsigned)waves.size()), dim3(64), 0, st, di, ds, des, dwv, dub, dsc);
        hipLaunchKernelGGL(lep_huffman_simt_encode_place_kernel, dim3((unsigned)es.size()), dim3(64), 0, st, di, ds, des, dub, dub + plan.nunits);
        hipLaunchKernelGGL((lep_huffman_simt_encode_units_kernel<true>), dim3((unsigned)waves.size()), dim3(64), 0, st, di, ds, des, dwv, dub, dsc);
        hipLaunchKernelGGL(lep_huffman_simt_encode_stuff_kernel, dim3((unsigned)es.size()), dim3(64), 0, st, di, ds, (const lephuff::SimtEncSeg*)des, dsc, d_out, d_out_len,
                           (lephuff::HuffEnd*)d_ends);
    }
    if ((int)es.size() < nseg)
        hipLaunchKernelGGL(lep_huffman_encode_kernel, dim3(nseg), dim3(64), 0, st, di, ds, d_out, d_out_len, (lephuff::HuffEnd*)d_ends);
    HIPCHK(g, hipGetLastError());
    HIPCHK(g, hipEventRecord(g->ev1, st));
    g->timed = true;
    g->last_kernel = es.empty() ? "lep_huffman_encode_kernel" : "lep_huffman_simt_encode_{units,place,stuff}_kernel";
    return 0;
}

// Byte runs moved back to back (lep_pack.h).  Its one workspace, W_PACK of the current arena set, is no decode session's: like the scan
// writer above (W_HUFF, W_HUFFENC) it may be launched on a set whose session is open.
int lep_gpu_pack_device(lep_gpu* g, const uint8_t* d_src, const uint64_t* src_off, const uint32_t* d_len, int n, uint8_t* d_dst, uint64_t d_dst_cap,
                        uint64_t* d_dst_off, void* hip_stream) {
    if (!g) return LEP_GPU_ERROR;
    if (n < 0 || n > leppack::kMaxRuns || !d_dst_off || (n > 0 && (!src_off || !d_len || !d_src || !d_dst))) {
        g->err = "lep_gpu_pack_device: 0 <= n <= 16384 runs, with their arrays";
        return LEP_ASSERTION_FAILURE;
    }
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : g->stream;
    HIPCHK(g, hipSetDevice(g->device));
    if (n == 0) { HIPCHK(g, hipMemsetAsync(d_dst_off, 0, sizeof(uint64_t), st)); return 0; }
    Workspace& ws = g->ws[lep_gpu::W_PACK + (g->cur & 1)];
    lepbuf::Block B;
    const size_t o_src = B.add(src_off, (size_t)n);
    if (int rc = stage(g, ws, B, st)) return rc;
    hipLaunchKernelGGL(lep_pack_offsets_kernel, dim3(1), dim3(leppack::kScanLanes), 0, st, d_len, n, d_dst_off);
    hipLaunchKernelGGL(lep_pack_copy_kernel, dim3((unsigned)n), dim3(64), 0, st, d_src, ws.at<const uint64_t>(o_src), d_len, n, d_dst, d_dst_cap, (const uint64_t*)d_dst_off);
    HIPCHK(g, hipGetLastError());
    g->last_kernel = "lep_pack_{offsets,copy}_kernel";
    return 0;
}

// ... with a window per run: run i gives its bytes [win_skip[i], min(d_len[i], win_skip[i] + win_take[i])).  W_PACK holds
// src_off[n] | skip[n] | take[n] | the clipped lengths[n] (written by the offsets kernel).
int lep_gpu_pack_window_device(lep_gpu* g, const uint8_t* d_src, const uint64_t* src_off, const uint32_t* d_len, const uint32_t* win_skip, const uint32_t* win_take,
                               int n, uint8_t* d_dst, uint64_t d_dst_cap, uint64_t* d_dst_off, void* hip_stream) {
    if (!g) return LEP_GPU_ERROR;
    if (n < 0 || n > leppack::kMaxRuns || !d_dst_off || (n > 0 && (!src_off || !d_len || !win_skip || !win_take || !d_src || !d_dst))) {
        g->err = "lep_gpu_pack_window_device: 0 <= n <= 16384 runs, with their arrays";
        return LEP_ASSERTION_FAILURE;
    }
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : g->stream;
    HIPCHK(g, hipSetDevice(g->device));
    if (n == 0) { HIPCHK(g, hipMemsetAsync(d_dst_off, 0, sizeof(uint64_t), st)); return 0; }
    Workspace& ws = g->ws[lep_gpu::W_PACK + (g->cur & 1)];
    lepbuf::Block B;
    const size_t o_src = B.add(src_off, (size_t)n), o_skip = B.add(win_skip, (size_t)n), o_take = B.add(win_take, (size_t)n), o_wlen = B.add<uint32_t>((size_t)n);
    if (int rc = stage(g, ws, B, st)) return rc;
    hipLaunchKernelGGL(lep_pack_window_offsets_kernel, dim3(1), dim3(leppack::kScanLanes), 0, st, d_len, ws.at<const uint32_t>(o_skip),
                       ws.at<const uint32_t>(o_take), n, ws.at<uint32_t>(o_wlen), d_dst_off);
    hipLaunchKernelGGL(lep_pack_window_copy_kernel, dim3((unsigned)n), dim3(64), 0, st, d_src, ws.at<const uint64_t>(o_src), ws.at<const uint32_t>(o_skip),
                       ws.at<const uint32_t>(o_wlen), n, d_dst, d_dst_cap, (const uint64_t*)d_dst_off);
    HIPCHK(g, hipGetLastError());
    g->last_kernel = "lep_pack_window_{offsets,copy}_kernel";
    return 0;
}

// Coefficient frames in device memory -> 8-bit sample planes (lep_samples.h).  Like the pack kernels its one workspace, W_SAMPLES of the
// current arena set, is no decode session's: a caller that holds a session turns each finished band into samples with a row range.
int lep_gpu_samples_device(lep_gpu* g, const lep_image_desc* images, int nimg, int scale, const int32_t* row_first, const int32_t* row_end,
                           uint8_t* const* d_planes, const int32_t* pitch, void* hip_stream) {
    if (!g) return LEP_GPU_ERROR;
    auto refuse = [g](const std::string& what) { g->err = "lep_gpu_samples_device: " + what; return (int)LEP_ASSERTION_FAILURE; };
    if (scale != 1 && scale != 8) return refuse("scale " + std::to_string(scale) + " (1 or 8)");
    if (nimg < 0 || nimg > (1 << 20) || (nimg > 0 && (!images || !d_planes || !pitch)) || (!row_first != !row_end)) return refuse("images, planes and pitches, and both ends of the row ranges or neither");
    std::vector<lepsamples::PlaneRec> recs;
    std::vector<uint32_t> first(1, 0u);
    for (int i = 0; i < nimg; ++i) {
        const lep_image_desc& d = images[i];
        if (d.ncomp < 1 || d.ncomp > LEP_MAX_COMPONENTS) return refuse("image " + std::to_string(i) + " has " + std::to_string(d.ncomp) + " components");
        for (int c = 0; c < d.ncomp; ++c) {
            const int k = i * 3 + c;
            const std::string who = "image " + std::to_string(i) + " component " + std::to_string(c) + ": ";
            const int wb = d.width_blocks[c], hb = d.height_blocks[c];
            if (wb < 1 || hb < 1 || wb > (1 << 24) || hb > (1 << 24)) return refuse(who + std::to_string(wb) + " x " + std::to_string(hb) + " blocks");
            if (!d.blocks[c] || ((uintptr_t)d.blocks[c] & 15u) || !d_planes[k]) return refuse(who + "a frame (16-byte aligned) and a plane");
            if (pitch[k] < wb * 8 / scale) return refuse(who + "pitch " + std::to_string(pitch[k]) + " is less than the plane's width " + std::to_string(wb * 8 / scale));
            const int r0 = row_first ? row_first[k] : 0, r1 = row_end ? row_end[k] : hb;
            if (r0 < 0 || r1 < r0 || r1 > hb)
                return refuse(who + "block rows [" + std::to_string(r0) + ", " + std::to_string(r1) + ") are not rows of its " + std::to_string(hb));
            lepsamples::PlaneRec r;
            const uint64_t units = lepsamples::fill_plane(&r, d.blocks[c], d_planes[k], wb, pitch[k], r0, r1, d.qtable_zigzag[c], scale);
            if (units + first.back() > 0x7fffffffull) return refuse("more than 2^31 wavefront units in one call");
            recs.push_back(r);
            first.push_back(first.back() + (uint32_t)units);
        }
    }
    const uint32_t total = first.back();
    if (!total) return 0;   // nothing to write: empty row ranges
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : g->stream;
    HIPCHK(g, hipSetDevice(g->device));
    const int nplanes = (int)recs.size();
    Workspace& ws = g->ws[lep_gpu::W_SAMPLES + (g->cur & 1)];
    lepbuf::Block B;   // the records, the unit counts behind them
    const size_t o_recs = B.add(recs.data(), recs.size()), o_first = B.add(first.data(), first.size(), 4);
    if (int rc = stage(g, ws, B, st)) return rc;
    const lepsamples::PlaneRec* d_recs = ws.at<const lepsamples::PlaneRec>(o_recs);
    const uint32_t* d_first = ws.at<const uint32_t>(o_first);
    const unsigned groups = (total + lepsamples::kWavesPerGroup - 1) / lepsamples::kWavesPerGroup;
    HIPCHK(g, hipEventRecord(g->ev0, st));
    if (scale == 1) hipLaunchKernelGGL(lep_samples_kernel, dim3(groups), dim3(64 * lepsamples::kWavesPerGroup), 0, st, d_recs, d_first, nplanes);
    else hipLaunchKernelGGL(lep_samples_dc_kernel, dim3(groups), dim3(64 * lepsamples::kWavesPerGroup), 0, st, d_recs, d_first, nplanes);
    HIPCHK(g, hipGetLastError());
    HIPCHK(g, hipEventRecord(g->ev1, st));
    g->timed = true;
    g->last_kernel = scale == 1 ? "lep_samples_kernel" : "lep_samples_dc_kernel";
    return 0;
}

// Sample planes in device memory -> pixels (lep_rgb.h).  Like lep_gpu_samples_device its one workspace, W_RGB of the current arena set, is
// no decode session's: a caller that holds a session colours each finished band with a row range.
int lep_gpu_rgb_device(lep_gpu* g, const lep_rgb_image* images, int nimg, void* hip_stream) {
    if (!g) return LEP_GPU_ERROR;
    auto refuse = [g](const std::string& what) { g->err = "lep_gpu_rgb_device: " + what; return (int)LEP_ASSERTION_FAILURE; };
    if (nimg < 0 || nimg > (1 << 20) || (nimg > 0 && !images)) return refuse("images");
    std::vector<leprgb::RgbRec> recs;
    std::vector<uint32_t> first(1, 0u);
    for (int i = 0; i < nimg; ++i) {
        const lep_rgb_image& m = images[i];
        const std::string who = "image " + std::to_string(i) + ": ";
        if (m.ncomp != 1 && m.ncomp != 3) return refuse(who + std::to_string(m.ncomp) + " components (1 or 3)");
        if (m.width < 1 || m.height < 1 || m.width > 65535 || m.height > 65535) return refuse(who + std::to_string(m.width) + " x " + std::to_string(m.height) + " pixels");
        leprgb::RgbRec r;
        const int64_t units = leprgb::fill_image(&r, m.width, m.height, m.ncomp, m.h_samp, m.v_samp, m.convert, m.d_plane, m.plane_pitch, m.d_rgb, m.rgb_pitch, m.y_first, m.y_end);
        if (units < 0) return refuse(who + "sampling factors that are not 1..4 or no integral multiples of one another");
        if (!m.d_rgb) return refuse(who + "no output");
        const int row_bytes = m.width * (m.ncomp == 1 ? 1 : 3);
        if (m.rgb_pitch < row_bytes) return refuse(who + "rgb_pitch " + std::to_string(m.rgb_pitch) + " is less than a row's " + std::to_string(row_bytes) + " bytes");
        if (m.y_first < 0 || m.y_end < m.y_first || m.y_end > m.height)
            return refuse(who + "rows [" + std::to_string(m.y_first) + ", " + std::to_string(m.y_end) + ") are not rows of its " + std::to_string(m.height));
        for (int c = 0; c < m.ncomp; ++c) {
            if (!m.d_plane[c]) return refuse(who + "component " + std::to_string(c) + " has no plane");
            if (m.plane_pitch[c] < r.dw[c])
                return refuse(who + "component " + std::to_string(c) + ": pitch " + std::to_string(m.plane_pitch[c]) + " is less than its " + std::to_string(r.dw[c]) + " samples");
        }
        if ((uint64_t)units + first.back() > 0x7fffffffull) return refuse("more than 2^31 wavefront units in one call");
        recs.push_back(r);
        first.push_back(first.back() + (uint32_t)units);
    }
    const uint32_t total = first.back();
    if (!total) return 0;   // nothing to write: empty row ranges
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : g->stream;
    HIPCHK(g, hipSetDevice(g->device));
    Workspace& ws = g->ws[lep_gpu::W_RGB + (g->cur & 1)];
    lepbuf::Block B;   // the records, the unit counts behind them
    const size_t o_recs = B.add(recs.data(), recs.size()), o_first = B.add(first.data(), first.size(), 4);
    if (int rc = stage(g, ws, B, st)) return rc;
    const unsigned groups = (total + leprgb::kWavesPerGroup - 1) / leprgb::kWavesPerGroup;
    HIPCHK(g, hipEventRecord(g->ev0, st));
    hipLaunchKernelGGL(lep_rgb_kernel, dim3(groups), dim3(64 * leprgb::kWavesPerGroup), 0, st, ws.at<const leprgb::RgbRec>(o_recs), ws.at<const uint32_t>(o_first), nimg);
    HIPCHK(g, hipGetLastError());
    HIPCHK(g, hipEventRecord(g->ev1, st));
    g->timed = true;
    g->last_kernel = "lep_rgb_kernel";
    return 0;
}

static_assert(sizeof(lep_huffprogdec_scan) == sizeof(lephuff::ProgDecScan), "C ABI mirrors");

static int progdec_launch_scans(lep_gpu* g, const lephuff::ProgDecPlan::Levels& b, lep_huffdec_row* d_rows, hipStream_t st);
static int progdec_launch_by_level(lep_gpu* g, const lephuff::ProgDecPlan::Pieces& c, lep_huffdec_row* d_rows, hipStream_t st, bool time_from_here);

// Which scans go to which kernels, in which order, with which marks and dependencies: lep_scan_decode_plan.h's plan.  Here: the
// sequential frames' scans to the sequential decoders, then the files without a scan of the interval form, then those with one.
int lep_gpu_huffman_progressive_decode_device(lep_gpu* g, const lep_huffprogdec_scan* scans, int nscan, lep_huffdec_row* d_rows, void* hip_stream) {
    if (!g) return LEP_GPU_ERROR;
    if (nscan <= 0) return 0;
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : g->stream;
    HIPCHK(g, hipSetDevice(g->device));
    lephuff::ProgDecOptions o;
    o.lanes = !(getenv("LEP_HUFFDEC_SIMT") && atoi(getenv("LEP_HUFFDEC_SIMT")) == 0);
    o.win = g->huffprogdec_win != 0; o.rst = g->huffprogdec_rst != 0; o.piece_floor = g->huffprogdec_rst_floor;
    o.pipeline = g->huffprog_pipeline != 0; o.pipeline_max = g->huffprog_pipeline_max; o.split = g->huffprog_split != 0;
    lephuff::ProgDecPlan plan;
    if (lephuff::prog_dec_plan(reinterpret_cast<const lephuff::ProgDecScan*>(scans), nscan, o, &plan)) return LEP_ASSERTION_FAILURE;
    static_assert(sizeof(lep_huffdec_image) == sizeof(lephuff::HuffDecImage), "C ABI mirrors");
    for (uint64_t at : plan.declined) HIPCHK(g, hipMemsetAsync(d_rows + at, lephuff::kProgDecDeclinedFill, sizeof(lep_huffdec_row), st));
    const auto &many = plan.seq_lanes, &one = plan.seq_single;
    if (!many.empty()) { if (int rc = lep_gpu_huffman_decode_simt_device(g, reinterpret_cast<const lep_huffdec_image*>(many.data()), (int)many.size(), d_rows, st)) return rc; }
    if (!one.empty()) { if (int rc = lep_gpu_huffman_decode_device(g, reinterpret_cast<const lep_huffdec_image*>(one.data()), (int)one.size(), d_rows, st)) return rc; }
    if (!plan.b.sorted.empty()) { if (int rc = progdec_launch_scans(g, plan.b, d_rows, st)) return rc; }
    if (plan.c.plain.empty() && plan.c.rst.empty()) return 0;
    return progdec_launch_by_level(g, plan.c, d_rows, st, plan.b.sorted.empty());
}

// the scans of files that have a scan of lep_huffprogdec_rst.h's: dependency level after dependency level on the stream -- the pieces of
// the scans of that form, one launch of the window form's level-by-level kernel for the others -- and the reduce step behind the last
static int progdec_launch_by_level(lep_gpu* g, const lephuff::ProgDecPlan::Pieces& c, lep_huffdec_row* d_rows, hipStream_t st, bool time_from_here) {
    lepbuf::Block B;
    const size_t o_plain = B.add(c.plain.data(), c.plain.size()), o_rst = B.add(c.rst.data(), c.rst.size()), o_plan = B.add(c.plans.data(), c.plans.size()),
                 o_out = B.add<lephuff::ProgRstOut>((size_t)c.pieces);
    Workspace& ws = g->ws[lep_gpu::W_HUFFPROGRST];
    if (int rc = stage(g, ws, B, st)) return rc;
    if (time_from_here) HIPCHK(g, hipEventRecord(g->ev0, st));
    const lephuff::ProgDecScan* d_plain = ws.at<const lephuff::ProgDecScan>(o_plain);
    const lephuff::ProgDecScan* d_rst = ws.at<const lephuff::ProgDecScan>(o_rst);
    const lephuff::ProgRstScan* d_plan = ws.at<const lephuff::ProgRstScan>(o_plan);
    lephuff::ProgRstOut* d_out = ws.at<lephuff::ProgRstOut>(o_out);
    for (int lv = 0; lv < 64; ++lv) {
        const int np = c.pcut[lv + 1] - c.pcut[lv], nr = c.rcut[lv + 1] - c.rcut[lv];
        if (np > 0)
            hipLaunchKernelGGL(c.any_win ? lep_huffprogdec_win_kernel : lep_huffman_progressive_decode_kernel, dim3(np), dim3(64), 0, st, d_plain + c.pcut[lv], (lephuff::HuffDecRow*)d_rows);
        if (nr > 0)
            hipLaunchKernelGGL(lep_huffprogdec_rst_kernel, dim3(c.piece_cut(lv + 1) - c.piece_cut(lv)), dim3(64), 0, st, d_rst + c.rcut[lv], d_plan + c.rcut[lv], nr, d_out, (lephuff::HuffDecRow*)d_rows);
    }
    hipLaunchKernelGGL(lep_huffprogdec_rst_reduce_kernel, dim3((unsigned)c.rst.size()), dim3(64), 0, st, d_rst, d_plan, d_out, (lephuff::HuffDecRow*)d_rows);
    HIPCHK(g, hipGetLastError());
    HIPCHK(g, hipEventRecord(g->ev1, st));
    g->timed = true;
    g->last_kernel = "lep_huffprogdec_rst_kernel";
    return 0;
}

// progressive scans of files without that form: all levels as ONE pipelined launch, or level after level (stream order is the dependency)
static int progdec_launch_scans(lep_gpu* g, const lephuff::ProgDecPlan::Levels& b, lep_huffdec_row* d_rows, hipStream_t st) {
    const int nscan = (int)b.sorted.size();
    lepbuf::Block B;   // (the dependencies are read by the pipelined launch alone)
    const size_t o_scan = B.add(b.sorted.data(), (size_t)nscan), o_deps = b.pipelined ? B.add(b.deps.data(), (size_t)nscan) : B.add<lephuff::ProgDeps>((size_t)nscan),
                 o_prog = B.add<uint32_t>((size_t)nscan + 1);   // (+ the ticket counter behind the progress words)
    Workspace& progdec = g->ws[lep_gpu::W_HUFFPROGDEC];
    if (int rc = stage(g, progdec, B, st)) return rc;
    if (b.pipelined) HIPCHK(g, hipMemsetAsync(progdec.at<char>(o_prog), 0, (size_t)nscan * 4 + 4, st));
    HIPCHK(g, hipEventRecord(g->ev0, st));
    if (b.pipelined) {
        hipLaunchKernelGGL(b.any_win ? lep_huffprogdec_win_pipelined_kernel : lep_huffman_progressive_pipelined_kernel, dim3(nscan), dim3(64), 0, st,
                           progdec.at<const lephuff::ProgDecScan>(o_scan), (lephuff::HuffDecRow*)d_rows,
                           progdec.at<const lephuff::ProgDeps>(o_deps), progdec.at<uint32_t>(o_prog), progdec.at<uint32_t>(o_prog) + nscan);
        HIPCHK(g, hipGetLastError());
        HIPCHK(g, hipEventRecord(g->ev1, st));
        g->timed = true;
        g->last_kernel = b.any_win ? "lep_huffprogdec_win_pipelined_kernel" : "lep_huffman_progressive_pipelined_kernel";
        return 0;
    }
    for (size_t q = 0; q + 1 < b.cut.size(); ++q) {   // one launch per level (LEP_HUFFPROG_SPLIT: per level and kind of scan)
        const int n = b.cut[q + 1] - b.cut[q];
        if (n <= 0) continue;
        hipLaunchKernelGGL(b.any_win ? lep_huffprogdec_win_kernel : lep_huffman_progressive_decode_kernel, dim3(n), dim3(64), 0, st,
                           progdec.at<const lephuff::ProgDecScan>(o_scan) + b.cut[q], (lephuff::HuffDecRow*)d_rows);
    }
    HIPCHK(g, hipGetLastError());
    HIPCHK(g, hipEventRecord(g->ev1, st));
    g->timed = true;
    g->last_kernel = b.any_win ? "lep_huffprogdec_win_kernel" : "lep_huffman_progressive_decode_kernel";
    return 0;
}

static_assert(sizeof(lep_huffprog_image) == sizeof(lephuff::ProgImage) && sizeof(lep_huffprog_scan) == sizeof(lephuff::ProgScan), "C ABI mirrors");

int lep_gpu_huffman_progressive_encode_device(lep_gpu* g, const lep_huffprog_image* images, int nimg, const lep_huffprog_scan* scans, int nscan,
                                              uint8_t* d_out, uint32_t* d_corr, uint32_t* d_out_len, void* hip_stream) {
    if (!g) return LEP_GPU_ERROR;
    if (nscan <= 0) return 0;
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : g->stream;
    HIPCHK(g, hipSetDevice(g->device));
    const int turn = (g->huffprog_turn ^= 1);
    Workspace &prog = g->ws[lep_gpu::W_HUFFPROG + turn], &seq = g->ws[lep_gpu::W_HUFFSEQ + turn], &simt = g->ws[lep_gpu::W_HUFFPROGSIMT + turn];
    std::vector<lephuff::ProgScan> hscan((size_t)nscan);   // the scans as the device gets them: `pad` is edited below, before the block is staged
    memcpy(hscan.data(), scans, (size_t)nscan * sizeof(lep_huffprog_scan));
    lephuff::ProgScan* hs = hscan.data();
    for (uint32_t& c : g->huffprog_forms) c = 0;
    std::vector<uint32_t> file_bound((size_t)nscan);
    for (int i = 0; i < nscan; ++i) { file_bound[(size_t)i] = hs[i].pad; hs[i].pad = 0; }   // (the caller's field; on the device it says which kernel owns the scan)
    // scans of SEQUENTIAL frames coded in several scans (lep_huffprog.h sequential_scan_segment): the sequential scan encoders write them,
    // each scan an image with one segment; their byte counts are moved to the scans' places behind that launch
    std::vector<lep_huff_image> seq_img;
    std::vector<lep_huff_segment> seq_seg;
    std::vector<uint32_t> seq_which, seq_cap;
    for (int i = 0; i < nscan; ++i) {
        if (!lephuff::prog_is_sequential(hs[i])) continue;
        if (hs[i].image < 0 || hs[i].image >= nimg || hs[i].cmpc < 1 || hs[i].cmpc > 4) return LEP_ASSERTION_FAILURE;
        lephuff::HuffImage hi;
        lephuff::HuffSegment sg;
        lephuff::sequential_scan_segment(reinterpret_cast<const lephuff::ProgImage&>(images[hs[i].image]), hs[i], (int32_t)seq_img.size(), &hi, &sg);
        lep_huff_image ci; lep_huff_segment cs;
        memcpy(&ci, &hi, sizeof ci); memcpy(&cs, &sg, sizeof cs);
        seq_img.push_back(ci); seq_seg.push_back(cs);
        seq_which.push_back((uint32_t)i); seq_cap.push_back(hs[i].out_cap);
        hs[i].pad = lephuff::kProgScanSeq;
    }
    if (!seq_seg.empty()) {
        const size_t n = seq_seg.size();
        lepbuf::Block S;   // which | caps | byte counts | (16-byte aligned) end states
        const size_t o_which = S.add(seq_which.data(), n, 4), o_cap = S.add(seq_cap.data(), n, 4), o_len = S.add<uint32_t>(n, 4), o_end = S.add<lep_huff_end>(n, 16);
        if (int rc = stage(g, seq, S, st)) return rc;
        if (int rc = lep_gpu_huffman_encode_device(g, seq_img.data(), (int)n, seq_seg.data(), (int)n, d_out, seq.at<uint32_t>(o_len), seq.at<lep_huff_end>(o_end), st)) return rc;
        hipLaunchKernelGGL(lep_huffprog_seq_lens_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, seq.at<const uint32_t>(o_which), seq.at<const uint32_t>(o_cap),
                           seq.at<const uint32_t>(o_len), seq.at<const lephuff::HuffEnd>(o_end), (int)n, d_out_len);
        g->huffprog_forms[3] = (uint32_t)n;
        if ((int)n == nscan) { HIPCHK(g, hipGetLastError()); return 0; }
    }
    // which scans the lane-per-unit kernels take, and what they need: lep_huffprog_simt.h's plan; the wavefront-per-scan kernel keeps the others
    lephuff::ProgSimtPlan plan;
    lephuff::prog_simt_plan(reinterpret_cast<const lephuff::ProgImage*>(images), nimg, hs, nscan, file_bound.data(), g->huffprog_simt != 0, g->huffprog_simt_rst != 0, &plan);
    const auto& ps = plan.ps; const auto& waves = plan.waves; const auto& regions = plan.regions;
    g->huffprog_forms[0] = plan.forms[0]; g->huffprog_forms[1] = plan.forms[1];
    lepbuf::Block D, E;
    const size_t o_img = D.add(images, (size_t)nimg), o_scan = D.add(hs, (size_t)nscan);
    const size_t o_ps = E.add(ps.data(), ps.size()), o_wv = E.add(waves.data(), waves.size()), o_rg = E.add(regions.data(), regions.size()),
                 o_un = E.add<uint32_t>(plan.nunits * lephuff::prog_simt_unit_words(plan.intervals)), o_sc = E.add<uint8_t>(plan.scratch_bytes);
    g->huffprog_forms[2] = (uint32_t)((size_t)nscan - ps.size() - seq_seg.size());
    if (int rc = stage(g, prog, D, st)) return rc;
    if (!ps.empty()) { if (int rc = stage(g, simt, E, st)) return rc; }
    const lephuff::ProgImage* di = prog.at<const lephuff::ProgImage>(o_img);
    const lephuff::ProgScan* ds = prog.at<const lephuff::ProgScan>(o_scan);
    HIPCHK(g, hipEventRecord(g->ev0, st));
    if (!ps.empty()) {
        lephuff::ProgSimtScan* dps = simt.at<lephuff::ProgSimtScan>(o_ps);
        const lephuff::ProgSimtWave* dwv = simt.at<const lephuff::ProgSimtWave>(o_wv);
        uint32_t* dun = simt.at<uint32_t>(o_un);
        uint8_t* dsc = simt.at<uint8_t>(o_sc);
        uint32_t longest = 0;
        for (const lephuff::ProgSimtRegion& r : regions) longest = (uint32_t)std::max<uint64_t>(longest, r.bytes);
        const uint32_t chunk16 = 4096;   // 64 KB of a bit buffer per workgroup of the clearing kernel
        hipLaunchKernelGGL((lep_huffprog_simt_units_kernel<false>), dim3((unsigned)waves.size()), dim3(64), 0, st, di, ds, (const lephuff::ProgSimtScan*)dps, dwv, dun, plan.nunits, dsc);
        hipLaunchKernelGGL(lep_huffprog_simt_place_kernel, dim3((unsigned)ps.size()), dim3(64), 0, st, ds, dps, dun, plan.nunits);
        hipLaunchKernelGGL(lep_huffprog_simt_assign_kernel, dim3((unsigned)(regions.size() + 63) / 64), dim3(64), 0, st, simt.at<const lephuff::ProgSimtRegion>(o_rg), (int)regions.size(), dps);
        hipLaunchKernelGGL(lep_huffprog_simt_zero_kernel, dim3((unsigned)ps.size(), (longest / 16 + chunk16 - 1) / chunk16 + 1), dim3(256), 0, st, (const lephuff::ProgSimtScan*)dps, dsc, chunk16);
        hipLaunchKernelGGL((lep_huffprog_simt_units_kernel<true>), dim3((unsigned)waves.size()), dim3(64), 0, st, di, ds, (const lephuff::ProgSimtScan*)dps, dwv, dun, plan.nunits, dsc);
        hipLaunchKernelGGL(lep_huffprog_simt_stuff_kernel, dim3((unsigned)ps.size()), dim3(64), 0, st, di, ds, (const lephuff::ProgSimtScan*)dps, dsc, d_out, d_out_len);
    }
    if (ps.size() + seq_seg.size() < (size_t)nscan)
        hipLaunchKernelGGL(lep_huffman_progressive_encode_kernel, dim3(nscan), dim3(64), 0, st, di, ds, d_out, d_corr, d_out_len);
    HIPCHK(g, hipGetLastError());
    HIPCHK(g, hipEventRecord(g->ev1, st));
    g->timed = true;
    g->last_kernel = ps.empty() ? "lep_huffman_progressive_encode_kernel" : "lep_huffprog_simt_{units,place,stuff}_kernel";
    return 0;
}

static_assert(sizeof(lep_huffdec_image) == sizeof(lephuff::HuffDecImage) && sizeof(lep_huffdec_row) == sizeof(lephuff::HuffDecRow), "C ABI mirrors");

int lep_gpu_huffman_decode_device(lep_gpu* g, const lep_huffdec_image* images, int nimg, lep_huffdec_row* d_rows, void* hip_stream) {
    if (!g) return LEP_GPU_ERROR;
    if (nimg <= 0) return 0;
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : g->stream;
    HIPCHK(g, hipSetDevice(g->device));
    Workspace& huffdec = g->ws[lep_gpu::W_HUFFDEC];
    lepbuf::Block B;
    const size_t o_img = B.add(images, (size_t)nimg);
    if (int rc = stage(g, huffdec, B, st)) return rc;
    HIPCHK(g, hipEventRecord(g->ev0, st));
    hipLaunchKernelGGL(lep_huffman_decode_kernel, dim3(nimg), dim3(64), 0, st, huffdec.at<const lephuff::HuffDecImage>(o_img), (lephuff::HuffDecRow*)d_rows);
    HIPCHK(g, hipGetLastError());
    HIPCHK(g, hipEventRecord(g->ev1, st));
    g->timed = true;
    g->last_kernel = "lep_huffman_decode_kernel";
    return 0;
}

int lep_gpu_huffman_decode_simt_device(lep_gpu* g, const lep_huffdec_image* images, int nimg, lep_huffdec_row* d_rows, void* hip_stream) {
    if (!g) return LEP_GPU_ERROR;
    if (nimg <= 0) return 0;
    // subsequences, wavefronts and side array: lep_huffdec_simt.h's plan -- as many lanes as fill the chip a few times over (64 x the
    // wavefronts it holds, twice) unless LEP_HUFFDEC_SIMT_BITS says how long a subsequence is
    lephuff::SimtDecPlan plan;
    if (lephuff::simt_dec_plan(reinterpret_cast<const lephuff::HuffDecImage*>(images), nimg, g->simt_sub_bits, (uint64_t)64 * 8192 * 2, &plan)) return LEP_ASSERTION_FAILURE;
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : g->stream;
    HIPCHK(g, hipSetDevice(g->device));
    const size_t nsub_all = plan.nsub_all;
    lepbuf::Block D, P;
    const size_t o_img = D.add(images, (size_t)nimg);
    const size_t o_si = P.add(plan.si.data(), plan.si.size()), o_wv = P.add(plan.waves.data(), plan.waves.size()), o_s0 = P.add<lephuff::SimtSub>(nsub_all),
                 o_s1 = P.add<lephuff::SimtSub>(nsub_all), o_pl = P.add<lephuff::SimtPlace>(nsub_all), o_sl = P.add<lephuff::SimtSlots>(plan.nslots);
    Workspace &huffdec = g->ws[lep_gpu::W_HUFFDEC], &par = g->ws[lep_gpu::W_HUFFPAR];
    if (int rc = stage(g, huffdec, D, st)) return rc;
    if (int rc = stage(g, par, P, st)) return rc;
    const lephuff::HuffDecImage* di = huffdec.at<const lephuff::HuffDecImage>(o_img);
    lephuff::SimtImage* dsi = par.at<lephuff::SimtImage>(o_si);
    const lephuff::SimtWave* dwv = par.at<const lephuff::SimtWave>(o_wv);
    lephuff::SimtSub* buf[2] = {par.at<lephuff::SimtSub>(o_s0), par.at<lephuff::SimtSub>(o_s1)};
    lephuff::SimtPlace* dpl = par.at<lephuff::SimtPlace>(o_pl);
    lephuff::SimtSlots* dsl = par.at<lephuff::SimtSlots>(o_sl);
    const int nw = (int)plan.waves.size(), nw_plain = plan.nw_plain, nw_wide = nw - nw_plain;
    HIPCHK(g, hipEventRecord(g->ev0, st));
    for (int k = 0; k <= lephuff::kSimtSettle; ++k) {       // pass A (k = 0: nothing is read), then the settle passes
        const lephuff::SimtSub* in = buf[(k + 1) & 1];
        if (nw_plain) hipLaunchKernelGGL(lep_huffman_simt_settle_kernel, dim3(nw_plain), dim3(64), 0, st, di, dsi, dwv, in, buf[k & 1], k, dsl);
        if (nw_wide) hipLaunchKernelGGL(lep_huffman_simt_settle_kernel, dim3(nw_wide), dim3(64), sizeof(lephuff::SimtColumns), st, di, dsi, dwv + nw_plain, in, buf[k & 1], k, dsl);
    }
    const lephuff::SimtSub* fin = buf[lephuff::kSimtSettle & 1];
    hipLaunchKernelGGL(lep_huffman_simt_place_kernel, dim3(nimg), dim3(64), 0, st, di, dsi, fin, dpl, lephuff::kSimtSettle, (lephuff::HuffDecRow*)d_rows,
                       (const lephuff::SimtSlots*)dsl);
    hipLaunchKernelGGL(lep_huffman_simt_write_kernel, dim3(nw), dim3(64), 0, st, di, dsi, dwv, fin, (const lephuff::SimtPlace*)dpl, (lephuff::HuffDecRow*)d_rows);
    hipLaunchKernelGGL(lep_huffman_simt_finish_kernel, dim3((nimg + 255) / 256), dim3(256), 0, st, di, nimg, (lephuff::HuffDecRow*)d_rows, (const lephuff::SimtImage*)dsi);
    HIPCHK(g, hipGetLastError());
    HIPCHK(g, hipEventRecord(g->ev1, st));
    g->timed = true;
    // (lanes of the launch and the subsequence length it was cut with -- LEP_HUFFDEC_SIMT_BITS or the plan's rule: tests that force short
    // subsequences read here that they got them)
    snprintf(g->simt_name, sizeof g->simt_name, "lep_huffman_simt_{settle,place,write}_kernel (%zu lanes, %u bits)", nsub_all, (unsigned)plan.L);
    g->last_kernel = g->simt_name;
    return 0;
}

int lep_gpu_expect_company(lep_gpu* g, int on) {
    if (!g) return LEP_GPU_ERROR;
    g->dec_company = on ? 1 : 0;
    return 0;
}

int lep_gpu_use_arena(lep_gpu* g, int k) {
    if (!g || k < 0 || k > 1) return LEP_ASSERTION_FAILURE;
    g->cur = k;
    return 0;
}

// Called by a caller that is about to destroy HIP streams it passed to launch functions of this object (the batch pipelines' per-call
// streams): the upload ring's events were recorded on those streams, and an event whose stream is gone must not be waited on again --
// hipEventSynchronize then answers from freed memory (seen on the MI355X as "operation not permitted on an event last recorded in a
// capturing stream" from a call that never captures anything, one run in a few).  Waits for every slot's copy and forgets the events.
int lep_gpu_settle_uploads(lep_gpu* g) {
    if (!g) return LEP_GPU_ERROR;
    for (lep_gpu::Staging& sl : g->staging) {
        if (sl.used && sl.ev) (void)hipEventSynchronize(sl.ev);
        sl.used = false;
        if (sl.ev) { (void)hipEventDestroy(sl.ev); sl.ev = nullptr; }
    }
    (void)hipGetLastError();
    return 0;
}

int lep_gpu_sync(lep_gpu* g) {
    HIPCHK(g, hipSetDevice(g->device));
    HIPCHK(g, hipDeviceSynchronize());
    return 0;
}

const char* lep_gpu_last_kernel_name(lep_gpu* g) { return g ? g->last_kernel : ""; }
int lep_gpu_huffman_progressive_encode_forms(lep_gpu* g, uint32_t counts[4]) {
    if (!g || !counts) return LEP_GPU_ERROR;
    for (int i = 0; i < 4; ++i) counts[i] = g->huffprog_forms[i];
    return 0;
}
int lep_gpu_device(lep_gpu* g) { return g ? g->device : -1; }
int lep_gpu_stream_pack(lep_gpu* g) { return g ? g->stream_pack : 0; }
int lep_gpu_cut_progressive(lep_gpu* g, int on) {
    if (!g) return 0;
    if (on >= 0) g->cut_progressive = on != 0;
    return g->cut_progressive;
}
// "0000:c1:00.0" of the device the object was created on (hipDeviceGetPCIBusId): which physical GPU a rank of a multi-GPU run drives
int lep_gpu_pci_bus_id(lep_gpu* g, char* out, int cap) {
    if (!g || !out || cap < 16) return LEP_ASSERTION_FAILURE;
    HIPCHK(g, hipDeviceGetPCIBusId(out, cap, g->device));
    return 0;
}

double lep_gpu_last_kernel_ms(lep_gpu* g) {
    if (!g->timed) return -1.0;
    float ms = 0;
    if (hipEventSynchronize(g->ev1) != hipSuccess) return -1.0;
    if (hipEventElapsedTime(&ms, g->ev0, g->ev1) != hipSuccess) return -1.0;
    return ms;
}

// stage times of the most recent split-phase encode launch: count + plan, emit, fold, gather, write (ms; -1 when the launch was
// not one); returns the number of stages
int lep_gpu_last_stage_ms(lep_gpu* g, double* ms, int cap) {
    if (!g || g->nstage <= 0) return 0;
    if (hipEventSynchronize(g->ev_stage[g->nstage]) != hipSuccess) return 0;
    int n = 0;
    for (; n < g->nstage && n < cap; ++n) {
        float t = 0;
        ms[n] = hipEventElapsedTime(&t, g->ev_stage[n], g->ev_stage[n + 1]) == hipSuccess ? (double)t : -1.0;
    }
    return n;
}

// device self-test of the arithmetic that has no CPU twin (float-reciprocal division in lep3::prob_of); 0 = all exact
int lep_gpu_selftest(lep_gpu* g) {
    HIPCHK(g, hipSetDevice(g->device));
    uint32_t* d = nullptr;
    HIPCHK(g, hipMalloc((void**)&d, 4));
    HIPCHK(g, hipMemset(d, 0, 4));
    hipLaunchKernelGGL(lep_selftest_kernel, dim3(255), dim3(256), 0, g->stream, d);
    uint32_t h = 1;
    HIPCHK(g, hipMemcpyAsync(&h, d, 4, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(g, hipStreamSynchronize(g->stream));
    HIPCHK(g, hipFree(d));
    return h == 0 ? 0 : LEP_ASSERTION_FAILURE;
}

// diagnosis: the lane-per-unit scan encoder's work area as the last lep_gpu_huffman_encode_device left it (segment / wave descriptors,
// unit positions, plain prefix sums, bit buffers + marker maps; the layout is that function's), copied to `out`; returns the bytes copied.
// scripts/diag_scan_encode_isolate.py compares two builds of the library pass by pass with it.
size_t lep_gpu_debug_huffenc(lep_gpu* g, void* out, size_t cap) {
    if (!g || !g->ws[lep_gpu::W_HUFFENC + (g->cur & 1)].p) return 0;
    const Workspace& w = g->ws[lep_gpu::W_HUFFENC + (g->cur & 1)];
    if (hipSetDevice(g->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return 0;
    const size_t n = std::min(cap, w.cap);
    return hipMemcpy(out, w.p, n, hipMemcpyDeviceToHost) == hipSuccess ? n : 0;
}

// tests: the split-phase encoder's bool writer kernels on bin lists the caller gives, one list per segment, launched in launch_enc5's
// order in one of its three forms (include/lepton_mi355x.h).  The lists are laid out as gather leaves them (each 256-byte aligned with
// room to the next multiple of 128 bins, 256 bytes behind the last); for the forms in parts a small arena holds every segment's Ckpt5
// table and WriterState5, a part's bins reach the device when its turn comes (what lies behind them is still 0xA5) and SegPlan5::nbins is
// set before the last part, as gather's last part sets it.  Everything is memory of the call's own, on the object's stream.
namespace {
struct DebugDev {   // device allocations of one debug call: freed on every way out
    std::vector<void*> p;
    ~DebugDev() { for (void* q : p) (void)hipFree(q); }
    hipError_t get(void** out, size_t bytes) {
        *out = nullptr;
        const hipError_t e = hipMalloc(out, bytes ? bytes : 16);
        if (e == hipSuccess) p.push_back(*out);
        return e;
    }
};
}  // namespace
int lep_gpu_debug_write_bins(lep_gpu* g, int form, int parts, int chunks, int nseg, const uint16_t* bins, const uint32_t* nbins,
                             const uint64_t* stream_off, const uint32_t* stream_cap, const int32_t* plan_status, const uint32_t* part_first,
                             int guard, uint8_t* arena_out, size_t arena_bytes, uint32_t* stream_len, int32_t* status, void* wchunks) {
    if (!g) return LEP_GPU_ERROR;
    if (int rc = refuse_if_session(g, "lep_gpu_debug_write_bins")) return rc;
    const bool in_parts = form == LEP_DEBUG_WRITE_LANE || form == LEP_DEBUG_WRITE_PART_CHUNKS;
    bool ok = nseg >= 1 && nseg <= 65536 && bins && nbins && stream_off && stream_cap && arena_out && stream_len && status &&
              (form == LEP_DEBUG_WRITE_LANE || form == LEP_DEBUG_WRITE_STITCHED || form == LEP_DEBUG_WRITE_PART_CHUNKS);
    if (ok && in_parts) ok = parts >= 1 && parts <= (int)lep5::kMaxParts && (parts == 1 || part_first);
    if (ok && form == LEP_DEBUG_WRITE_STITCHED) ok = parts == 1 && chunks >= 1 && chunks <= 256;
    if (ok && form == LEP_DEBUG_WRITE_PART_CHUNKS) ok = chunks >= 1 && chunks <= 32;
    uint64_t end = 0;
    for (int s = 0; ok && s < nseg; ++s) {   // reservations: ascending, apart, inside the arena; part bounds: ascending from 0, inside the list
        ok = stream_off[s] >= end && stream_off[s] + stream_cap[s] <= arena_bytes && nbins[s] < (1u << 28);
        end = stream_off[s] + stream_cap[s];
        for (int p = 0; ok && in_parts && parts > 1 && p < parts; ++p) {
            const uint32_t b = part_first[(size_t)s * parts + p];
            ok = p == 0 ? b == 0 : (b >= part_first[(size_t)s * parts + p - 1] && b <= nbins[s]);
        }
    }
    if (!ok) { g->err = "lep_gpu_debug_write_bins: arguments out of range"; return LEP_ASSERTION_FAILURE; }
    HIPCHK(g, hipSetDevice(g->device));
    const lep5::Enc5WriterPlan W = lep5::enc5_writer_form(form, nseg, parts, chunks);
    constexpr uint32_t kSegArena = 1024;   // [kMaxParts] Ckpt5 | WriterState5
    static_assert(lep5::kMaxParts * sizeof(lep5::Ckpt5) + sizeof(lep5::WriterState5) <= kSegArena, "a segment's checkpoints and writer state");
    std::vector<lep5::SegPlan5> plans((size_t)nseg);
    std::vector<SegDev> segs((size_t)nseg);
    std::vector<uint8_t> h_arena((size_t)nseg * kSegArena, 0xEE);
    std::vector<uint64_t> first((size_t)nseg + 1, 0);   // where the caller's lists start in `bins`
    uint64_t total = 0;
    for (int s = 0; s < nseg; ++s) {
        lep5::SegPlan5& P = plans[(size_t)s];
        memset(&P, 0, sizeof P);
        P.arena_off = (uint64_t)s * kSegArena; P.ckpt_base = 0; P.wstate_base = (uint32_t)(lep5::kMaxParts * sizeof(lep5::Ckpt5)); P.arena_bytes = kSegArena;
        P.bins_off = total; P.bins_cap = (nbins[s] + 127u) & ~127u;
        P.nbins = in_parts && parts > 1 ? 0xEEEEEEEEu : nbins[s];   // (gather's last part writes it: nothing may ask for it before)
        P.status = plan_status ? plan_status[s] : 0;
        total += P.bins_cap;
        first[(size_t)s + 1] = first[(size_t)s] + nbins[s];
        lep5::Ckpt5* ck = reinterpret_cast<lep5::Ckpt5*>(h_arena.data() + P.arena_off);
        for (int p = 1; in_parts && p < parts; ++p) ck[p].nbins = part_first[(size_t)s * parts + p];
        SegDev& sd = segs[(size_t)s];
        memset(&sd, 0, sizeof sd);
        sd.stream_off = stream_off[s]; sd.stream_cap = stream_cap[s]; sd.slot = (uint32_t)s;
    }
    std::vector<lep5::SegPlan5> plans_last(plans);   // ... as they are once the last part is there
    for (int s = 0; s < nseg; ++s) plans_last[(size_t)s].nbins = nbins[s];
    std::vector<uint16_t> h_bins((size_t)total + 128, 0xA5A5);
    for (int s = 0; s < nseg; ++s)
        if (nbins[s]) memcpy(h_bins.data() + plans[(size_t)s].bins_off, bins + first[(size_t)s], (size_t)nbins[s] * 2);
    DebugDev dev;
    lep5::SegPlan5* d_plans; SegDev* d_segs; uint8_t *d_arena, *d_out; uint16_t* d_list; lep5::WChunk5* d_recs; uint32_t *d_len, *d_nb; int32_t* d_status;
    const size_t list_bytes = (size_t)total * 2 + 256, rec_bytes = (size_t)nseg * (size_t)std::max(W.records, 1) * sizeof(lep5::WChunk5);
    HIPCHK(g, dev.get((void**)&d_plans, plans.size() * sizeof(lep5::SegPlan5)));
    HIPCHK(g, dev.get((void**)&d_segs, segs.size() * sizeof(SegDev)));
    HIPCHK(g, dev.get((void**)&d_arena, h_arena.size()));
    HIPCHK(g, dev.get((void**)&d_list, list_bytes));
    HIPCHK(g, dev.get((void**)&d_recs, rec_bytes));
    HIPCHK(g, dev.get((void**)&d_out, arena_bytes));
    HIPCHK(g, dev.get((void**)&d_len, (size_t)nseg * 4));
    HIPCHK(g, dev.get((void**)&d_nb, (size_t)nseg * 4));
    HIPCHK(g, dev.get((void**)&d_status, (size_t)nseg * 4));
    hipStream_t st = g->stream;
    HIPCHK(g, hipMemcpyAsync(d_plans, plans.data(), plans.size() * sizeof(lep5::SegPlan5), hipMemcpyHostToDevice, st));
    HIPCHK(g, hipMemcpyAsync(d_segs, segs.data(), segs.size() * sizeof(SegDev), hipMemcpyHostToDevice, st));
    HIPCHK(g, hipMemcpyAsync(d_arena, h_arena.data(), h_arena.size(), hipMemcpyHostToDevice, st));
    HIPCHK(g, hipMemsetAsync(d_list, 0xA5, list_bytes, st));
    HIPCHK(g, hipMemsetAsync(d_recs, 0xEE, rec_bytes, st));
    HIPCHK(g, hipMemsetAsync(d_out, guard & 255, arena_bytes ? arena_bytes : 16, st));
    HIPCHK(g, hipMemsetAsync(d_len, 0x7f, (size_t)nseg * 4, st));
    HIPCHK(g, hipMemsetAsync(d_status, 0x7f, (size_t)nseg * 4, st));
    // part p's bins of every segment (all of them where the form has no parts)
    auto send_part = [&](int p) -> int {
        if (p == parts) return 0;
        if (!in_parts || parts == 1) { HIPCHK(g, hipMemcpyAsync(d_list, h_bins.data(), (size_t)total * 2, hipMemcpyHostToDevice, st)); return 0; }
        for (int s = 0; s < nseg; ++s) {
            const uint32_t b0 = part_first[(size_t)s * parts + p], b1 = p + 1 < parts ? part_first[(size_t)s * parts + p + 1] : nbins[s];
            const uint64_t at = plans[(size_t)s].bins_off + b0;
            if (b1 > b0) HIPCHK(g, hipMemcpyAsync(d_list + at, h_bins.data() + at, (size_t)(b1 - b0) * 2, hipMemcpyHostToDevice, st));
        }
        if (p + 1 == parts) HIPCHK(g, hipMemcpyAsync(d_plans, plans_last.data(), plans_last.size() * sizeof(lep5::SegPlan5), hipMemcpyHostToDevice, st));
        return 0;
    };
    if (int rc = launch_enc5_writer(W, d_plans, d_list, d_segs, nseg, d_recs, d_arena, d_out, d_len, d_status, d_nb, st, send_part)) return rc;
    HIPCHK(g, hipGetLastError());
    HIPCHK(g, hipMemcpyAsync(arena_out, d_out, arena_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(g, hipMemcpyAsync(stream_len, d_len, (size_t)nseg * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(g, hipMemcpyAsync(status, d_status, (size_t)nseg * 4, hipMemcpyDeviceToHost, st));
    if (wchunks && W.records) HIPCHK(g, hipMemcpyAsync(wchunks, d_recs, rec_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(g, hipStreamSynchronize(st));
    return 0;
}

// tests: the stitched writer's records of the most recent split-phase launch, a copy out of W_ENC5_WCHUNKS in the caller's segment order
int lep_gpu_debug_wchunks(lep_gpu* g, void* out, size_t cap_records, int* nseg, int* parts, int* chunks) {
    if (!g) return 0;
    const int K = g->wchunks_parts * g->wchunks_per_part, n = (int)g->wchunks_slots.size();
    if (nseg) *nseg = K ? n : 0;
    if (parts) *parts = g->wchunks_parts;
    if (chunks) *chunks = g->wchunks_per_part;
    const Workspace& w = g->ws[lep_gpu::W_ENC5_WCHUNKS];
    if (!K || !out || cap_records < (size_t)n * K || !w.p || w.cap < (size_t)n * K * sizeof(lep5::WChunk5)) return K;
    if (hipSetDevice(g->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return 0;
    std::vector<lep5::WChunk5> recs((size_t)n * K);
    if (hipMemcpy(recs.data(), w.p, recs.size() * sizeof(lep5::WChunk5), hipMemcpyDeviceToHost) != hipSuccess) return 0;
    for (int i = 0; i < n; ++i)   // launch order -> the caller's
        memcpy((char*)out + (size_t)g->wchunks_slots[(size_t)i] * K * sizeof(lep5::WChunk5), &recs[(size_t)i * K], (size_t)K * sizeof(lep5::WChunk5));
    return K;
}

// profiling builds (-DLEP_PROF) only: per-phase shader-clock totals folded over the segments of the last decoder launch
int lep_gpu_debug_prof(lep_gpu* g, uint64_t* out /* [64][32] */) {
#ifdef LEP_PROF
    std::vector<unsigned long long> h(8192 * 32);   // fold the per-wave accumulators into the 64 x 32 report
    HIPCHK(g, hipMemcpyFromSymbol(h.data(), HIP_SYMBOL(g_prof4), sizeof(unsigned long long) * 8192 * 32));
    memset(out, 0, sizeof(uint64_t) * 64 * 32);
    for (int s = 0; s < 8192; ++s)
        for (int i = 0; i < 32; ++i) out[(s & 63) * 32 + i] += h[(size_t)s * 32 + i];
    return 0;
#else
    (void)g; (void)out;
    return LEP_GPU_ERROR;
#endif
}

// give back what the object caches between launches (models, neighbour rings, the split-phase encoder's scratch): all of it
// is re-acquired by the next launch that needs it.  Waits for the device first.
int lep_gpu_trim(lep_gpu* g) {
    // (a trim takes the models and rings of BOTH arena sets: refused while either has a decode session)
    for (int k = 0; k < 2; ++k)
        if (g->rows[k].open) { g->err = "lep_gpu_trim / lep_gpu_release_memory: arena set " + std::to_string(k) + " belongs to a decode session until lep_gpu_decode_rows_end"; return LEP_ASSERTION_FAILURE; }
    HIPCHK(g, hipSetDevice(g->device));
    HIPCHK(g, hipDeviceSynchronize());
    for (int w = 0; w < lep_gpu::W_TRIMMED; ++w) dev_release(g, g->ws[w]);
    return 0;
}
// ... and hand them to the driver (the pool too): for a process that wants the device's memory for something else
int lep_gpu_release_memory(lep_gpu* g) {
    if (int rc = lep_gpu_trim(g)) return rc;
    vmm_drain_pool(g);
    return 0;
}
int lep_gpu_malloc(lep_gpu* g, size_t bytes, void** dptr) {
    HIPCHK(g, hipSetDevice(g->device));
    if (hipMalloc(dptr, bytes ? bytes : 16) != hipSuccess) {   // (no room: the caches first, pool included, then the batch calls' staging)
        (void)hipGetLastError();
        if (int rc = lep_gpu_release_memory(g)) return rc;
        if (hipMalloc(dptr, bytes ? bytes : 16) != hipSuccess) {
            (void)hipGetLastError();
            lep_batch_release();
            HIPCHK(g, hipMalloc(dptr, bytes ? bytes : 16));
        }
    }
    return 0;
}
int lep_gpu_free(lep_gpu* g, void* dptr) { HIPCHK(g, hipFree(dptr)); return 0; }
int lep_gpu_memcpy_h2d(lep_gpu* g, void* dst, const void* src, size_t bytes) { HIPCHK(g, hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice)); return 0; }
int lep_gpu_memcpy_d2h(lep_gpu* g, void* dst, const void* src, size_t bytes) { HIPCHK(g, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost)); return 0; }
int lep_gpu_memcpy_d2d(lep_gpu* g, void* dst, const void* src, size_t bytes) { HIPCHK(g, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToDevice)); return 0; }
int lep_gpu_memset(lep_gpu* g, void* dst, int value, size_t bytes) { HIPCHK(g, hipMemset(dst, value, bytes)); return 0; }

// ---- host-buffer variants: stage frames through HBM, run the device path, fetch results --------------
static int stage_images(lep_gpu* g, const lep_image_desc* images, int nimg, std::vector<lep_image_desc>* dev, bool upload) {
    size_t total = 0;
    for (int i = 0; i < nimg; ++i)
        for (int c = 0; c < images[i].ncomp && c < 3; ++c) total += (size_t)images[i].width_blocks[c] * images[i].height_blocks[c] * 128;
    if (int rc = ensure(g, g->ws[lep_gpu::W_BLOCKS], total + 256)) return rc;
    char* const d_blocks = g->ws[lep_gpu::W_BLOCKS].at<char>(0);
    dev->assign(images, images + nimg);
    size_t off = 0;
    for (int i = 0; i < nimg; ++i)
        for (int c = 0; c < images[i].ncomp && c < 3; ++c) {
            size_t bytes = (size_t)images[i].width_blocks[c] * images[i].height_blocks[c] * 128;
            (*dev)[i].blocks[c] = (int16_t*)(d_blocks + off);
            if (upload) HIPCHK(g, hipMemcpyAsync(d_blocks + off, images[i].blocks[c], bytes, hipMemcpyHostToDevice, g->stream));
            else HIPCHK(g, hipMemsetAsync(d_blocks + off, 0, bytes, g->stream));
            off += bytes;
        }
    return 0;
}

int lep_gpu_encode_host(lep_gpu* g, const lep_image_desc* images, int nimg, const lep_segment* segs, int nseg, lep_bytes* out,
                        int32_t* status) {
    if (!g) return LEP_GPU_ERROR;
    HIPCHK(g, hipSetDevice(g->device));
    std::vector<lep_image_desc> dev;
    if (int rc = stage_images(g, images, nimg, &dev, true)) return rc;
    std::vector<uint64_t> offs(nseg + 1, 0);
    for (int s = 0; s < nseg; ++s) offs[s + 1] = offs[s] + out[s].cap;
    if (int rc = ensure(g, g->ws[lep_gpu::W_STREAMS], offs[nseg] + 16)) return rc;
    if (int rc = ensure(g, g->ws[lep_gpu::W_LENS], (size_t)nseg * 8 + 16)) return rc;
    uint8_t* const d_streams = g->ws[lep_gpu::W_STREAMS].at<uint8_t>(0);
    uint32_t* d_len = g->ws[lep_gpu::W_LENS].at<uint32_t>(0);
    int32_t* d_status = (int32_t*)(d_len + nseg);
    int rc = launch<false>(g, dev.data(), nimg, segs, nseg, d_streams, offs.data(), d_len, d_status, g->stream);
    if (rc) return rc;
    std::vector<uint32_t> lens(nseg);
    std::vector<int32_t> st(nseg);
    HIPCHK(g, hipMemcpyAsync(lens.data(), d_len, nseg * 4, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(g, hipMemcpyAsync(st.data(), d_status, nseg * 4, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(g, hipStreamSynchronize(g->stream));
    int worst = 0;
    for (int s = 0; s < nseg; ++s) {
        if (status) status[s] = st[s];
        if (st[s] && !worst) worst = st[s];
        out[s].len = st[s] ? 0 : lens[s];
        if (!st[s] && lens[s]) HIPCHK(g, hipMemcpyAsync(out[s].data, d_streams + offs[s], lens[s], hipMemcpyDeviceToHost, g->stream));
    }
    HIPCHK(g, hipStreamSynchronize(g->stream));
    return worst;
}

int lep_gpu_decode_host(lep_gpu* g, const lep_image_desc* images, int nimg, const lep_segment* segs, int nseg,
                        const lep_bytes* in, int32_t* status) {
    if (!g) return LEP_GPU_ERROR;
    HIPCHK(g, hipSetDevice(g->device));
    std::vector<lep_image_desc> dev;
    if (int rc = stage_images(g, images, nimg, &dev, false)) return rc;
    std::vector<uint64_t> offs(nseg + 1, 0);
    std::vector<uint32_t> lens(nseg);
    for (int s = 0; s < nseg; ++s) { offs[s + 1] = offs[s] + in[s].len; lens[s] = (uint32_t)in[s].len; }
    if (int rc = ensure(g, g->ws[lep_gpu::W_STREAMS], offs[nseg] + 16)) return rc;
    if (int rc = ensure(g, g->ws[lep_gpu::W_LENS], (size_t)nseg * 8 + 16)) return rc;
    uint8_t* const d_streams = g->ws[lep_gpu::W_STREAMS].at<uint8_t>(0);
    uint32_t* d_len = g->ws[lep_gpu::W_LENS].at<uint32_t>(0);
    int32_t* d_status = (int32_t*)(d_len + nseg);
    for (int s = 0; s < nseg; ++s)
        if (in[s].len) HIPCHK(g, hipMemcpyAsync(d_streams + offs[s], in[s].data, in[s].len, hipMemcpyHostToDevice, g->stream));
    HIPCHK(g, hipMemcpyAsync(d_len, lens.data(), nseg * 4, hipMemcpyHostToDevice, g->stream));
    HIPCHK(g, hipStreamSynchronize(g->stream));
    int rc = launch<true>(g, dev.data(), nimg, segs, nseg, d_streams, offs.data(), d_len, d_status, g->stream);
    if (rc) return rc;
    std::vector<int32_t> st(nseg);
    HIPCHK(g, hipMemcpyAsync(st.data(), d_status, nseg * 4, hipMemcpyDeviceToHost, g->stream));
    for (int i = 0; i < nimg; ++i)
        for (int c = 0; c < images[i].ncomp && c < 3; ++c) {
            size_t bytes = (size_t)images[i].width_blocks[c] * images[i].height_blocks[c] * 128;
            HIPCHK(g, hipMemcpyAsync(images[i].blocks[c], dev[i].blocks[c], bytes, hipMemcpyDeviceToHost, g->stream));
        }
    HIPCHK(g, hipStreamSynchronize(g->stream));
    int worst = 0;
    for (int s = 0; s < nseg; ++s) {
        if (status) status[s] = st[s];
        if (st[s] && !worst) worst = st[s];
    }
    return worst;
}

}  // extern "C"

// a refusal made outside this file in the object's name (lep_planes.cc; declared in lep_handles.h): the text lep_gpu_last_error returns
namespace lep {
int gpu_refuse(lep_gpu* g, int code, const std::string& what) {
    if (g) g->err = what;
    return code;
}
}  // namespace lep
