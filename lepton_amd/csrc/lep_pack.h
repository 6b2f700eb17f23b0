// lep_pack.h -- lep_gpu_pack_device's two kernels: byte runs that lie apart in device memory (the scan bytes a band of MCU rows added to
// every segment's slot) moved back to back, so that they cross PCIe in one copy instead of one per run.
//   lep_pack_offsets_kernel   one workgroup of 1024 lanes: exclusive prefix sum of up to 16384 lengths (16 per lane, a wave scan,
//                             the sixteen wave totals through LDS); dst_off[n] = the total
//   lep_pack_copy_kernel      one wavefront per run: byte head up to the destination's next dword boundary, then whole dwords stored
//                             to the aligned destination -- each made of the two aligned source dwords it straddles --, byte tail.
//                             Every load is an aligned dword that holds at least one byte of the run (or a single byte of it):
//                             nothing in front of or behind the run's first / last dword is touched.
// A total beyond dst_cap copies nothing: every wavefront reads dst_off[n] and leaves.
// lep_gpu_pack_window_device is the same pair with a window per run (skip, take: host values): the offsets kernel clips every
// device-resident length to its window (window_len) -- that is what it sums and what it leaves for the copy kernel --, and the copy
// starts skip bytes into the run, at whatever alignment that leaves: copy_run's contract, held for the window's bytes.
#pragma once
#include <stdint.h>

namespace leppack {

constexpr int kMaxRuns = 16384;
constexpr int kScanLanes = 1024;
constexpr int kPerLane = kMaxRuns / kScanLanes;

#if defined(__HIPCC__)
#define LEP_PACK_DEV __device__ __forceinline__
#else
#define LEP_PACK_DEV inline
#endif

// One lane's share of a run's copy (lane 0 .. 63 of the run's wavefront).  Plain C++: tests/emu/pack_copy_emu.cc steps it lane by lane.
LEP_PACK_DEV void copy_run(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, uint32_t len, uint32_t lane) {
    const uint32_t to_boundary = (uint32_t)(-(uintptr_t)dst & 3u);
    const uint32_t head = len < to_boundary ? len : to_boundary;
    if (lane < head) dst[lane] = src[lane];
    const uint32_t nd = (len - head) >> 2, tail = (len - head) & 3u;
    const uint8_t* s = src + head;
    uint32_t* d32 = reinterpret_cast<uint32_t*>(dst + head);
    const uint32_t sh = (uint32_t)((uintptr_t)s & 3u);
    const uint32_t* s32 = reinterpret_cast<const uint32_t*>(s - sh);
    if (sh == 0) {
        for (uint32_t i = lane; i < nd; i += 64) d32[i] = s32[i];
    } else {
        const uint32_t down = sh * 8, up = 32 - down;
        for (uint32_t i = lane; i < nd; i += 64) d32[i] = (s32[i] >> down) | (s32[i + 1] << up);
    }
    if (lane < tail) dst[head + nd * 4 + lane] = s[nd * 4 + lane];
}

// What of a run of len bytes lies in its window: the bytes [skip, min(len, skip + take)), none when the run ends in front of it.
LEP_PACK_DEV uint32_t window_len(uint32_t len, uint32_t skip, uint32_t take) {
    if (len <= skip) return 0u;
    const uint32_t rest = len - skip;
    return rest < take ? rest : take;
}

#if defined(__HIPCC__)
// len_of(i): the length run i contributes (a plain load, or the clipped length of a windowed run)
template <class LenOf>
__device__ __forceinline__ void offsets(LenOf len_of, int n, uint64_t* __restrict__ dst_off) {
    __shared__ uint64_t wave_total[kScanLanes / 64];
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const int first = t * kPerLane;
    uint32_t mine[kPerLane];
    uint64_t sum = 0;
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) {
        mine[k] = first + k < n ? len_of(first + k) : 0u;
        sum += mine[k];
    }
    uint64_t incl = sum;   // inclusive scan over the wave's lanes
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    uint64_t base = 0;
    for (int w = 0; w < wave; ++w) base += wave_total[w];
    uint64_t at = base + incl - sum;
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) {
        if (first + k < n) dst_off[first + k] = at;
        at += mine[k];
        if (first + k == n - 1) dst_off[n] = at;
    }
}
#endif

}  // namespace leppack
