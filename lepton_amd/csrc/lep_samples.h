// lep_samples.h -- lep_gpu_samples_device's kernels: the coefficient frames the coders keep in device memory turned into 8-bit sample
// planes, one plane per component at the component's own resolution (no upsampling, no colour conversion), at full scale and at 1/8.
//
// The arithmetic (the definition; tests/samples_ref.py restates it in 64-bit integers).  For a block with coefficients c[0..63] and
// quantisation table q[0..63], d[k] = c[k] * q[k], laid out as an 8x8 raster.
//   Scale 1: the two-pass integer transform of libjpeg's jidctint ("islow") with 13-bit constants, columns first, then rows.  With
//   the inputs i0..i7 of one column or row:
//       z1 = (i2+i6)*4433;  t2 = z1 - i6*15137;  t3 = z1 + i2*6270
//       t0 = (i0+i4)<<13;   t1 = (i0-i4)<<13
//       t10 = t0+t3; t13 = t0-t3; t11 = t1+t2; t12 = t1-t2
//       a0 = i7; a1 = i5; a2 = i3; a3 = i1
//       z1 = a0+a3; z2 = a1+a2; z3 = a0+a2; z4 = a1+a3; z5 = (z3+z4)*9633
//       a0 *= 2446; a1 *= 16819; a2 *= 25172; a3 *= 12299
//       z1 *= -7373; z2 *= -20995; z3 = z3*-16069 + z5; z4 = z4*-3196 + z5
//       a0 += z1+z3; a1 += z2+z4; a2 += z2+z3; a3 += z1+z4
//       out[0..7] = t10+a3, t11+a2, t12+a1, t13+a0, t13-a0, t12-a1, t11-a2, t10-a3
//   every output descaled as (x + (1 << (s-1))) >> s with an arithmetic shift, s = 11 behind the column pass and 18 behind the row
//   pass; the sample is clamp(result + 128, 0, 255).
//   Scale 8: one sample per block, clamp(((d[0] + 4) >> 3) + 128, 0, 255).
//   Domain: the result is exact integer arithmetic for frames in which every |d[k]| <= 32767 and every value between the passes is
//   <= 32767 in magnitude.  Each output of a pass is a linear form of its inputs whose absolute coefficients sum to at most 61214, so a
//   final sum fits in 32 bits for inputs up to 35079 in magnitude: inside the domain 32-bit arithmetic is exact even where a partial
//   sum wraps.  All sums are done in unsigned 32-bit.  Outside the domain the result is what these formulas give in wrapping 32-bit
//   arithmetic (libjpeg does not agree with itself out there: its SIMD path multiplies in 16 bits and saturates between the passes,
//   its one-sample path wraps through a table instead of clamping).
//
// The kernels.  Work is cut into wavefront units; a table of per-plane records (PlaneRec) and the running unit counts (first[]) say
// which plane, block row and group of blocks a unit is.
//   scale 1  a unit is eight horizontally adjacent blocks, 1 KB in a row of the frame: one 16-byte load per lane.  A lane dequantises
//            its eight coefficients (aligned order: lep_core.h kA2R) and scatters them in raster order into an LDS tile of 32-bit
//            values; the column pass runs with lane = (block, column), the row pass with lane = (row, block), so that the eight lanes
//            of one sample row store 8 bytes each into 64 consecutive bytes of the plane.  The tile is padded (tile_at): rows are 9
//            dwords apart, blocks 72, blocks 4..7 four more -- ds_read_b32 is served in groups of 32 lanes over 32 banks, and with this
//            layout the 32 lanes of a group read 32 different banks in both passes (unpadded, eight lanes would share each bank).
//   scale 8  a unit is 64 horizontally adjacent blocks; a lane takes one block's DC and stores one byte: 64 consecutive samples.
// Lanes whose block lies beyond the row's end neither load nor store.  The work is bound by memory: every coefficient is read once
// (scale 8: the 128-byte line of every block for its DC) and every sample written once.
// The lanes' work is plain C++ that tests/emu/samples_emu.cc steps lane by lane (lep_wave.h); the __global__ entries are in lep_gpu.hip.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "lep_wave.h"

namespace lepsamples {

constexpr int kDcAligned = 49;          // the DC's place in a block in aligned order
constexpr int kTileWords = 584;         // tile_at(7, 7, 7) + 1 = 579, rounded up
constexpr int kWavesPerGroup = 4;       // wavefronts per workgroup: each has a tile of its own and never waits for another

// raster index of aligned entry a: lep_core.h's kA2R again, 8-byte aligned so that a lane fetches its eight places with one load, and
// here so that the emulation needs this header and lep_wave.h alone
#ifdef __HIP_DEVICE_COMPILE__
#define LEP_SAMPLES_TABLE __constant__ static const
#else
#define LEP_SAMPLES_TABLE static const
#endif
alignas(8) LEP_SAMPLES_TABLE uint8_t kAlignedToRaster[64] = {
    9, 10, 17, 25, 18, 11, 12, 19, 26, 33, 41, 34, 27, 20, 13, 14, 21, 28, 35, 42, 49, 57, 50, 43, 36,
    29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63,
    0, 1, 2, 3, 4, 5, 6, 7, 8, 16, 24, 32, 40, 48, 56};

typedef int16_t Lane8 __attribute__((vector_size(16)));   // a lane's 16 bytes of a frame row / of the table (a vector type: one load)

// One plane of the launch.  Uploaded as it stands; first[] (uint32, planes + 1 entries: the units in front of each plane) follows the records.
struct alignas(16) PlaneRec {
    const int16_t* blocks;      // the component's frame: width_blocks x height_blocks blocks of 64 int16, aligned order, 16-byte aligned
    uint8_t* plane;             // sample (0, 0) of the plane
    int32_t width_blocks;
    int32_t pitch;              // bytes from one sample row to the next
    int32_t row_first;          // block rows [row_first, row_first + rows) are written
    int32_t units_per_row;      // (width_blocks + 7) / 8 at scale 1, (width_blocks + 63) / 64 at scale 8
    int32_t pad[4];
    uint16_t q[64];             // quantisation table in aligned order; 16-byte aligned: a lane loads eight entries at once
};
static_assert(sizeof(PlaneRec) == 176 && offsetof(PlaneRec, q) == 48, "PlaneRec is uploaded as bytes");

#if defined(__HIPCC__)
#define LEP_SAMPLES_DEV __device__ __forceinline__
#else
#define LEP_SAMPLES_DEV inline
#endif

// the plane of unit `unit`: the last p with first[p] <= unit (first[0] = 0, unit < first[n]); planes without units are stepped over
LEP_SAMPLES_DEV int plane_of(const uint32_t* first, int n, uint32_t unit) {
    int lo = 0, hi = n;   // first[lo] <= unit < first[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] <= unit) lo = mid; else hi = mid;
    }
    return lo;
}

LEP_SAMPLES_DEV int tile_at(int block, int row, int col) { return block * 72 + (block >> 2) * 4 + row * 9 + col; }

LEP_SAMPLES_DEV int32_t descale(uint32_t x, int s) { return (int32_t)(x + (1u << (s - 1))) >> s; }
LEP_SAMPLES_DEV uint32_t clamp_sample(int32_t v) { v += 128; return (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v); }

// one pass over eight values, not descaled (unsigned: sums may wrap, the domain's results do not depend on it)
LEP_SAMPLES_DEV void idct8(const uint32_t* i, uint32_t* out) {
    uint32_t z1 = (i[2] + i[6]) * 4433u;
    const uint32_t t2 = z1 - i[6] * 15137u, t3 = z1 + i[2] * 6270u;
    const uint32_t t0 = (i[0] + i[4]) << 13, t1 = (i[0] - i[4]) << 13;
    const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    uint32_t a0 = i[7], a1 = i[5], a2 = i[3], a3 = i[1];
    z1 = a0 + a3;
    uint32_t z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const uint32_t z5 = (z3 + z4) * 9633u;
    a0 *= 2446u; a1 *= 16819u; a2 *= 25172u; a3 *= 12299u;
    z1 *= (uint32_t)-7373; z2 *= (uint32_t)-20995; z3 = z3 * (uint32_t)-16069 + z5; z4 = z4 * (uint32_t)-3196 + z5;
    a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
    out[0] = t10 + a3; out[1] = t11 + a2; out[2] = t12 + a1; out[3] = t13 + a0;
    out[4] = t13 - a0; out[5] = t12 - a1; out[6] = t11 - a2; out[7] = t10 - a3;
}

// scale 1, first step: lane (block = lane / 8, eighth = lane % 8) loads aligned entries eighth * 8 .. + 7 of its block, multiplies them
// with the table and puts them at their raster places in the tile.  nb = blocks of this unit (1..8).
LEP_SAMPLES_DEV void load_scatter(const PlaneRec& r, int row, int unit_in_row, int nb, int lane, uint32_t* tile) {
    const int b = lane >> 3, e = lane & 7;
    if (b >= nb) return;
    const size_t block = (size_t)row * (size_t)r.width_blocks + (size_t)unit_in_row * 8 + (size_t)b;
    const Lane8 c = lepwave::gld(reinterpret_cast<const Lane8*>(r.blocks + block * 64) + e);
    const Lane8 q = lepwave::gld(reinterpret_cast<const Lane8*>(r.q) + e);
    uint64_t places;   // the eight raster places of this lane's entries, a byte each
    __builtin_memcpy(&places, kAlignedToRaster + e * 8, 8);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int at = (int)(places >> (8 * k)) & 63;
        tile[tile_at(b, at >> 3, at & 7)] = (uint32_t)(int32_t)c[k] * (uint32_t)(uint16_t)q[k];
    }
}

// second step: lane (block = lane / 8, column = lane % 8) transforms its column in place
LEP_SAMPLES_DEV void column_pass(int nb, int lane, uint32_t* tile) {
    const int b = lane >> 3, col = lane & 7;
    if (b >= nb) return;
    uint32_t in[8], out[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) in[k] = tile[tile_at(b, k, col)];
    idct8(in, out);
#pragma unroll
    for (int k = 0; k < 8; ++k) tile[tile_at(b, k, col)] = (uint32_t)descale(out[k], 11);
}

// third step: lane (row = lane / 8, block = lane % 8) transforms its row and stores its 8 samples
LEP_SAMPLES_DEV void row_pass_store(const PlaneRec& r, int row, int unit_in_row, int nb, int lane, const uint32_t* tile) {
    const int y = lane >> 3, b = lane & 7;
    if (b >= nb) return;
    uint32_t in[8], out[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) in[k] = tile[tile_at(b, y, k)];
    idct8(in, out);
    uint64_t bytes = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) bytes |= (uint64_t)clamp_sample(descale(out[k], 18)) << (8 * k);
    uint8_t* dst = r.plane + ((size_t)row * 8 + (size_t)y) * (size_t)r.pitch + ((size_t)unit_in_row * 8 + (size_t)b) * 8;
    if (((uintptr_t)dst & 7u) == 0) {
        lepwave::gst(reinterpret_cast<uint64_t*>(dst), bytes);
    } else {   // a plane or a pitch that is no multiple of 8: byte by byte
#pragma unroll
        for (int k = 0; k < 8; ++k) lepwave::gst(dst + k, (uint8_t)(bytes >> (8 * k)));
    }
}

// which block row and group of blocks unit `unit` is, and how many blocks of the row it holds (per: blocks per unit)
struct Unit { int plane, row, in_row, nb; };
LEP_SAMPLES_DEV Unit unit_at(const PlaneRec* recs, const uint32_t* first, int nplanes, uint32_t unit, int per) {
    Unit u;
    u.plane = plane_of(first, nplanes, unit);
    const PlaneRec& r = recs[u.plane];
    const uint32_t local = unit - first[u.plane];
    u.row = r.row_first + (int)(local / (uint32_t)r.units_per_row);
    u.in_row = (int)(local % (uint32_t)r.units_per_row);
    const int left = r.width_blocks - u.in_row * per;
    u.nb = left < per ? left : per;
    return u;
}

// A wavefront's unit at scale 1 (unit < first[nplanes], wave-uniform; tile: kTileWords of LDS that are this wavefront's alone).
LEP_SAMPLES_DEV void wave_samples(const PlaneRec* recs, const uint32_t* first, int nplanes, uint32_t unit, uint32_t* tile) {
    const Unit u = unit_at(recs, first, nplanes, unit, 8);
    const PlaneRec& r = recs[u.plane];
    LANES(l) { load_scatter(r, u.row, u.in_row, u.nb, l, tile); }
    LSYNC();
    LANES(l) { column_pass(u.nb, l, tile); }
    LSYNC();
    LANES(l) { row_pass_store(r, u.row, u.in_row, u.nb, l, tile); }
}

// A wavefront's unit at scale 8: 64 blocks of one block row, a sample each.
LEP_SAMPLES_DEV void wave_samples_dc(const PlaneRec* recs, const uint32_t* first, int nplanes, uint32_t unit) {
    const Unit u = unit_at(recs, first, nplanes, unit, 64);
    const PlaneRec& r = recs[u.plane];
    LANES(l) {
        if (l < u.nb) {
            const size_t x = (size_t)u.in_row * 64 + (size_t)l;
            const int16_t dc = lepwave::gld(r.blocks + ((size_t)u.row * (size_t)r.width_blocks + x) * 64 + kDcAligned);
            const uint32_t d = (uint32_t)(int32_t)dc * (uint32_t)r.q[kDcAligned];
            lepwave::gst(r.plane + (size_t)u.row * (size_t)r.pitch + x, (uint8_t)clamp_sample((int32_t)(d + 4u) >> 3));
        }
    }
}

// Host side, shared by lep_gpu_samples_device and the emulation: one plane's record (q_zigzag: lep_image_desc's table; block rows
// [row_first, row_end) are written).  Returns the plane's units.
static const uint8_t kZigzagToAligned[64] = {
    49, 50, 57, 58, 0, 51, 52, 1, 2, 59, 60, 3, 4, 5, 53, 54, 6, 7, 8, 9, 61, 62, 10, 11,
    12, 13, 14, 55, 56, 15, 16, 17, 18, 19, 20, 63, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32,
    33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47, 48};
inline uint64_t fill_plane(PlaneRec* r, const int16_t* blocks, uint8_t* plane, int width_blocks, int pitch, int row_first, int row_end,
                           const uint16_t* q_zigzag, int scale) {
    r->blocks = blocks; r->plane = plane;
    r->width_blocks = width_blocks; r->pitch = pitch; r->row_first = row_first;
    r->units_per_row = scale == 8 ? (width_blocks + 63) / 64 : (width_blocks + 7) / 8;
    r->pad[0] = r->pad[1] = r->pad[2] = r->pad[3] = 0;
    for (int z = 0; z < 64; ++z) r->q[kZigzagToAligned[z]] = q_zigzag[z];
    return (uint64_t)(row_end - row_first) * (uint64_t)r->units_per_row;
}

}  // namespace lepsamples
