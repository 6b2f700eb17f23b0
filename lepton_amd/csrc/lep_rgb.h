// lep_rgb.h -- lep_gpu_rgb_device's kernel: 8-bit sample planes (lep_samples.h makes them) turned into pixels, interleaved R,G,B or
// one byte per pixel for a one-component image, cropped to the image's size: chroma upsampling and colour conversion as libjpeg's
// default full-scale path does them (fancy upsampling, no merged upsampling, jdcolor's table arithmetic).
//
// The definition (tests/rgb_ref.py restates it in numpy with 64-bit integers; tests/test_rgb_reference.py holds that against libjpeg).
//   Geometry.  Image W x H, hmax = max h_samp, vmax = max v_samp.  Component c: dw = ceil(W * h_c / hmax), dh = ceil(H * v_c / vmax);
//   only the top-left dw x dh samples of its plane are used, x[r][k]; whatever else the block grid holds is ignored.  fh = hmax / h_c,
//   fv = vmax / v_c, both integral or the image is refused.  A one-component image has fh = fv = 1 whatever its factors say.
//   Upsampling.  Neighbours out of range are the edge sample itself: up(r) = x[max(r-1, 0)], dn(r) = x[min(r+1, dh-1)], columns alike
//   with dw.  Division is an arithmetic right shift.  The result is cropped to W x H.
//     (fh, fv) = (1, 1)          out = x
//     (2, 1), dw > 2             out[y][2k]   = (3 x[y][k] + x[y][k-1] + 1) >> 2
//                                out[y][2k+1] = (3 x[y][k] + x[y][k+1] + 2) >> 2
//     (1, 2), any width          out[2r][k]   = (3 x[r][k] + up(r)[k] + 1) >> 2
//                                out[2r+1][k] = (3 x[r][k] + dn(r)[k] + 2) >> 2
//     (2, 2), dw > 2             s[2r][k] = 3 x[r][k] + up(r)[k],  s[2r+1][k] = 3 x[r][k] + dn(r)[k]   (not rounded)
//                                out[y][2k]   = (3 s[y][k] + s[y][k-1] + 8) >> 4
//                                out[y][2k+1] = (3 s[y][k] + s[y][k+1] + 7) >> 4
//     (2, 1) or (2, 2) with dw <= 2, and every other integral pair (3, 4, (2, 4), (4, 2), ...): replication, out[y][x] = x[y / fv][x / fh]
//   Colour.  FIX(f) = (int)(f * 65536 + 0.5), cb' = Cb - 128, cr' = Cr - 128:
//     R = clamp(Y + ((FIX(1.40200) cr' + 32768) >> 16))
//     B = clamp(Y + ((FIX(1.77200) cb' + 32768) >> 16))
//     G = clamp(Y + ((-FIX(0.34414) cb' + 32768 - FIX(0.71414) cr') >> 16))        clamp to 0..255; every product fits in 32 bits
//   An image whose components are R, G, B as they are (convert = 0) is upsampled all the same and not converted.
//
// The kernel.  Work is cut into wavefront units; a table of per-image records (RgbRec) and the running unit counts (first[]) say which
// image, output row and stretch of that row a unit is.  A unit is 256 pixels of one output row, four per lane.  A lane fetches, per
// component, the four samples under its pixels (no horizontal upsampling: x0 .. x0+3) or the two under them and one on either side
// (2:1: x0/2 - 1 .. x0/2 + 2), from one source row or from the two a vertical 2:1 takes -- as one aligned dword, as two aligned dwords
// shifted, or, at the row's ends and in rows that do not start on a dword, byte by byte with the index clamped into the row, which IS
// the edge rule.  It stores its 12 bytes as three dwords -- a wavefront 768 consecutive bytes -- or byte by byte where the destination is
// no multiple of 4 or the row ends inside its four pixels.  No load reaches beyond sample dw - 1 of a row, no store beyond the row's
// last pixel.  Rows of a vertically subsampled component are read twice, by the two output rows they feed.
// The lanes' work is plain C++ that tests/emu/rgb_emu.cc steps lane by lane (lep_wave.h); the __global__ entry is in lep_gpu.hip.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "lep_samples.h"
#include "lep_wave.h"

namespace leprgb {

constexpr int kLanePixels = 4;                  // pixels of a lane
constexpr int kUnitPixels = 64 * kLanePixels;   // ... of a wavefront unit
constexpr int kWavesPerGroup = 4;               // wavefronts per workgroup: each has a unit of its own and never waits for another

constexpr int32_t kFixCrR = 91881, kFixCbB = 116130, kFixCbG = 22554, kFixCrG = 46802;   // FIX(1.40200), FIX(1.77200), FIX(0.34414), FIX(0.71414)

enum Mode : uint8_t { kCopy = 0, kTriangleV = 1, kTriangleH = 2, kTriangleHV = 3, kReplicate = 4 };

// One image of the launch.  Uploaded as it stands; first[] (uint32, images + 1 entries: the units in front of each image) follows the records.
struct alignas(16) RgbRec {
    const uint8_t* plane[3];    // sample (0, 0) of each component's plane
    uint8_t* rgb;               // pixel (0, 0) of the output
    int32_t pitch[3];           // bytes from one sample row to the next
    int32_t rgb_pitch;          // ... from one pixel row to the next
    int32_t dw[3], dh[3];       // the samples of each plane that are used
    int32_t width;              // pixels in a row
    int32_t y_first;            // rows [y_first, y_first + rows) are written
    int32_t units_per_row;      // (width + 255) / 256
    int32_t ncomp;              // 1 or 3
    int32_t convert;            // 1: the components are Y, Cb, Cr; 0: they are what is stored
    uint8_t fh[3], fv[3], mode[3];
    uint8_t pad[11];
};
static_assert(sizeof(RgbRec) == 112 && offsetof(RgbRec, pitch) == 32 && offsetof(RgbRec, fh) == 92, "RgbRec is uploaded as bytes");

#if defined(__HIPCC__)
#define LEP_RGB_DEV __device__ __forceinline__
#else
#define LEP_RGB_DEV inline
#endif

// samples k .. k + 3 of a row of dw samples, a byte each, the lowest first; an index outside the row is moved to the row's nearer end
LEP_RGB_DEV uint32_t load4(const uint8_t* row, int dw, int k) {
    if (((uintptr_t)row & 3u) == 0 && k >= 0) {
        const int a = k & ~3, shift = (k & 3) * 8;
        if (shift == 0 && a + 4 <= dw) return lepwave::gld(reinterpret_cast<const uint32_t*>(row + a));
        if (a + 8 <= dw) {
            const uint64_t lo = lepwave::gld(reinterpret_cast<const uint32_t*>(row + a)), hi = lepwave::gld(reinterpret_cast<const uint32_t*>(row + a + 4));
            return (uint32_t)((lo | (hi << 32)) >> shift);
        }
    }
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int at = k + j < 0 ? 0 : k + j > dw - 1 ? dw - 1 : k + j;
        v |= (uint32_t)lepwave::gld(row + at) << (8 * j);
    }
    return v;
}
// samples (x + j) / fh, j = 0 .. 3, likewise
LEP_RGB_DEV uint32_t load4_replicated(const uint8_t* row, int dw, int x, int fh) {
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = (x + j) / fh, at = k > dw - 1 ? dw - 1 : k;
        v |= (uint32_t)lepwave::gld(row + at) << (8 * j);
    }
    return v;
}

LEP_RGB_DEV int32_t byte_of(uint32_t v, int j) { return (int32_t)((v >> (8 * j)) & 255u); }

// component c under pixels x0 .. x0 + 3 of output row y, upsampled
LEP_RGB_DEV void component4(const RgbRec& r, int c, int y, int x0, int32_t* out) {
    const uint8_t* const plane = r.plane[c];
    const size_t pitch = (size_t)r.pitch[c];
    const int dw = r.dw[c], dh = r.dh[c], mode = r.mode[c];
    if (mode == kCopy) {
        const uint32_t v = load4(plane + (size_t)y * pitch, dw, x0);
#pragma unroll
        for (int j = 0; j < 4; ++j) out[j] = byte_of(v, j);
        return;
    }
    if (mode == kReplicate) {
        const uint32_t v = load4_replicated(plane + (size_t)(y / r.fv[c]) * pitch, dw, x0, r.fh[c]);
#pragma unroll
        for (int j = 0; j < 4; ++j) out[j] = byte_of(v, j);
        return;
    }
    if (mode == kTriangleH) {
        const uint32_t v = load4(plane + (size_t)y * pitch, dw, (x0 >> 1) - 1);
        const int32_t s0 = byte_of(v, 0), s1 = byte_of(v, 1), s2 = byte_of(v, 2), s3 = byte_of(v, 3);
        out[0] = (3 * s1 + s0 + 1) >> 2; out[1] = (3 * s1 + s2 + 2) >> 2;
        out[2] = (3 * s2 + s1 + 1) >> 2; out[3] = (3 * s2 + s3 + 2) >> 2;
        return;
    }
    // a vertical 2:1: the row under y and the one above (even y) or below it (odd y)
    const int odd = y & 1, near = y >> 1;
    const int far = odd ? (near + 1 > dh - 1 ? dh - 1 : near + 1) : (near - 1 < 0 ? 0 : near - 1);
    const int k = mode == kTriangleV ? x0 : (x0 >> 1) - 1;
    const uint32_t vn = load4(plane + (size_t)near * pitch, dw, k), vf = load4(plane + (size_t)far * pitch, dw, k);
    int32_t s[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = 3 * byte_of(vn, j) + byte_of(vf, j);
    if (mode == kTriangleV) {
#pragma unroll
        for (int j = 0; j < 4; ++j) out[j] = (s[j] + 1 + odd) >> 2;
        return;
    }
    out[0] = (3 * s[1] + s[0] + 8) >> 4; out[1] = (3 * s[1] + s[2] + 7) >> 4;
    out[2] = (3 * s[2] + s[1] + 8) >> 4; out[3] = (3 * s[2] + s[3] + 7) >> 4;
}

LEP_RGB_DEV uint32_t clamp255(int32_t v) { return (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v); }

// a lane's pixels x0 .. x0 + 3 of output row y (x0 a multiple of 4)
LEP_RGB_DEV void lane_rgb(const RgbRec& r, int y, int x0) {
    if (x0 >= r.width) return;
    const int left = r.width - x0, n = left < kLanePixels ? left : kLanePixels;
    int32_t a[4];
    component4(r, 0, y, x0, a);
    if (r.ncomp == 1) {
        uint8_t* dst = r.rgb + (size_t)y * (size_t)r.rgb_pitch + (size_t)x0;
        if (n == 4 && ((uintptr_t)dst & 3u) == 0) {
            lepwave::gst(reinterpret_cast<uint32_t*>(dst), (uint32_t)a[0] | (uint32_t)a[1] << 8 | (uint32_t)a[2] << 16 | (uint32_t)a[3] << 24);
        } else {
            for (int j = 0; j < n; ++j) lepwave::gst(dst + j, (uint8_t)a[j]);
        }
        return;
    }
    int32_t b[4], c[4];
    component4(r, 1, y, x0, b);
    component4(r, 2, y, x0, c);
    uint32_t px[4];   // R | G << 8 | B << 16
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (r.convert) {
            const int32_t cb = b[j] - 128, cr = c[j] - 128;
            const uint32_t R = clamp255(a[j] + ((kFixCrR * cr + 32768) >> 16));
            const uint32_t G = clamp255(a[j] + ((-kFixCbG * cb + 32768 - kFixCrG * cr) >> 16));
            const uint32_t B = clamp255(a[j] + ((kFixCbB * cb + 32768) >> 16));
            px[j] = R | G << 8 | B << 16;
        } else {
            px[j] = (uint32_t)a[j] | (uint32_t)b[j] << 8 | (uint32_t)c[j] << 16;
        }
    }
    uint8_t* dst = r.rgb + (size_t)y * (size_t)r.rgb_pitch + (size_t)x0 * 3;
    if (n == 4 && ((uintptr_t)dst & 3u) == 0) {
        uint32_t* d = reinterpret_cast<uint32_t*>(dst);
        lepwave::gst(d, px[0] | px[1] << 24);
        lepwave::gst(d + 1, px[1] >> 8 | px[2] << 16);
        lepwave::gst(d + 2, px[2] >> 16 | px[3] << 8);
    } else {   // an output or a pitch that is no multiple of 4, or the row's last pixels: byte by byte
        for (int j = 0; j < n; ++j) {
            lepwave::gst(dst + 3 * j, (uint8_t)px[j]);
            lepwave::gst(dst + 3 * j + 1, (uint8_t)(px[j] >> 8));
            lepwave::gst(dst + 3 * j + 2, (uint8_t)(px[j] >> 16));
        }
    }
}

// A wavefront's unit (unit < first[nimg], wave-uniform): 256 pixels of one output row of one image.
LEP_RGB_DEV void wave_rgb(const RgbRec* recs, const uint32_t* first, int nimg, uint32_t unit) {
    const int i = lepsamples::plane_of(first, nimg, unit);
    const RgbRec& r = recs[i];
    const uint32_t local = unit - first[i];
    const int y = r.y_first + (int)(local / (uint32_t)r.units_per_row);
    const int x_unit = (int)(local % (uint32_t)r.units_per_row) * kUnitPixels;
    LANES(l) { lane_rgb(r, y, x_unit + l * kLanePixels); }
}

// Host side, shared by lep_gpu_rgb_device and the emulation: one image's record.  Returns the image's units, -1 where a sampling factor
// is not 1 .. 4 or does not divide the largest, the size is not 1 .. 65535 or there are not one or three components.  Pointers, pitches
// and the row range are taken as they are: the caller holds them against dw / dh / width, which are filled in whatever they are.
inline int64_t fill_image(RgbRec* r, int width, int height, int ncomp, const int32_t* h_samp, const int32_t* v_samp, int convert,
                          const uint8_t* const* planes, const int32_t* pitch, uint8_t* rgb, int rgb_pitch, int y_first, int y_end) {
    *r = RgbRec();
    if ((ncomp != 1 && ncomp != 3) || width < 1 || height < 1 || width > 65535 || height > 65535) return -1;
    int hmax = 1, vmax = 1;
    for (int c = 0; c < ncomp; ++c) {
        if (h_samp[c] < 1 || h_samp[c] > 4 || v_samp[c] < 1 || v_samp[c] > 4) return -1;
        hmax = h_samp[c] > hmax ? h_samp[c] : hmax;
        vmax = v_samp[c] > vmax ? v_samp[c] : vmax;
    }
    for (int c = 0; c < ncomp; ++c) {
        const int hs = ncomp == 1 ? hmax : h_samp[c], vs = ncomp == 1 ? vmax : v_samp[c];
        if (hmax % hs || vmax % vs) return -1;
        const int fh = hmax / hs, fv = vmax / vs;
        r->plane[c] = planes[c]; r->pitch[c] = pitch[c];
        r->dw[c] = (width * hs + hmax - 1) / hmax;
        r->dh[c] = (height * vs + vmax - 1) / vmax;
        r->fh[c] = (uint8_t)fh; r->fv[c] = (uint8_t)fv;
        r->mode[c] = fh == 1 && fv == 1 ? kCopy : fh == 1 && fv == 2 ? kTriangleV : fh == 2 && fv == 1 && r->dw[c] > 2 ? kTriangleH
                     : fh == 2 && fv == 2 && r->dw[c] > 2 ? kTriangleHV : kReplicate;
    }
    r->rgb = rgb; r->rgb_pitch = rgb_pitch;
    r->width = width; r->y_first = y_first; r->ncomp = ncomp; r->convert = convert ? 1 : 0;
    r->units_per_row = (width + kUnitPixels - 1) / kUnitPixels;
    return y_end > y_first ? (int64_t)(y_end - y_first) * r->units_per_row : 0;
}

}  // namespace leprgb
