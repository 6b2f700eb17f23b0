// lep_planes.cc -- lep_decompress_planes and lep_decompress_rgb: a .lep file to 8-bit sample planes (lep_samples.h) and on to pixels
// (lep_rgb.h).  A source of its own because these are the whole-file calls that drive the device through the lep_gpu_*_device entry
// points: lep_api.cc stays linkable with the host parsers alone.
#include "../../include/lepton_mi355x.h"

#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "jpeg_model.h"
#include "lep_container.h"
#include "lep_handles.h"

namespace {

// The front both calls share.  It is lep_decompress's: the same parse, the same decode launch on a zero-filled frame, the same exit
// codes.  The frame never leaves the device: lep_gpu_samples_device reads it where the decoder left it and writes the planes behind it.
struct Front {
    lep_gpu* g = nullptr;
    std::unique_ptr<lep_file> file;
    lep_image_desc d;
    void* dev = nullptr;            // one device allocation: frame | planes | streams | lengths | statuses
    uint8_t* d_planes0 = nullptr;
    size_t plane_bytes = 0;
    size_t plane_off[LEP_MAX_COMPONENTS] = {0, 0, 0};
    int32_t pitch[LEP_MAX_COMPONENTS] = {0, 0, 0}, plane_width[LEP_MAX_COMPONENTS] = {0, 0, 0}, plane_height[LEP_MAX_COMPONENTS] = {0, 0, 0};
    ~Front() { if (dev) lep_gpu_free(g, dev); }
    const lep::JpegFile& jpeg() const { return file->lf.jpeg; }

    int open(lep_gpu* gpu, const uint8_t* lepdata, size_t len) {
        g = gpu;
        lep_file* f = nullptr;
        if (int rc = lep_file_open_next(lepdata, len, nullptr, &f)) return rc;
        file.reset(f);
        lep_file_describe_into(f, nullptr, (size_t)-1, &d);   // geometry only: the frame is device memory
        return 0;
    }
    // the decode launch and the sample planes, left in device memory
    int planes(int scale) {
        lep_file* f = file.get();
        lep_segment segs[LEP_MAX_SEGMENTS];
        lep_bytes streams[LEP_MAX_SEGMENTS];
        const int n = lep_file_segments(f, segs, streams, 0);
        size_t frame_bytes = 0, stream_bytes = 0;
        for (int c = 0; c < d.ncomp; ++c) {
            frame_bytes += (size_t)d.width_blocks[c] * d.height_blocks[c] * 128;
            plane_width[c] = pitch[c] = d.width_blocks[c] * 8 / scale;
            plane_height[c] = d.height_blocks[c] * 8 / scale;
            plane_off[c] = plane_bytes;
            plane_bytes += ((size_t)pitch[c] * plane_height[c] + 15) & ~(size_t)15;
        }
        std::vector<uint64_t> offs((size_t)n + 1, 0);
        std::vector<uint32_t> lens((size_t)n, 0);
        for (int s = 0; s < n; ++s) { offs[s + 1] = offs[s] + streams[s].len; lens[s] = (uint32_t)streams[s].len; }
        stream_bytes = (offs[n] + 16 + 15) & ~(size_t)15;
        if (int rc = lep_gpu_malloc(g, frame_bytes + plane_bytes + stream_bytes + (size_t)n * 8 + 16, &dev)) return rc;
        uint8_t* const d_frame = (uint8_t*)dev;
        d_planes0 = d_frame + frame_bytes;
        uint8_t* const d_streams = d_planes0 + plane_bytes;
        uint32_t* const d_len = (uint32_t*)(d_streams + stream_bytes);
        int32_t* const d_status = (int32_t*)(d_len + n);
        if (int rc = lep_gpu_memset(g, d_frame, 0, frame_bytes)) return rc;
        size_t at = 0;
        for (int c = 0; c < d.ncomp; ++c) { d.blocks[c] = (int16_t*)(d_frame + at); at += (size_t)d.width_blocks[c] * d.height_blocks[c] * 128; }
        for (int s = 0; s < n; ++s)
            if (streams[s].len)
                if (int rc = lep_gpu_memcpy_h2d(g, d_streams + offs[s], streams[s].data, streams[s].len)) return rc;
        if (n)
            if (int rc = lep_gpu_memcpy_h2d(g, d_len, lens.data(), (size_t)n * 4)) return rc;
        if (int rc = lep_gpu_decode_device(g, &d, 1, segs, n, d_streams, offs.data(), d_len, d_status, nullptr)) return rc;
        std::vector<int32_t> st((size_t)n, 0);
        if (n)
            if (int rc = lep_gpu_memcpy_d2h(g, st.data(), d_status, (size_t)n * 4)) return rc;   // (waits for the decoder)
        for (int s = 0; s < n; ++s)
            if (st[s]) return st[s];
        uint8_t* d_plane[LEP_MAX_COMPONENTS] = {nullptr, nullptr, nullptr};
        for (int c = 0; c < d.ncomp; ++c) d_plane[c] = d_planes0 + plane_off[c];
        return lep_gpu_samples_device(g, &d, 1, scale, nullptr, nullptr, d_plane, pitch, nullptr);
    }
};

// libjpeg's rule for a three-component file (jdapimin.c, default_decompress_parms): are the components Y, Cb, Cr?  hdr: the marker
// segments after SOI.  The segments in front of the first scan are the ones libjpeg has seen when it decides.
bool components_are_ycbcr(const lep::JpegFile& jf) {
    const std::vector<uint8_t>& h = jf.hdr;
    bool jfif = false, adobe = false;
    int transform = 0;
    for (size_t at = 0; at + 4 <= h.size() && h[at] == 0xFF;) {
        const int marker = h[at + 1];
        const size_t seg = ((size_t)h[at + 2] << 8) | h[at + 3];
        if (seg < 2 || at + 2 + seg > h.size()) break;
        const uint8_t* body = h.data() + at + 4;
        const size_t n = seg - 2;
        if (marker == 0xE0 && n >= 14 && !memcmp(body, "JFIF\0", 5)) jfif = true;
        if (marker == 0xEE && n >= 12 && !memcmp(body, "Adobe", 5)) { adobe = true; transform = body[11]; }
        if (marker == 0xDA) break;
        at += 2 + seg;
    }
    if (jfif) return true;
    if (adobe) return transform != 0;
    return !(jf.comp[0].jid == 'R' && jf.comp[1].jid == 'G' && jf.comp[2].jid == 'B');
}

}  // namespace

extern "C" {

// .lep -> sample planes: the front, and the planes come down.
int lep_decompress_planes(lep_gpu* g, const uint8_t* lepdata, size_t len, int scale, lep_planes* out) {
    if (!g) return LEP_GPU_ERROR;
    if (!out || (scale != 1 && scale != 8)) return LEP_ASSERTION_FAILURE;
    memset(out, 0, sizeof *out);
    Front fr;
    if (int rc = fr.open(g, lepdata, len)) return rc;
    if (int rc = fr.planes(scale)) return rc;
    const lep::JpegFile& jf = fr.jpeg();
    uint8_t* host = (uint8_t*)malloc(fr.plane_bytes ? fr.plane_bytes : 1);
    if (!host) return LEP_OS_ERROR;
    if (int rc = lep_gpu_memcpy_d2h(g, host, fr.d_planes0, fr.plane_bytes)) { free(host); return rc; }
    out->width = jf.width; out->height = jf.height; out->ncomp = fr.d.ncomp; out->scale = scale;
    for (int c = 0; c < fr.d.ncomp; ++c) {
        out->h_samp[c] = jf.comp[c].hs; out->v_samp[c] = jf.comp[c].vs;
        out->plane_width[c] = fr.plane_width[c]; out->plane_height[c] = fr.plane_height[c];
        out->pitch[c] = fr.pitch[c];
        out->plane[c] = host + fr.plane_off[c];
    }
    return 0;
}

// .lep -> pixels: the front at scale 1, lep_gpu_rgb_device on the planes where they lie, and only the pixels come down.
int lep_decompress_rgb(lep_gpu* g, const uint8_t* lepdata, size_t len, lep_rgb* out) {
    if (!g) return LEP_GPU_ERROR;
    if (!out) return LEP_ASSERTION_FAILURE;
    memset(out, 0, sizeof *out);
    Front fr;
    if (int rc = fr.open(g, lepdata, len)) return rc;
    const lep::JpegFile& jf = fr.jpeg();
    // what lep_gpu_rgb_device would refuse is refused here, before anything is launched, as a file this call does not take
    const int nc = fr.d.ncomp;
    if (nc != 1 && nc != 3) return lep::gpu_refuse(g, LEP_UNSUPPORTED_JPEG, "lep_decompress_rgb: " + std::to_string(nc) + " components (1 or 3)");
    lep_rgb_image m;
    memset(&m, 0, sizeof m);
    m.width = jf.width; m.height = jf.height; m.ncomp = nc;
    int hmax = 1, vmax = 1;
    for (int c = 0; c < nc; ++c) {
        m.h_samp[c] = jf.comp[c].hs; m.v_samp[c] = jf.comp[c].vs;
        hmax = jf.comp[c].hs > hmax ? jf.comp[c].hs : hmax; vmax = jf.comp[c].vs > vmax ? jf.comp[c].vs : vmax;
    }
    for (int c = 0; c < nc && nc > 1; ++c)
        if (m.h_samp[c] < 1 || m.v_samp[c] < 1 || hmax % m.h_samp[c] || vmax % m.v_samp[c])
            return lep::gpu_refuse(g, LEP_UNSUPPORTED_JPEG, "lep_decompress_rgb: component " + std::to_string(c) + " is sampled " + std::to_string(m.h_samp[c]) + " x " +
                                   std::to_string(m.v_samp[c]) + " in a frame of " + std::to_string(hmax) + " x " + std::to_string(vmax) + ": no integral factor");
    m.convert = nc == 3 && components_are_ycbcr(jf) ? 1 : 0;
    if (int rc = fr.planes(1)) return rc;
    const int channels = nc == 1 ? 1 : 3;
    const size_t row = (size_t)jf.width * channels, bytes = row * (size_t)jf.height;
    void* d_rgb = nullptr;
    if (int rc = lep_gpu_malloc(g, bytes + 16, &d_rgb)) return rc;
    struct Free { lep_gpu* g; void* p; ~Free() { lep_gpu_free(g, p); } } release{g, d_rgb};
    for (int c = 0; c < nc; ++c) { m.d_plane[c] = fr.d_planes0 + fr.plane_off[c]; m.plane_pitch[c] = fr.pitch[c]; }
    m.d_rgb = (uint8_t*)d_rgb; m.rgb_pitch = (int32_t)row;
    m.y_first = 0; m.y_end = jf.height;
    if (int rc = lep_gpu_rgb_device(g, &m, 1, nullptr)) return rc;
    uint8_t* host = (uint8_t*)malloc(bytes ? bytes : 1);
    if (!host) return LEP_OS_ERROR;
    if (int rc = lep_gpu_memcpy_d2h(g, host, d_rgb, bytes)) { free(host); return rc; }
    out->width = jf.width; out->height = jf.height; out->channels = channels; out->pitch = (int32_t)row;
    out->pixels = host;
    return 0;
}

}  // extern "C"
