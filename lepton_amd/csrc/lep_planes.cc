// lep_planes.cc -- lep_decompress_planes: a .lep file to 8-bit sample planes (lep_samples.h).  A source of its own because it is the one
// whole-file call that drives the device through the lep_gpu_*_device entry points: lep_api.cc stays linkable with the host parsers alone.
#include "../../include/lepton_mi355x.h"

#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "jpeg_model.h"
#include "lep_container.h"
#include "lep_handles.h"

extern "C" {

// .lep -> sample planes.  The front is lep_decompress's: the same parse, the same decode launch on a zero-filled frame, the same exit
// codes.  The frame never leaves the device: lep_gpu_samples_device reads it where the decoder left it, and the planes come down.
int lep_decompress_planes(lep_gpu* g, const uint8_t* lepdata, size_t len, int scale, lep_planes* out) {
    if (!g) return LEP_GPU_ERROR;
    if (!out || (scale != 1 && scale != 8)) return LEP_ASSERTION_FAILURE;
    memset(out, 0, sizeof *out);
    lep_file* f = nullptr;
    if (int rc = lep_file_open_next(lepdata, len, nullptr, &f)) return rc;
    std::unique_ptr<lep_file> hold(f);
    const lep::JpegFile& jf = f->lf.jpeg;
    lep_image_desc d;
    lep_file_describe_into(f, nullptr, (size_t)-1, &d);   // geometry only: the frame is device memory
    lep_segment segs[LEP_MAX_SEGMENTS];
    lep_bytes streams[LEP_MAX_SEGMENTS];
    const int n = lep_file_segments(f, segs, streams, 0);
    // one device allocation: frame | planes | streams | lengths | statuses
    size_t frame_bytes = 0, plane_bytes = 0, stream_bytes = 0;
    size_t plane_off[LEP_MAX_COMPONENTS] = {0, 0, 0};
    int32_t pitch[LEP_MAX_COMPONENTS] = {0, 0, 0};
    for (int c = 0; c < d.ncomp; ++c) {
        frame_bytes += (size_t)d.width_blocks[c] * d.height_blocks[c] * 128;
        out->plane_width[c] = pitch[c] = d.width_blocks[c] * 8 / scale;
        out->plane_height[c] = d.height_blocks[c] * 8 / scale;
        plane_off[c] = plane_bytes;
        plane_bytes += ((size_t)pitch[c] * out->plane_height[c] + 15) & ~(size_t)15;
    }
    std::vector<uint64_t> offs((size_t)n + 1, 0);
    std::vector<uint32_t> lens((size_t)n, 0);
    for (int s = 0; s < n; ++s) { offs[s + 1] = offs[s] + streams[s].len; lens[s] = (uint32_t)streams[s].len; }
    stream_bytes = (offs[n] + 16 + 15) & ~(size_t)15;
    void* dev = nullptr;
    if (int rc = lep_gpu_malloc(g, frame_bytes + plane_bytes + stream_bytes + (size_t)n * 8 + 16, &dev)) return rc;
    struct Free { lep_gpu* g; void* p; ~Free() { lep_gpu_free(g, p); } } release{g, dev};
    uint8_t* const d_frame = (uint8_t*)dev;
    uint8_t* const d_planes0 = d_frame + frame_bytes;
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
    if (int rc = lep_gpu_samples_device(g, &d, 1, scale, nullptr, nullptr, d_plane, pitch, nullptr)) return rc;
    uint8_t* host = (uint8_t*)malloc(plane_bytes ? plane_bytes : 1);
    if (!host) return LEP_OS_ERROR;
    if (int rc = lep_gpu_memcpy_d2h(g, host, d_planes0, plane_bytes)) { free(host); return rc; }
    out->width = jf.width; out->height = jf.height; out->ncomp = d.ncomp; out->scale = scale;
    for (int c = 0; c < d.ncomp; ++c) {
        out->h_samp[c] = jf.comp[c].hs; out->v_samp[c] = jf.comp[c].vs;
        out->pitch[c] = pitch[c];
        out->plane[c] = host + plane_off[c];
    }
    return 0;
}

}  // extern "C"
