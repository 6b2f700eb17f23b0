// lep_stream_session.h -- what lep_decompress_stream (lep_stream.cc) and lep_decompress_batch_stream (lep_batch_stream.cc) share: the rule
// that says which files are decoded in a session, and the owners of a call's device memory and of its open session.
#pragma once
#include <vector>

#include "../../include/lepton_mi355x.h"
#include "lep_handles.h"

namespace lep {

// Is this parsed file one that is streamed -- any single file the split re-coder plans (recode_prepare says gpu_ok): a whole baseline file
// ('Z') or a -startbyte / -trunc slice ('Y'), one scan of one, two or three components, several thread segments or one, cut inside the scan
// or not, with or without restart intervals?  Not streamed: chains of files, and whatever recode_prepare does not plan or declines
// (progressive files, sequential frames in several scans, cut files with restart intervals or one component, the layouts it sends to the
// host re-coder).  true: *plan is its plan, segs / streams (LEP_MAX_SEGMENTS each) its *nseg segments.  lep_file_streams_in_session is
// this rule for a caller without a device.
bool streams_in_session(lep_file* f, const uint8_t* lepdata, size_t len, RecodePlan* plan, lep_segment* segs, lep_bytes* streams, int* nseg);

struct DeviceMem {   // device allocations of one call, freed when it returns
    lep_gpu* g;
    std::vector<void*> ptrs;
    explicit DeviceMem(lep_gpu* g_) : g(g_) {}
    ~DeviceMem() { for (void* p : ptrs) lep_gpu_free(g, p); }
    DeviceMem(const DeviceMem&) = delete;
    DeviceMem& operator=(const DeviceMem&) = delete;
    int get(size_t bytes, void** out) { int rc = lep_gpu_malloc(g, bytes, out); if (!rc) ptrs.push_back(*out); return rc; }
};
struct SessionEnd { lep_gpu* g; bool open = false; ~SessionEnd() { if (open) lep_gpu_decode_rows_end(g); } };

}  // namespace lep
