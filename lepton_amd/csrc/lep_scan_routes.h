// lep_scan_routes.h -- which of the two sequential scan decoders an image goes to: ONE rule, for the lane decoder's launch plan
// (lep_huffdec_simt.h simt_dec_plan), the progressive decoder's (lep_scan_decode_plan.h) and the batch pipeline (lep_batch.hip), which
// sees the C ABI's struct and none of the kernels' headers -- hence a header of its own and a template over the struct.
#pragma once

namespace lephuff {

// The lane-per-subsequence decoder (lep_huffdec_simt.h) takes an image without restart intervals, and one with them whose markers all
// stand where they should and whose positions the caller has put behind the scan bytes (flags & 2: LEP_HUFFDEC_RST_TABLE, kHuffDecRstTable).
// An interval without that table is the single-wave kernel's (lep_huffdec.h).
template <class Image>
inline bool simt_dec_takes(const Image& im) { return im.rsti == 0 || (im.flags & 2) != 0; }

}  // namespace lephuff
