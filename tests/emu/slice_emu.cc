// slice_emu.cc -- TEST ONLY: blind_wide_emu.cc (core_emu.cc and the lane passes with their side array) with one more driver: a scan decoded
// with lep_huffdec_image.first_mcu_row = r by BOTH scan decoders -- the lane-per-subsequence passes stepped as the launch code runs them
// (lep_huffdec_simt.h) and the single-wave kernel (lep_huffdec.h).  first_mcu_row only withholds stores: the caller compares records and
// frames against r = 0.  Never linked into the product.
#include "blind_wide_emu.cc"

// lanes != 0: emu_huffman_decode_image_simt_slots with `sub_bits`; else emu_huffman_decode_image.  The frame is img->blocks (zeroed by the caller).
extern "C" int emu_huffman_decode_image_from_row(const lep_huffdec_image* img, int first_mcu_row, int lanes, uint32_t sub_bits, lep_huffdec_row* rows) {
    lep_huffdec_image im;
    memcpy(&im, img, sizeof im);
    im.first_mcu_row = first_mcu_row;
    if (lanes) return emu_huffman_decode_image_simt_slots(&im, rows, sub_bits, nullptr, nullptr);
    return emu_huffman_decode_image(&im, rows);
}
