// blind_wide_emu.cc -- TEST ONLY: core_emu.cc with one more entry point to scan_dec_driver.h, which hands the passes of lep_huffdec_simt.h what
// the launch code (lep_gpu_huffman_decode_simt_device) hands the kernels: the side array of slot sums that blind images of more than four
// blocks per MCU need (SimtSlots, sized and offset by the launch code's plan) and the lanes' columns (SimtColumns, LDS on the GPU).
// core_emu.cc's own emu_huffman_decode_image_simt passes no side array, and to it such an image is what it was before there was one.
// Never linked into the product.
#include "core_emu.cc"

// emu_huffman_decode_image_simt with the side array: same arguments, same result conventions
extern "C" int emu_huffman_decode_image_simt_slots(const lep_huffdec_image* img, lep_huffdec_row* rows, uint32_t sub_bits, int32_t* settle_moved, uint32_t* nsub_out) {
    return emu_simt_decode_one(img, rows, sub_bits, settle_moved, nsub_out, true);
}
