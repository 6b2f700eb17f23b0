// blind_wide_emu.cc -- TEST ONLY: core_emu.cc with one more driver for lep_huffdec_simt.h, which hands the passes what the launch code
// (lep_gpu_huffman_decode_simt_device) hands the kernels: the side array of slot sums that blind images of more than four blocks per
// MCU need (SimtSlots, sized as there) and the lanes' columns (SimtColumns, LDS on the GPU).  core_emu.cc's own
// emu_huffman_decode_image_simt passes neither, and to it such an image is what it was before the side array existed.  Never linked
// into the product.
#include "core_emu.cc"

// emu_huffman_decode_image_simt with the side array: same arguments, same result conventions
extern "C" int emu_huffman_decode_image_simt_slots(const lep_huffdec_image* img, lep_huffdec_row* rows, uint32_t sub_bits, int32_t* settle_moved, uint32_t* nsub_out) {
    static lephuff::SimtShared sh;
    static lephuff::SimtColumns cols;
    static lephuff::SimtTile tile;
    lephuff::HuffDecImage im;
    memcpy(&im, img, sizeof im);
    im.rows_off = 0;
    const uint32_t L = (sub_bits + 31u) & ~31u;
    if (!L) return -1;
    lephuff::SimtImage si;
    memset(&si, 0, sizeof si);
    si.first = 0; si.sub_bits = L;
    si.nsub = (uint32_t)std::max<uint64_t>(1, ((uint64_t)im.scan_len * 8u + L - 1) / L);
    if (im.flags & lephuff::kHuffDecRstTable) {   // lane = restart interval
        if (im.rsti <= 0 || im.mcuc <= 0) return -1;
        si.nsub = (uint32_t)((im.mcuc - 1) / im.rsti) + 1u;
        si.changed[0] = 0xff;
    }
    std::vector<lephuff::SimtSub> buf[2] = {std::vector<lephuff::SimtSub>(si.nsub), std::vector<lephuff::SimtSub>(si.nsub)};
    std::vector<lephuff::SimtPlace> place(si.nsub);
    // (an entry per subsequence of a wide blind image, none for any other -- but the pointer is passed all the same, as the launch code does)
    std::vector<lephuff::SimtSlots> slots((lephuff::simt_blind_wide(&im) ? si.nsub : 0) + 1);
    si.slots = 0;
    lephuff::HuffDecRow* r = reinterpret_cast<lephuff::HuffDecRow*>(rows);
    for (int k = 0; k <= lephuff::kSimtSettle; ++k)
        for (uint32_t f = 0; f < si.nsub; f += 64) lephuff::simt_guess_or_settle(&im, &sh, &si, buf[(k + 1) & 1].data(), buf[k & 1].data(), f, k, slots.data(), &cols);
    const lephuff::SimtSub* fin = buf[lephuff::kSimtSettle & 1].data();
    lephuff::simt_place(&im, &si, fin, place.data(), lephuff::kSimtSettle, r, slots.data());
    for (uint32_t f = 0; f < si.nsub; f += 64) lephuff::simt_write(&im, &sh, &tile, &si, fin, place.data(), r, f);
    if (rows[im.mcuv].aux == lephuff::kHuffDecRowUnwritten) { si.status |= 2; rows[im.mcuv].aux = 255; }   // (lep_huffman_simt_finish_kernel)
    if (im.flags & lephuff::kHuffDecRstTable) {
        int status = si.status & 0x3fffff;
        const int pad = lephuff::simt_intervals_pad(&si, &status);
        rows[im.mcuv].aux = pad | (status << 8);
    } else
        rows[im.mcuv].aux = (rows[im.mcuv].aux & (255 | lephuff::kHuffDecRowTruncated)) | ((si.status & 0x3fffff) << 8);
    if (settle_moved) for (int k = 0; k <= lephuff::kSimtSettle; ++k) settle_moved[k] = si.changed[k];
    if (nsub_out) *nsub_out = si.nsub;
    return 0;
}
