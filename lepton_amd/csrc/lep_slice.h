// lep_slice.h -- `-startbyte` slices inside the library: what the batch pipeline (lep_batch.hip) needs of a slice beyond the public header.
// Defined in lep_api.cc beside their public whole-file forms; not part of the C ABI.
#pragma once
#include "../../include/lepton_mi355x.h"

// lep_jpeg_open_slice with the coefficient frame decoded into caller-provided memory (lep_jpeg_open_into's contract)
int lep_jpeg_open_slice_into(const uint8_t* jpg, size_t len, size_t start_byte, void* frame_mem, size_t frame_cap, lep_jpeg** out);
// lep_jpeg_open_gpu for a slice: the same layouts are eligible, the scan is decoded from its first block, and lep_jpeg_finish_gpu drops the
// hand-off rows in front of start_byte and collects the prefix garbage -- from `jpg`, which must stay alive until then
int lep_jpeg_open_gpu_slice(const uint8_t* jpg, size_t len, size_t start_byte, lep_jpeg** out, lep_huffdec_image* image, int* eligible);
// the first luma block row a parsed slice keeps (its first hand-off's luma_y_start; 0 for a whole file): the frame rows in front of it are
// read by nobody -- not coded, not restored, not compared
int lep_jpeg_first_kept_luma_row(const lep_jpeg* j);
// 1: a whole file, or a slice whose hand-offs tile its bytes like a whole file's -- at least one MCU row kept and the first kept record
// BEHIND start_byte, so that the prefix garbage ends where the writer's first byte stands.  0: a slice the reference's own re-coder may
// not restore (first record exactly at start_byte, the final record alone): lep_compress_slice, which always restores and compares, decides
int lep_jpeg_slice_tiles(const lep_jpeg* j);
