/*
 * lepton_mi355x.h -- C ABI of liblepton_mi355x.so, the MI355X-native drop-in for Lepton's
 * arithmetic-coding hot path (the code behind BaseEncoder::encode_chunk / BaseDecoder::decode_chunk,
 * src/lepton/base_coders.hh:26-65 of dropbox/lepton).  Plain pointers and sizes only.
 *
 * Layers, bottom up:
 *   1. lep_gpu_*        the hot path itself: batches of (image x thread-segment) work items coded by
 *                        HIP kernels on gfx950.  Replaces VP8ComponentEncoder::vp8_full_encoder's
 *                        per-segment loop (src/lepton/vp8_encoder.cc:239-445, 460-519) and
 *                        VP8ComponentDecoder::decode_chunk / LeptonCodec::decode_row
 *                        (src/lepton/vp8_decoder.cc:387-490, src/lepton/lepton_codec.cc:7-47,119-309).
 *   2. lep_jpeg_* / lep_file_*   host-side callers either side of the hot path (JPEG <-> coefficient
 *                        frames, .lep container); what src/lepton/jpgcoder.cc + recoder.cc do.
 *   3. lep_compress / lep_decompress   whole-file convenience = `lepton in.jpg out.lep` and back.
 *
 * Return values are the reference's process exit codes (src/vp8/util/memory.hh:13-40); 0 = SUCCESS.
 * There is NO CPU fallback: every lep_gpu_* entry point fails with LEP_GPU_ERROR when no gfx950
 * device or kernel image is available.
 */
#ifndef LEPTON_MI355X_H
#define LEPTON_MI355X_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum {
    LEP_SUCCESS = 0, LEP_ASSERTION_FAILURE = 1, LEP_CODING_ERROR = 2, LEP_SHORT_READ = 3,
    LEP_UNSUPPORTED_4_COLORS = 4, LEP_COEFFICIENT_OUT_OF_RANGE = 6, LEP_STREAM_INCONSISTENT = 7,
    LEP_PROGRESSIVE_UNSUPPORTED = 8, LEP_SAMPLING_BEYOND_TWO_UNSUPPORTED = 10,
    LEP_THREADING_PARTIAL_MCU = 12, LEP_VERSION_UNSUPPORTED = 13, LEP_ONLY_GARBAGE_NO_JPEG = 14, LEP_OS_ERROR = 33,
    LEP_SAMPLING_BEYOND_FOUR_UNSUPPORTED = 11,
    LEP_OOM = 37,                      /* a .lep whose header claims sizes beyond the reference's 576 MiB arena (its allocator's exit code) */
    LEP_TOO_MUCH_MEMORY_NEEDED = 38,   /* coefficient frame beyond the reference's default budget of 4,423,680 blocks (566 MB) */
    LEP_ROUNDTRIP_FAILURE = 41, LEP_UNSUPPORTED_JPEG = 42, LEP_UNSUPPORTED_JPEG_WITH_ZERO_IDCT_0 = 43,
    LEP_BUFFER_TOO_SMALL = 100,
    LEP_GPU_PATH_DECLINED = 101,       /* lep_file_recode_finish: the scan encoder stopped at the cut of a truncated file before the byte bound was
                                          reached (or does not take the file): call lep_file_recode, the host re-coder, instead */
    LEP_GPU_ERROR = 120
};

#define LEP_MAX_COMPONENTS 3   /* default reference build: ColorChannel::NumBlockTypes == 3 */
#define LEP_MAX_SEGMENTS 16    /* MuxReader::MAX_STREAM_ID, src/io/MuxReader.hh:201 */

/* One image's coefficient frame: what UncompressedComponents exposes to encode_chunk
 * (src/lepton/uncompressed_components.hh:24-302; consumed at src/lepton/vp8_encoder.cc:521-548). */
typedef struct lep_image_desc {
    int32_t ncomp;                                   /* get_num_components() */
    int32_t mcu_rows;                                /* get_mcu_count_vertical() */
    int32_t width_blocks[LEP_MAX_COMPONENTS];        /* block_width(c) */
    int32_t height_blocks[LEP_MAX_COMPONENTS];       /* full_component_nosync(c).original_height() */
    int32_t coded_blocks[LEP_MAX_COMPONENTS];        /* component_size_in_blocks(c) (truncated files) */
    int32_t coded_height[LEP_MAX_COMPONENTS];        /* get_max_coded_heights()[c] */
    uint16_t qtable_zigzag[LEP_MAX_COMPONENTS][64];  /* get_quantization_tables(c), zig-zag order */
    /* per component: width*height AlignedBlocks = 64 x int16 in "aligned" order
     * (src/vp8/util/aligned_block.hh:32-44).  HOST pointers for lep_gpu_*_host, DEVICE pointers
     * for lep_gpu_*_device. */
    int16_t *blocks[LEP_MAX_COMPONENTS];
} lep_image_desc;

/* One thread segment of one image = one independent arithmetic-coded stream = one wavefront.
 * luma_y_start/end come from ThreadHandoff (src/lepton/thread_handoff.hh:8-39). */
typedef struct lep_segment {
    int32_t image;          /* index into the images[] array of the call */
    int32_t luma_y_start;
    int32_t luma_y_end;
    int32_t is_last;        /* last segment of its image runs to the end (vp8_encoder.cc:280) */
} lep_segment;

typedef struct lep_bytes { uint8_t *data; size_t len; size_t cap; } lep_bytes;

/* ---- layer 1: the GPU hot path ------------------------------------------------------------- */
typedef struct lep_gpu lep_gpu;   /* owns a HIP stream, per-segment models and staging buffers */

int lep_gpu_create(int device, lep_gpu **out);
void lep_gpu_destroy(lep_gpu *g);
const char *lep_gpu_last_error(lep_gpu *g);
int lep_gpu_device(lep_gpu *g);   /* the HIP device this object was created on */
size_t lep_gpu_debug_huffenc(lep_gpu *g, void *out, size_t cap);   /* diagnosis: the lane-per-unit scan encoder's work area after its last launch */
int lep_gpu_pci_bus_id(lep_gpu *g, char *out, int cap);   /* its PCI address ("0000:c1:00.0", cap >= 16): which physical GPU a rank drives */

/* Encode nseg segments of nimg images.  Host variant: blocks[] are host pointers, copied to HBM,
 * coded, streams copied back into out[i] (out[i].data with capacity out[i].cap; len is set).
 * status[i] receives the per-segment exit code. */
int lep_gpu_encode_host(lep_gpu *g, const lep_image_desc *images, int nimg, const lep_segment *segs, int nseg,
                        lep_bytes *out, int32_t *status);
/* Decode: in[i] are the de-multiplexed streams; coefficient rows of each segment are written into
 * images[].blocks (host). */
int lep_gpu_decode_host(lep_gpu *g, const lep_image_desc *images, int nimg, const lep_segment *segs, int nseg,
                        const lep_bytes *in, int32_t *status);

/* Device-resident variants (inputs already in HBM; nothing crosses PCIe inside the call):
 * images[].blocks are device pointers; streams live in one device arena: segment i uses
 * [stream_offsets[i], stream_offsets[i+1]) of d_streams; d_stream_len[i] (device, uint32) is
 * written by encode and read by decode.  hip_stream may be NULL (library stream).
 * The calls enqueue work and return; lep_gpu_sync waits.  kernel_ms (may be NULL) receives the
 * HIP-event time of the kernel(s) when sync'd via lep_gpu_last_kernel_ms. */
int lep_gpu_encode_device(lep_gpu *g, const lep_image_desc *images, int nimg, const lep_segment *segs, int nseg,
                          uint8_t *d_streams, const uint64_t *stream_offsets, uint32_t *d_stream_len,
                          int32_t *d_status, void *hip_stream);
int lep_gpu_decode_device(lep_gpu *g, const lep_image_desc *images, int nimg, const lep_segment *segs, int nseg,
                          const uint8_t *d_streams, const uint64_t *stream_offsets, const uint32_t *d_stream_len,
                          int32_t *d_status, void *hip_stream);
/* Resumable decode: the launch of lep_gpu_decode_device advanced one band of MCU rows at a time, every band a launch that finishes, so
 * that the frame rows a band completed can be used (re-coded, sent on) while the rest is still to be decoded, and a stream that turns
 * inconsistent says at which block.
 *   begin    derives, orders and uploads what a decode launch needs into the current workspace set (lep_gpu_use_arena) and clears the
 *            segments' resume records.  d_streams / d_stream_len and the frames stay the caller's and must live until `end`.
 *   advance  launches one band on the session's stream, waits for it and copies the records back: every running segment decodes on
 *            up to the MCU row (the one it stood in + band_mcu_rows); band_mcu_rows <= 0 = to the end.  progress[nseg] (host, the
 *            caller's segment order; may be NULL) and *running (segments still running; may be NULL) are filled.  The frames are
 *            readable between two advances.  A segment that finished or failed is not touched by later advances.
 *   end      closes the session.
 * A session owns the workspace set that was current at `begin`: until `end`, encode / decode launches and a second `begin` on that set,
 * and lep_gpu_trim / lep_gpu_release_memory (which take both sets' memory), return LEP_ASSERTION_FAILURE with a lep_gpu_last_error
 * text; the other set stays usable after lep_gpu_use_arena.  advance / end act on the set that is current when they are called.
 * lep_gpu_decode_device / _host are unchanged and do not go through the banded kernel. */
typedef struct lep_decode_progress {       /* one per segment, caller's order */
    int32_t status;                        /* -1 running, -2 retired by the caller, 0 finished, otherwise the exit code */
    int32_t rows_done[LEP_MAX_COMPONENTS]; /* every block row of component c that is this segment's and lies below rows_done[c] is in the frame */
    int32_t fail_component, fail_y, fail_x;/* the block at which status became non-zero (it is not stored, everything before it is); -1 otherwise */
    uint32_t bins;
} lep_decode_progress;
int lep_gpu_decode_rows_begin(lep_gpu *g, const lep_image_desc *images, int nimg, const lep_segment *segs, int nseg,
                              const uint8_t *d_streams, const uint64_t *stream_offsets, const uint32_t *d_stream_len, void *hip_stream);
int lep_gpu_decode_rows_advance(lep_gpu *g, int band_mcu_rows, lep_decode_progress *progress /* host, nseg */, int *running);
int lep_gpu_decode_rows_end(lep_gpu *g);
/* Between two advances (or before the first): the session's segments seg_index[0..n) -- the caller's order, as in progress[] -- are
 * retired.  A retired segment is decoded no further: later advances leave at its record, touch nothing of it and do not count it in
 * *running; its progress.status is -2 and its rows_done stays what the last band left.  Rows below rows_done are in the frame, nothing
 * behind them was stored.  A segment that has finished or failed keeps its state.  The record's state word is written by a copy in
 * the order of the session's stream.  LEP_ASSERTION_FAILURE with a lep_gpu_last_error text: no session on the current workspace set,
 * or an index that is not one of the session's.  A caller that never retires sees no difference. */
int lep_gpu_decode_rows_retire(lep_gpu *g, const int32_t *seg_index, int n);
/* Workspace set (0 or 1) the next lep_gpu_*_device launches use.  Two launches that overlap in time (different hip streams) must
 * use different sets; a set may be reused once the launch that used it has finished (stream order does that when the same
 * stream always goes with the same set).  Default 0. */
int lep_gpu_use_arena(lep_gpu *g, int k);
/* on = 1: the decode launches that follow will share the chip with a neighbour launch on another stream (both workspace sets in use):
 * they take the register budget that lets two launches' wavefronts sit on one SIMD.  0 = back to choosing by launch size. */
int lep_gpu_expect_company(lep_gpu *g, int on);
/* A caller that passed streams of its own (`hip_stream` arguments) calls this BEFORE destroying them: the object's descriptor-upload
 * ring holds events recorded on those streams; this waits for the copies and drops the events. */
int lep_gpu_settle_uploads(lep_gpu *g);
int lep_gpu_sync(lep_gpu *g);
double lep_gpu_last_kernel_ms(lep_gpu *g);          /* HIP-event duration of the most recent encode / decode / scan / sample launch (ms; -1: none timed) */
/* The split-phase encoder (lep_enc5.h) is several kernels: stage times of the most recent encode launch that used it, in
 * order count + plan, emit, fold, gather, write (HIP events on the launch stream); returns how many were written (0: the
 * launch was a single-kernel one). */
int lep_gpu_last_stage_ms(lep_gpu *g, double *ms, int cap);
const char *lep_gpu_last_kernel_name(lep_gpu *g);   /* which kernel generation / register-budget variant that launch used */
/* Tests: the split-phase encoder's bool writer kernels on bin lists the caller gives -- one list per segment, `bins` holds them back to
 * back (entries probability | bit << 8), nbins[s] their lengths -- launched in the encoder's order, by the encoder's own launch function, in
 * one of its three forms (csrc/lep_enc5_plan.h: which of them a launch of the encoder takes, and with which cut):
 *   LEP_DEBUG_WRITE_LANE         the lane-per-segment writer in `parts` parts (1..8; chunks is not read)
 *   LEP_DEBUG_WRITE_STITCHED     range / link / code / stitch over `chunks` chunks per segment (1..256; parts = 1)
 *   LEP_DEBUG_WRITE_PART_CHUNKS  range / link / code of `chunks` (1..32) chunks per part, part by part, then one stitch
 * For the forms in parts with parts > 1, part_first[s * parts + p] is the first bin of segment s's part p: 0 for p = 0, ascending, at
 * most nbins[s]; equal neighbours are empty parts.  A part's bins reach the device when the part's kernels are queued.
 * Segment s writes into [stream_off[s], stream_off[s] + stream_cap[s]) of an output arena of arena_bytes that the call fills with the
 * byte `guard` first; the reservations ascend and may leave gaps.  plan_status (may be NULL): a non-zero entry is a segment the walks
 * refused -- the writer passes the code on and codes nothing.  The whole arena comes back in arena_out, with stream_len[nseg] and
 * status[nseg] (both start as 0x7f7f7f7f) and, for the chunked forms, the writer's records in wchunks (may be NULL): per segment
 * parts * chunks records of 16 uint32 -- q_guess, q_end, shifts, q_start, t_start, keep, keep_bits, carry, pos_end, 7 unused.
 * Uses memory of its own and the object's stream; waits for the result.  LEP_ASSERTION_FAILURE: arguments out of range, or a decode
 * session owns the current workspace set. */
enum { LEP_DEBUG_WRITE_LANE = 0, LEP_DEBUG_WRITE_STITCHED = 1, LEP_DEBUG_WRITE_PART_CHUNKS = 2 };
int lep_gpu_debug_write_bins(lep_gpu *g, int form, int parts, int chunks, int nseg, const uint16_t *bins, const uint32_t *nbins,
                             const uint64_t *stream_off, const uint32_t *stream_cap, const int32_t *plan_status, const uint32_t *part_first,
                             int guard, uint8_t *arena_out, size_t arena_bytes, uint32_t *stream_len, int32_t *status, void *wchunks);
/* Tests: the stitched writer's records of the most recent encode launch, in the caller's segment order, parts * chunks per segment
 * in the layout above; *nseg, *parts and *chunks (each may be NULL) say how that launch cut its segments -- parts = 1 for the writer
 * behind gather.  Returns parts * chunks, 0 when that launch used another writer; the records are copied when cap_records holds them all. */
int lep_gpu_debug_wchunks(lep_gpu *g, void *out, size_t cap_records, int *nseg, int *parts, int *chunks);
/* JPEG Huffman re-encode of decoded coefficient frames on the GPU (replaces recode_one_mcu_row / encode_block_seq,
 * src/lepton/recoder.cc:316-412, 245-314, for whole, untruncated sequential scans): one wavefront per thread segment writes
 * that segment's scan bytes (FF00-stuffed, RST markers included) to d_out + segs[i].out_off, at most segs[i].out_cap of
 * them; d_out_len[i] receives the count.  images[].blocks are device pointers.  lep_file_recode_plan fills both structs. */
typedef struct lep_huff_image {
    int32_t ncomp, mcuh, mcuv, mcuc;
    int32_t rsti, padbit;
    uint32_t rst_limit;
    int32_t interleaved;                 /* 1: MCUs of hs x vs blocks per component.  A one-component file (never interleaved: MCU = one block, the scan steps over the
                                          * frame's padding blocks) is planned as mcuh x mcuv = its nch x ncv blocks, hs = vs = 1, block rows bch apart, segments in block rows */
    int32_t hs[4], vs[4], bch[4];
    int32_t dc_tbl[4], ac_tbl[4];
    int32_t scan_cmp[4];
    int32_t trunc_bc[4];                 /* a file cut inside its scan (EEE section): blocks of each component in front of the cut; 0 = whole */
    const int16_t *blocks[4];
    uint32_t code[4][256];               /* [0..1] DC, [2..3] AC tables: code length << 16 | code */
} lep_huff_image;
typedef struct lep_huff_segment {
    int32_t image, mcu_row0, mcu_row1;
    uint32_t overhang;                   /* overhang_byte | num_overhang_bits << 8 (ThreadHandoff) */
    int16_t last_dc[4];
    uint64_t out_off;
    uint32_t out_cap;
    uint32_t pad;
} lep_huff_segment;
/* What a segment's writer ends in -- partial byte, its bit count, last DC per component -- i.e. what the NEXT hand-off must
 * have recorded: the reference asserts all three at every segment end (recode_physical_thread, src/lepton/recoder.cc:625-640);
 * lep_file_recode_finish holds them against the file's hand-offs.  attempted = bytes before clipping to out_cap. */
typedef struct lep_huff_end {
    uint32_t attempted;
    uint8_t overhang_byte, num_overhang_bits;
    int16_t last_dc[4];
    uint16_t pad;
} lep_huff_end;
/* d_ends: nseg records in device memory, or NULL.  Segments (of MCU-interleaved scans and of one-component files, with or without restart intervals) are written with one
 * lane per run of at most eight MCUs (lep_huff_simt.h: count, prefix sums, code, stuff; a run ends where its restart interval does and
 * carries the pad bits and the marker), the others with one wavefront per segment (lep_huff.h);
 * same bytes, same end states (LEP_HUFFENC_SIMT=0: the wavefront form for all).  `pad` of a segment is the library's: pass it as 0 (lep_file_recode_plan does).
 * The call copies its arrays before it returns and does not wait for the stream. */
int lep_gpu_huffman_encode_device(lep_gpu *g, const lep_huff_image *images, int nimg, const lep_huff_segment *segs, int nseg,
                                  uint8_t *d_out, uint32_t *d_out_len, lep_huff_end *d_ends, void *hip_stream);
/* Concatenate n byte runs that lie apart in device memory (lep_pack.h: a prefix-sum kernel of one workgroup, a copy kernel of one
 * wavefront per run that stores whole dwords to the aligned destination, byte heads and tails).  Run i is d_len[i] bytes at
 * d_src + src_off[i]; src_off is a host array that the call copies, d_len is device memory.  The runs go to d_dst back to back, in order;
 * sources and destinations may be aligned in any way.  d_dst_off[0..n] (device) receives the exclusive prefix sum of the lengths,
 * d_dst_off[n] the total; nothing behind d_dst + d_dst_off[n] is written.  A total beyond d_dst_cap copies nothing, and d_dst_off[n] still
 * holds the true total.  Enqueues on hip_stream and returns.  n <= 16384.  Its scratch is the current arena set's own and no decode
 * session's: it may be called while a session is open on that set. */
int lep_gpu_pack_device(lep_gpu *g, const uint8_t *d_src, const uint64_t *src_off, const uint32_t *d_len, int n,
                        uint8_t *d_dst, uint64_t d_dst_cap, uint64_t *d_dst_off, void *hip_stream);
/* The same with a window per run: run i contributes its bytes [win_skip[i], min(d_len[i], win_skip[i] + win_take[i])) -- nothing when
 * d_len[i] <= win_skip[i].  win_skip / win_take are host arrays that the call copies; the clipped lengths are made on the device from
 * d_len, and d_dst_off[0..n] is their prefix sum.  The copy starts at d_src + src_off[i] + win_skip[i] at whatever alignment that leaves,
 * loads no dword that holds no byte of the window and writes nothing behind d_dst + d_dst_off[n]; the cap, n <= 16384 and the use while a
 * session is open are as above. */
int lep_gpu_pack_window_device(lep_gpu *g, const uint8_t *d_src, const uint64_t *src_off, const uint32_t *d_len,
                               const uint32_t *win_skip, const uint32_t *win_take, int n,
                               uint8_t *d_dst, uint64_t d_dst_cap, uint64_t *d_dst_off, void *hip_stream);
/* Coefficient frames in device memory -> 8-bit sample planes, one per component at the component's own resolution: no upsampling, no
 * colour conversion, no cropping (lep_samples.h; nimg images in one launch; enqueues on hip_stream and returns; lep_gpu_last_kernel_ms
 * times it).  images[].blocks are device pointers, 16-byte aligned, the frames exactly as the coders keep them.  Plane k = image * 3 +
 * component is width_blocks * 8 / scale by height_blocks * 8 / scale samples at d_planes[k], pitch[k] bytes from row to row; entries of
 * components an image does not have are not read.
 * The arithmetic.  d[k] = c[k] * q[k], an 8x8 raster per block.
 *   scale 1: the two-pass integer transform of libjpeg's jidctint ("islow") with 13-bit constants, columns first, then rows; with the
 *   inputs i0..i7 of one column or row
 *       z1 = (i2+i6)*4433;  t2 = z1 - i6*15137;  t3 = z1 + i2*6270
 *       t0 = (i0+i4)<<13;   t1 = (i0-i4)<<13
 *       t10 = t0+t3; t13 = t0-t3; t11 = t1+t2; t12 = t1-t2
 *       a0 = i7; a1 = i5; a2 = i3; a3 = i1
 *       z1 = a0+a3; z2 = a1+a2; z3 = a0+a2; z4 = a1+a3; z5 = (z3+z4)*9633
 *       a0 *= 2446; a1 *= 16819; a2 *= 25172; a3 *= 12299
 *       z1 *= -7373; z2 *= -20995; z3 = z3*-16069 + z5; z4 = z4*-3196 + z5
 *       a0 += z1+z3; a1 += z2+z4; a2 += z2+z3; a3 += z1+z4
 *       out[0..7] = t10+a3, t11+a2, t12+a1, t13+a0, t13-a0, t12-a1, t11-a2, t10-a3
 *   each output descaled as (x + (1 << (s-1))) >> s, arithmetic shift, s = 11 behind the column pass and 18 behind the row pass; the
 *   sample is clamp(result + 128, 0, 255).
 *   scale 8: one sample per block, clamp(((d[0] + 4) >> 3) + 128, 0, 255).
 *   Exact integer arithmetic -- equal to libjpeg's islow decoder sample for sample -- for frames in which every |d[k]| <= 32767 and every
 *   value between the passes is <= 32767 in magnitude (real files: |d| up to 1020, 4188 between the passes); outside, what the formulas
 *   give in wrapping 32-bit arithmetic, where libjpeg does not agree with itself either.
 * row_first / row_end ([nimg * 3] block rows per plane, both NULL = every row): only the sample rows of block rows [row_first, row_end)
 * are written, at their place in the plane -- a caller that holds a decode session (lep_gpu_decode_rows_*) turns each finished band
 * into samples; the call uses no workspace of a session and may be made while one is open.  An empty range writes nothing.
 * LEP_ASSERTION_FAILURE with a lep_gpu_last_error text, nothing launched: a scale other than 1 or 8, a pitch below the plane's width, a
 * row range that is not inside the component, a missing or misaligned frame, a missing plane.  LEP_GPU_ERROR as everywhere. */
int lep_gpu_samples_device(lep_gpu *g, const lep_image_desc *images, int nimg, int scale /* 1 or 8 */,
                           const int32_t *row_first, const int32_t *row_end, /* [nimg*3] block rows per component, NULL = all */
                           uint8_t *const *d_planes /* [nimg*3] */, const int32_t *pitch /* [nimg*3], bytes */, void *hip_stream);
/* 8-bit sample planes in device memory (what lep_gpu_samples_device writes at scale 1) -> pixels: interleaved R,G,B, 3 bytes per pixel,
 * or 1 byte per pixel for a one-component image, cropped to width x height (lep_rgb.h; nimg images of whatever geometry in one launch;
 * enqueues on hip_stream and returns; lep_gpu_last_kernel_ms times it).  Equal byte for byte to libjpeg's default full-scale output
 * (fancy upsampling, no merged upsampling, jdcolor's table arithmetic) when the planes are lep_gpu_samples_device's.
 * The definition.
 *   Geometry.  hmax = max h_samp, vmax = max v_samp.  Component c: dw = ceil(width * h_c / hmax), dh = ceil(height * v_c / vmax); only
 *   the top-left dw x dh samples of its plane are used, x[r][k]; the rest of the block grid is ignored.  fh = hmax / h_c, fv = vmax / v_c
 *   must be integers.  A one-component image has fh = fv = 1 whatever its factors say.
 *   Upsampling.  Neighbours out of range are the edge sample itself: up(r) = x[max(r-1, 0)], dn(r) = x[min(r+1, dh-1)], columns alike
 *   with dw; division is an arithmetic right shift; the result is cropped to width x height.
 *     (fh, fv) = (1, 1)   out = x
 *     (2, 1), dw > 2      out[y][2k] = (3 x[y][k] + x[y][k-1] + 1) >> 2;   out[y][2k+1] = (3 x[y][k] + x[y][k+1] + 2) >> 2
 *     (1, 2), any width   out[2r][k] = (3 x[r][k] + up(r)[k] + 1) >> 2;    out[2r+1][k] = (3 x[r][k] + dn(r)[k] + 2) >> 2
 *     (2, 2), dw > 2      s[2r][k] = 3 x[r][k] + up(r)[k];  s[2r+1][k] = 3 x[r][k] + dn(r)[k]   (not rounded)
 *                         out[y][2k] = (3 s[y][k] + s[y][k-1] + 8) >> 4;   out[y][2k+1] = (3 s[y][k] + s[y][k+1] + 7) >> 4
 *     (2, 1) or (2, 2) with dw <= 2, and every other integral pair (a factor of 3 or 4, (2, 4), (4, 2), ...): replication,
 *                         out[y][x] = x[y / fv][x / fh]
 *   Colour (convert != 0).  FIX(f) = (int)(f * 65536 + 0.5), cb' = Cb - 128, cr' = Cr - 128, clamp to 0..255:
 *     R = clamp(Y + ((FIX(1.40200) cr' + 32768) >> 16));   B = clamp(Y + ((FIX(1.77200) cb' + 32768) >> 16))
 *     G = clamp(Y + ((-FIX(0.34414) cb' + 32768 - FIX(0.71414) cr') >> 16))
 *   convert == 0: the components are R, G, B as they are -- upsampled all the same, not converted.
 * Only output rows [y_first, y_end) are written, at their place; the call reads source rows up to one above and one below the rows the
 * range maps to, inside [0, dh), and the caller guarantees that those are in the planes: a holder of a decode session colours the
 * bands that are finished.  An empty range writes nothing.  Uses no workspace of a session.
 * LEP_ASSERTION_FAILURE with a lep_gpu_last_error text, nothing launched: a missing plane or output, a plane pitch below dw, an rgb_pitch
 * below the row's bytes, a row range that is not inside the image, ncomp other than 1 or 3, sampling factors outside 1..4 or not
 * integral multiples, a size outside 1..65535.  LEP_GPU_ERROR as everywhere. */
typedef struct lep_rgb_image {
    int32_t width, height, ncomp;                 /* pixels; 1 or 3 components */
    int32_t h_samp[3], v_samp[3];                 /* sampling factors */
    int32_t convert;                              /* 1: the components are Y, Cb, Cr; 0: they are R, G, B as they are */
    const uint8_t *d_plane[3];                    /* device memory: sample (0, 0) of each component */
    int32_t plane_pitch[3];                       /* bytes from row to row, >= dw */
    int32_t rgb_pitch;                            /* bytes from pixel row to pixel row, >= width * (ncomp == 1 ? 1 : 3) */
    uint8_t *d_rgb;                               /* device memory: pixel (0, 0) */
    int32_t y_first, y_end;                       /* output rows written, 0 <= y_first <= y_end <= height */
} lep_rgb_image;
int lep_gpu_rgb_device(lep_gpu *g, const lep_rgb_image *images, int nimg, void *hip_stream);
/* Progressive files that END INSIDE A SCAN (no EOI) in lep_compress_batch / lep_decompress_batch: on = 1 sends them to the scan kernels
 * (lep_jpeg_open_gpu_progressive_cut, lep_file_recode_plan_progressive_cut), on = 0 -- what a codec starts with, unless
 * LEP_CUT_PROGRESSIVE=1 was set when it was made -- keeps them with the host parser and re-coder, where every earlier release had them;
 * on < 0 changes nothing.  Returns the setting.  Same bytes and statuses either way. */
int lep_gpu_cut_progressive(lep_gpu *g, int on);
int lep_gpu_stream_pack(lep_gpu *g);   /* 1: lep_decompress_batch_stream packs a band's bytes before it fetches them; LEP_STREAM_PACK=0 when the codec is made: 0 */
/* The same for PROGRESSIVE files (BASELINE.json configs[4]; replaces the scan loop of recode_jpeg, src/lepton/jpgcoder.cc:3309-3716,
 * with encode_dc_prg_*, encode_ac_prg_fs / _sa, encode_eobrun, encode_crbits :4991-5400): every scan of a progressive file is a
 * function of the finished frame alone, so its bytes (FF00-stuffed, restart markers included) are written to d_out +
 * scans[i].out_off by one LANE per 32 blocks (lep_huffprog_simt.h: count / place / assign / code / stuff; in a scan with a restart
 * interval the units are cut at the intervals' ends); d_out_len[i] = byte count, bit 31 set = the scan outgrew its slot or its
 * scratch (let the host re-coder do that file).  d_corr: scratch for correction bits held back behind end-of-band runs
 * (scans[i].corr_off / corr_cap dwords).  lep_file_recode_plan_progressive fills both structs.
 * A file that ENDS INSIDE A SCAN (no EOI; no restart intervals): every scan is written whole from the frame, which is zero behind the
 * cut, and lep_file_recode_finish_progressive's byte bound cuts the output.  The scan the file ends in can be many times what the file
 * kept of it: its out_cap is what its geometry bounds it by, file_bound that much on top of the file's size.  A caller that decoded such
 * a file from ONE thread segment clears the frame from block coded_blocks[c] of every component on (lep_image_desc) in front of this
 * call: the reference's re-coder reads zeros there even where the stream coded a row's first block. */
typedef struct lep_huffprog_image {
    int32_t ncomp, mcuh, mcuv, mcuc;
    int32_t rsti, padbit;
    int32_t hs[4], vs[4], bch[4], bcv[4], nch[4], ncv[4], mbs[4];
    const int16_t *blocks[4];
} lep_huffprog_image;
typedef struct lep_huffprog_scan {
    int32_t image;
    int32_t cmpc, cmp[4];                /* components of the scan, in scan order */
    int32_t from, to, sah, sal;          /* spectral band, successive approximation high / low */
    int32_t max_eobrun;
    int32_t tbl[4];                      /* DC scans: table slot (0 / 1) of each scan component */
    int32_t rsti;                        /* this scan's restart interval (a DRI segment may stand in front of any scan: phone cameras write one per scan);
                                          * -1 = the image's (lep_huffprog_image.rsti).  Sits where the struct had four bytes of padding. */
    uint64_t out_off;
    uint32_t out_cap;
    uint32_t corr_off, corr_cap;         /* dwords */
    uint32_t file_bound;                 /* bytes ALL scans of this scan's image produce together at most (they are parts of one file: its
                                          * size); 0 = unknown, the sum of their out_cap.  Sizes the bit buffers of the lane-per-unit kernels. */
    uint32_t code[4][256];               /* length << 16 | code.  DC scans: [0..1] = DC tables 0 / 1; AC scans: [0] = the component's AC table; scans of
                                          * sequential frames (from 0 / to 63): [0..1] = DC tables 0 / 1, [2..3] = AC tables 0 / 1, tbl[i] = DC table | AC table << 8
                                          * of scan component i */
} lep_huffprog_scan;
int lep_gpu_huffman_progressive_encode_device(lep_gpu *g, const lep_huffprog_image *images, int nimg, const lep_huffprog_scan *scans,
                                              int nscan, uint8_t *d_out, uint32_t *d_corr, uint32_t *d_out_len, void *hip_stream);
/* How many scans of this codec's most recent lep_gpu_huffman_progressive_encode_device call (lep_decompress_batch and the round-trip check of
 * lep_compress_batch make one per chunk) went to each writer: counts[0] one lane per 32 blocks (lep_huffprog_simt.h), scans without a restart
 * interval, [1] the same kernels, scans with one (LEP_HUFFPROG_SIMT_RST=0 when the codec is made: these go to [2]), [2] one wavefront per scan
 * (lep_huffprog.h), [3] the sequential scan encoders (scans of sequential frames). */
int lep_gpu_huffman_progressive_encode_forms(lep_gpu *g, uint32_t counts[4]);
/* JPEG Huffman scan decode on the GPU (replaces decode_jpeg / decode_block_seq, src/lepton/jpgcoder.cc:2799-3302,
 * 4893-4966, for single-scan sequential files -- an interleaved scan of all components, or a one-component file, which is planned as
 * mcuh x mcuv = its nch x ncv blocks with hs = vs = 1 and block rows bch apart): one wavefront per image decodes the un-stuffed scan into
 * the zero-filled device frame images[i].blocks and writes images[i].mcuv + 1 records (bit position + last DC per MCU row,
 * final record: pad-bit pattern and status) at d_rows + images[i].rows_off.  lep_jpeg_open_gpu fills the struct. */
#define LEP_HUFFDEC_EARLY_EOF 1          /* lep_huffdec_image.flags */
#define LEP_HUFFDEC_RST_TABLE 2          /* ... a scan with restart intervals whose markers all stand where they should: their positions (uint32
                                            offsets into the un-stuffed scan, (mcuc - 1) / rsti of them) follow the scan bytes at
                                            scan + LEP_HUFFDEC_SCAN_ROOM(scan_len); every interval is then decoded by a lane of its own */
#define LEP_HUFFDEC_SCAN_ROOM(scan_len) ((((size_t)(scan_len)) + 64 + 15) & ~(size_t)15)   /* scan bytes + zero padding, 16-byte multiple */
#define LEP_HUFFDEC_ROW_TRUNCATED 0x40000000   /* final lep_huffdec_row.aux: the scan stopped in mid-image; .bitpos = blocks decoded (scan order) */
typedef struct lep_huffdec_image {
    const uint8_t *scan;                 /* device: un-stuffed scan bytes, 16-byte aligned, followed by >= 32 zero bytes */
    uint32_t scan_len;
    int32_t ncomp, mcuh, mcuv, mcuc, rsti;
    int32_t flags;                       /* LEP_HUFFDEC_EARLY_EOF: the file ends inside its scan (no EOI): the scan may stop in mid-image */
    int32_t first_mcu_row;               /* > 0: blocks of the MCU rows in front of it are decoded (records, status, DC chain) but not stored: their part of the
                                          * frame stays zero.  One-component images: block rows (the planned mcuv).  0 = the whole frame */
    int32_t hs[4], vs[4], bch[4], dc_tbl[4], ac_tbl[4], scan_cmp[4];
    int16_t *blocks[4];                  /* device: zero-filled coefficient frame */
    uint64_t rows_off;
    uint16_t lut[4][512];
    int32_t maxcode[4][8], valoff[4][8];   /* codes of 9..16 bits: largest code per length (-1 none), symbol index - code */
    uint8_t longsym[4][256];               /* their symbols in canonical order */
} lep_huffdec_image;
typedef struct lep_huffdec_row {
    uint32_t bitpos;
    int16_t last_dc[4];
    int32_t aux;
} lep_huffdec_row;
int lep_gpu_huffman_decode_device(lep_gpu *g, const lep_huffdec_image *images, int nimg, lep_huffdec_row *d_rows, void *hip_stream);
/* The same for PROGRESSIVE files (replaces the progressive branches of decode_jpeg's scan loop, src/lepton/jpgcoder.cc:2975-3260,
 * with decode_dc_prg_*, decode_ac_prg_fs / _sa, decode_eobrun_sa, skip_eobrun :4968-5335, :5462-5500): one wavefront per
 * (image, scan) whose 64 lanes decode the codes that would start at the next 64 bits while the scalar unit hops from code to
 * code (lep_huffprogdec_win.h; scans with restart intervals: one wavefront per piece of consecutive intervals where the descriptor carries
 * LEP_HUFFDEC_RST_TABLE, lep_huffprogdec_rst.h -- uniform vector code otherwise, lep_huffprogdec.h).  A refinement scan must see what the earlier scans of its band wrote, so every descriptor carries a
 * dependency `level`.  Up to 16384 scans go out as ONE launch, ordered by level, in which a scan waits -- MCU row by MCU row,
 * on a progress word the scans in front of it publish -- for the scans of its file (same frame pointers) whose component and
 * band meet its own: a file then takes as long as its longest scan instead of the sum over its levels.  Larger calls (or
 * LEP_HUFFPROG_PIPELINE=0) launch level after level on the stream.  Each scan writes its coefficients into the
 * zero-filled frame t.blocks, the first scan of a file also one record per MCU row at d_rows + t.rows_off, and every scan a
 * final record {bits consumed, last DC, pad bits | status << 8} at d_rows + result_off; a non-zero status anywhere sends the
 * whole file to the host parser.  lep_jpeg_open_gpu_progressive fills the descriptors.
 * A file that ENDS INSIDE A SCAN (no EOI): its last descriptor, and no other, carries LEP_HUFFDEC_EARLY_EOF in t.flags.  That scan is
 * decoded up to the block that reads the data's last bit -- every bit at or behind t.scan_len * 8 is zero by position, whatever the slot
 * holds there -- and its final record says LEP_HUFFDEC_ROW_TRUNCATED, .bitpos = the blocks of the scan's order up to and including that
 * one (a one-component scan: the position the block started at, + 1).  A block that meets the end and does not decode is a status like
 * any other.  Only lep_huffprogdec_win.h knows the cut: a flagged scan that form does not take (a restart interval, a slot that is not
 * 16-byte aligned, LEP_HUFFPROGDEC_WIN=0) goes to no kernel, its final record is filled with 0x80 bytes, the file goes to the host parser.
 * LEP_HUFFDEC_RST_TABLE in t.flags is the contract the sequential side has: a caller that passes a descriptor with the flag HAS PUT the
 * scan's marker positions (lep_jpeg_scan_restarts_of: uint32 offsets into this scan's un-stuffed bytes) behind the scan's slot, at
 * t.scan + LEP_HUFFPROGDEC_SCAN_ROOM(t.scan_len); a caller that has not put them there CLEARS the flag, and the scan goes to
 * lep_huffprogdec.h.  The scans of a file with at least one such scan are launched level after level (none of them waits on a
 * progress word); LEP_HUFFPROGDEC_RST=0 sends them to lep_huffprogdec.h whatever the flag says. */
#define LEP_HUFFPROGDEC_SCAN_ROOM(scan_len) ((((size_t)(scan_len)) + 80 + 15) & ~(size_t)15)   /* a progressive scan's slot: bytes + zero padding, 16-byte multiple */
typedef struct lep_huffprogdec_scan {
    lep_huffdec_image t;                 /* scan = this scan's bytes; lut[0..1] DC tables 0 / 1, lut[2] the scan's AC table */
    int32_t cmpc, cmp[4];
    int32_t from, to, sah, sal;
    int32_t bcv[4], nch[4], ncv[4], mbs[4];
    int32_t tbl[4];
    int32_t max_eobrun;
    int32_t want_rows;
    int32_t level;
    int32_t pad;
    uint64_t result_off;
} lep_huffprogdec_scan;
int lep_gpu_huffman_progressive_decode_device(lep_gpu *g, const lep_huffprogdec_scan *scans, int nscan, lep_huffdec_row *d_rows, void *hip_stream);
/* The same result with one LANE per subsequence (lep_huffdec_simt.h; the batch compressor's default): a scan is cut into thousands of subsequences, every lane decodes one with a
 * bit reader of its own -- a guess from its first bit, settle passes from where the lane in front ended until no end state moves,
 * a prefix sum, a write pass into the ZERO-FILLED frame.  Same records, same frame, same status semantics as the single-wave
 * kernel (bit-exact against it on MI355X and in the lane-loop emulation); scans with restart intervals are taken when the image
 * carries LEP_HUFFDEC_RST_TABLE (lane = restart interval) and refused otherwise (LEP_ASSERTION_FAILURE: the single-wave kernel's).
 * Scans whose blocks all use one DC and one AC table -- the bits do not say which block of the MCU a lane stands on -- are settled
 * through DC sums per MCU slot, for 2 .. 16 blocks per MCU (4:2:0 with one table pair is six): status 0 like any other whole scan.
 * LEP_HUFFDEC_SIMT_BITS forces the subsequence length (tests). */
int lep_gpu_huffman_decode_simt_device(lep_gpu *g, const lep_huffdec_image *images, int nimg, lep_huffdec_row *d_rows, void *hip_stream);
/* plain device memory helpers so non-torch callers need no HIP binding */
/* Device self-test of kernel arithmetic that has no CPU twin (exhaustive: the float-reciprocal Branch probability of the
 * kernels against integer division, src/vp8/model/branch.hh:82-125).  0 = exact everywhere. */
int lep_gpu_selftest(lep_gpu *g);
/* Gives back the device memory the object caches between launches (per-segment models, neighbour rings, the split-phase
 * encoder's scratch: ~140 MB per 4K image of the largest launch so far) -- to the object's own POOL: the workspaces are virtual
 * address ranges into which 512 MB chunks are mapped, a trimmed workspace is unmapped and its chunks wait for the next workspace that
 * grows (of whatever kind).  Cheap in both directions (96 GB: 19 ms to unmap, 14 ms to map again) -- what is NOT cheap is taking
 * memory from the driver, which clears it: ~40 ms per GB (hipMalloc of 96 GB: 3 - 4 s); round 3 measured that as "memory serves
 * the kernels slower after a trim".  Waits for the device. */
int lep_gpu_trim(lep_gpu *g);
/* lep_gpu_trim, and the pool handed to the driver: for a process that wants the device's memory for something else.  (The
 * library does this itself before it reports an allocation failure of its staging.) */
int lep_gpu_release_memory(lep_gpu *g);
/* Profiling builds (-DLEP_PROF) only: per-phase shader-clock totals [64 segments][32 slots] of the last decoder launch. */
int lep_gpu_debug_prof(lep_gpu *g, uint64_t *out);
int lep_gpu_malloc(lep_gpu *g, size_t bytes, void **dptr);
int lep_gpu_free(lep_gpu *g, void *dptr);
int lep_gpu_memcpy_h2d(lep_gpu *g, void *dst, const void *src, size_t bytes);
int lep_gpu_memcpy_d2h(lep_gpu *g, void *dst, const void *src, size_t bytes);
int lep_gpu_memcpy_d2d(lep_gpu *g, void *dst, const void *src, size_t bytes);
int lep_gpu_memset(lep_gpu *g, void *dst, int value, size_t bytes);

/* ---- layer 2: host-side callers of the hot path --------------------------------------------- */
typedef struct lep_jpeg lep_jpeg;   /* a parsed JPEG: header bytes, coefficient frame, row hand-offs */
typedef struct lep_file lep_file;   /* a parsed .lep: header sections, hand-offs, de-muxed streams */

/* JPEG -> coefficient frame (read_jpeg + decode_jpeg, src/lepton/jpgcoder.cc:2269-2466, 2799-3302) */
int lep_jpeg_open(const uint8_t *jpg, size_t len, int allow_progressive, lep_jpeg **out);
/* the same, with the coefficient frame decoded straight into caller-provided memory (frame_cap bytes, planes back to back,
 * e.g. pinned staging memory): no allocation, page faults or later copy; falls back to owned storage when it is too small */
int lep_jpeg_open_into(const uint8_t *jpg, size_t len, int allow_progressive, void *frame_mem, size_t frame_cap, lep_jpeg **out);
/* frame size from the SOF marker alone (no scan decode) */
int lep_jpeg_peek_frame_bytes(const uint8_t *jpg, size_t len, size_t *bytes);
/* JPEG parse with the scan decode left to lep_gpu_huffman_decode_device: splits the file and reads the tables only.
 * *eligible = 0: the file needs the host decoder (call lep_jpeg_open / lep_jpeg_open_into instead).  Otherwise *image is
 * filled except for scan / blocks / rows_off (device addresses, the caller's), lep_jpeg_scan_bytes gives the bytes to
 * upload, and lep_jpeg_finish_gpu turns the kernel's row records into hand-offs (non-zero: irregular scan, use the host). */
int lep_jpeg_open_gpu(const uint8_t *jpg, size_t len, lep_jpeg **out, lep_huffdec_image *image, int *eligible);
/* the parse behind lep_compress_slice: len already bounded by -trunc; lep_jpeg_plan / lep_jpeg_write_lep then produce the 'Y' file */
int lep_jpeg_open_slice(const uint8_t *jpg, size_t len, size_t start_byte, lep_jpeg **out);
/* `lepton -embedding=<offset>` (jpgcoder.cc:1135-1137, 2275-2282; test_suite/test_embedded.sh): a JPEG that sits `offset` bytes
 * into a larger blob; the .lep ('PGE' section + ordinary garbage) restores the whole blob */
int lep_jpeg_open_embedded(const uint8_t *blob, size_t len, size_t offset, lep_jpeg **out);
int lep_compress_embedded(lep_gpu *g, const uint8_t *blob, size_t len, size_t offset, lep_bytes *out);
/* progressive files, and sequential frames coded in several scans (their scans: from 0 / to 63, t = the frame with all four tables,
 * a record per MCU row of the scan's own geometry; lep_gpu_huffman_progressive_decode_device hands them to the sequential scan decoders):
 * after lep_jpeg_open_gpu answered *eligible = 0.  Fills up to `cap` scan descriptors (t.scan = byte offset of
 * the scan inside lep_jpeg_scan_bytes, t.rows_off / result_off relative to the file's first record -- the caller adds its arena
 * offsets and sets t.blocks); *rows_needed = records the file needs in the row arena.  _finish turns the kernels' records into
 * the hand-offs and bookkeeping of the .lep header (non-zero: irregular, use the host parser).
 * A file that ends inside a scan: *eligible = 0, as ever.  lep_jpeg_open_gpu_progressive_cut takes PROGRESSIVE files of that kind too,
 * their last scan flagged LEP_HUFFDEC_EARLY_EOF -- unless a scan of the file has a restart interval or the last scan holds no byte of
 * data (cut sequential frames in several scans stay with the host parser): for a caller that launches the descriptors through
 * lep_gpu_huffman_progressive_decode_device, which knows the flag.  lep_compress_batch is that caller. */
int lep_jpeg_open_gpu_progressive(lep_jpeg *j, lep_huffprogdec_scan *scans, int cap, int *nscan, int *rows_needed, int *eligible);
int lep_jpeg_open_gpu_progressive_cut(lep_jpeg *j, lep_huffprogdec_scan *scans, int cap, int *nscan, int *rows_needed, int *eligible);
int lep_jpeg_finish_gpu_progressive(lep_jpeg *j, const lep_huffprogdec_scan *scans, int nscan, const lep_huffdec_row *rows);
/* The Huffman half of the round-trip check (validation.cc:97-218) for a file whose scans lep_jpeg_open_gpu_progressive took:
 * the plan that writes every scan of the parsed file again on the GPU (lep_gpu_huffman_progressive_encode_device; the caller
 * sets image->blocks, out_off, corr_off) and where each scan's own bytes lie in the file (first byte, length -- up to the
 * marker that ends the scan), to be compared with what the kernel wrote.  *eligible = 0: check on the host instead.
 * A file that ends inside a scan: *eligible = 0.  lep_jpeg_plan_progressive_check_cut plans those too: the length of the scan the file
 * ends in is what the file kept of it less the file's last two bytes (which the container stores as they are); the kernel writes that
 * scan whole -- its out_cap is its geometry's -- and its FIRST file_len bytes are the ones to compare. */
int lep_jpeg_plan_progressive_check(lep_jpeg *j, size_t jpeg_len, lep_huffprog_image *image, lep_huffprog_scan *scans,
                                    uint32_t *file_first, uint32_t *file_len, int cap, int *nscan, int *eligible);
int lep_jpeg_plan_progressive_check_cut(lep_jpeg *j, size_t jpeg_len, lep_huffprog_image *image, lep_huffprog_scan *scans,
                                        uint32_t *file_first, uint32_t *file_len, int cap, int *nscan, int *eligible);
int lep_jpeg_scan_bytes(const lep_jpeg *j, const uint8_t **data, size_t *len);
/* The restart markers of a file lep_jpeg_open_gpu flagged LEP_HUFFDEC_RST_TABLE: the offset in the un-stuffed scan bytes at which
 * each stood.  The caller puts them, as uint32, at scan + LEP_HUFFDEC_SCAN_ROOM(scan_len) on the device. */
int lep_jpeg_scan_restarts(const lep_jpeg *j, const uint32_t **pos, size_t *count);
/* The same for scan `scan_index` of the file (0 = the first; what lep_jpeg_open_gpu_progressive's descriptors are indexed by): offsets
 * relative to THAT scan's first un-stuffed byte.  For a scan flagged LEP_HUFFDEC_RST_TABLE there are (units - 1) / rsti of them, units =
 * MCUs of an interleaved scan, the component's nch x ncv blocks of a one-component scan. */
int lep_jpeg_scan_restarts_of(const lep_jpeg *j, int scan_index, const uint32_t **pos, size_t *count);
int lep_jpeg_finish_gpu(lep_jpeg *j, const lep_huffdec_row *rows);
void lep_jpeg_close(lep_jpeg *j);
int lep_jpeg_describe(const lep_jpeg *j, lep_image_desc *desc);          /* host pointers into j */
int lep_jpeg_is_progressive(const lep_jpeg *j);   /* 1: not a single interleaved sequential scan (needs the progressive re-coder) */
/* A file that ends inside its scan, parsed by the host parser (lep_jpeg_open and its kin): 1 when the block that met the end of the data had
 * failed to decode -- bits that are no code, a run that leaves its band -- and was kept all the same, as the reference keeps it; 0 otherwise,
 * and for every file a GPU scan decoder finished.  Those decoders leave exactly such files to the host parser. */
int lep_jpeg_cut_block_irregular(const lep_jpeg *j);
/* segment choice of write_ujpg (src/lepton/jpgcoder.cc:3856-3934); returns count, fills segs */
int lep_jpeg_plan(const lep_jpeg *j, int max_threads, lep_segment *segs, int image_index);
/* -maxencodethreads / -minencodethreads / -evensplit (jpgcoder.cc:1064-1095): they change how many thread segments a file gets
 * and where they are cut, i.e. the .lep bytes; 0 / 0 / 0 leaves the reference's defaults (8, 1, by compressed size) */
int lep_jpeg_set_encode_options(lep_jpeg *j, int max_threads, int min_threads, int even_split);
/* `lepton -brotliheader` (src/lepton/jpgcoder.cc:1116-1119, 4038): container format version 2 -- the header is a brotli stream
 * (BrotliCodec::Compress, src/io/BrotliCompression.cc:45-98, with the vendored brotli 1.0.0 encoder: compiled into the library from
 * the reference's dependency tree when build() finds it) and the packets end with FF FE FF.  1 = the default (zlib).  Returns
 * LEP_VERSION_UNSUPPORTED for a version this build cannot write; lep_container_can_write_version asks without a file. */
int lep_jpeg_set_container_version(lep_jpeg *j, int version);
int lep_container_can_write_version(int version);
/* whole .lep file from the per-segment streams (header + mux + trailer) */
int lep_jpeg_write_lep(const lep_jpeg *j, int max_threads, const lep_bytes *streams, int nstreams, lep_bytes *out);
/* The Huffman half of the reference's default round-trip check (src/lepton/validation.cc:97-218; `lepton` without
 * -skipverify exits with ROUNDTRIP_FAILURE when the file it would restore differs from its input): parses `lepdata` (what
 * lep_jpeg_write_lep just produced), re-codes j's own coefficient frame with the .lep's header, and compares the result
 * with `want` (the whole input; for a slice the bytes [start_byte, trunc); for an embedded JPEG the whole blob).  Host
 * only.  The arithmetic-coder half (streams -> the same coefficients) is lep_batch_options.verify's on-GPU comparison.
 * Returns 0, LEP_ROUNDTRIP_FAILURE, or the exit code of a .lep that does not parse.  Files the reference itself cannot
 * restore -- e.g. a one-component frame with sampling factors 2x2, restart markers and more than one MCU row -- end here. */
int lep_jpeg_check_restores(const lep_jpeg *j, const uint8_t *lepdata, size_t lep_len, const uint8_t *want, size_t want_len);

/* .lep -> streams + frame geometry (read_ujpg, src/lepton/jpgcoder.cc:4117-4362) */
int lep_file_open(const uint8_t *lepdata, size_t len, lep_file **out);
/* Format versions >= 2 (brotli header, `lepton -brotliheader`) mark the end of their packets, so several files may follow
 * each other in one stream and restore the concatenation of their JPEGs (jpgcoder.cc:1868-1897): lep_file_consumed = bytes
 * the parsed file occupies; lep_chained_file_follows = another file's magic stands behind them; lep_file_open_next parses
 * it, handing over what `prev` left in the shared header reader (the "CNT" sections `lepton -lepcat` writes,
 * concat.cc:84-95).  lep_decompress walks such streams itself. */
size_t lep_file_consumed(const lep_file *f);
int lep_chained_file_follows(const uint8_t *lepdata, size_t len, size_t consumed);
int lep_file_open_next(const uint8_t *lepdata, size_t len, const lep_file *prev, lep_file **out);
void lep_file_close(lep_file *f);
int lep_file_describe(lep_file *f, lep_image_desc *desc);                /* allocates zeroed host frame */
int lep_file_describe_into(lep_file *f, void *frame_mem, size_t frame_cap, lep_image_desc *desc);   /* frame in caller memory; (NULL, (size_t)-1) = geometry only */
int lep_file_segments(const lep_file *f, lep_segment *segs, lep_bytes *streams, int image_index);
uint32_t lep_file_jpeg_size(const lep_file *f);
size_t lep_file_frame_bytes(const lep_file *f);   /* bytes of the coefficient frame lep_file_describe will expose */
/* coefficient frame -> original JPEG bytes (recode_baseline_jpeg, src/lepton/recoder.cc:694-889) */
int lep_file_recode(lep_file *f, lep_bytes *out);
/* The same with the Huffman coding done by lep_gpu_huffman_encode_device: _plan walks the header and, if the file is
 * eligible (*gpu_ok = 1), fills the image / per-segment parameters (blocks[], image index and out_off are the caller's to
 * set; out_cap is the segment's byte bound); _finish glues header, the segments' scan bytes and the trailer together. */
int lep_file_recode_plan(lep_file *f, lep_huff_image *image, lep_huff_segment *segs, int *nseg, int *gpu_ok);
/* after _plan: the bytes in front of the scan, as _finish will write them (they stay the file's) */
int lep_file_recode_head(const lep_file *f, const uint8_t **data, size_t *len);
/* ends: the kernel's per-segment end states (NULL: only the byte counts are held against the hand-offs) */
int lep_file_recode_finish(lep_file *f, const lep_bytes *seg_bytes, const lep_huff_end *ends, int nseg, lep_bytes *out);
/* The same checks and the same tail one by one, for a caller that kept a segment's end state and byte count but not its bytes (a range
 * read).  _segment_end: segment q ran to its end in state *end with `bytes` bytes; last_given != 0: it is the last one of the file.
 * 0, LEP_GPU_PATH_DECLINED (what the writer said about a cut: the host re-coder decides) or LEP_ASSERTION_FAILURE (partial byte, bit
 * count, last DCs or byte count are not what hand-off q + 1 recorded).  _tail: what the finish writes behind the last segment's bytes
 * (misplaced restart markers, the rest of the header, the garbage) when bytes_in_front bytes stand in front of it; *first (may be
 * NULL) is where it starts: bytes_in_front, or the bound in front of the garbage where that is less.  Both need the plan. */
int lep_file_recode_segment_end(lep_file *f, int q, const lep_huff_end *end, uint64_t bytes, int last_given);
int lep_file_recode_tail(lep_file *f, uint64_t bytes_in_front, lep_bytes *out, uint64_t *first);
/* progressive files: _plan fills the image and up to `cap` scan descriptors (out_cap / corr_cap = what each scan may need;
 * image index, out_off, corr_off and blocks[] are the caller's to set); *gpu_ok = 0: the file keeps the host re-coder
 * (truncated, withheld restart markers ...).  SEQUENTIAL frames coded in several scans are planned here too: their scans have
 * from 0 / to 63 (no progressive scan has), all four tables in code[] and the components' choice of them in tbl[], and
 * lep_gpu_huffman_progressive_encode_device hands them to the sequential scan encoders.  _finish glues header pieces, scans and trailer. */
/* Compression with verification, baseline files: the plan that writes the parsed file's scan again on the GPU from its coefficient frame
 * (lep_gpu_huffman_encode_device; images[].blocks and the segments' out_off are the caller's to set) and, per thread segment, the
 * bytes of the file it must reproduce -- the Huffman half of the reference's round-trip check (src/lepton/validation.cc:97-218),
 * executed, not argued.  *eligible = 0: the file keeps the host check (lep_jpeg_check_restores).
 * NOT a read-only call: the parsed file is lent to the plan for its duration (the tables in front of the scan are read again from the
 * header bytes, a warning level may be set) -- the handle must not be used from another thread while it runs. */
int lep_jpeg_plan_scan_check(lep_jpeg *j, size_t jpeg_len, lep_huff_image *image, lep_huff_segment *segs, uint32_t *file_first, uint32_t *file_len, int cap,
                             int *nseg, int *eligible);
int lep_jpeg_scan_file_range(const lep_jpeg *j, uint32_t *first, uint32_t *len);
int lep_file_recode_plan_progressive(lep_file *f, lep_huffprog_image *image, lep_huffprog_scan *scans, int cap, int *nscan, int *gpu_ok);
/* The same, and progressive files that END INSIDE A SCAN too (the plain entry answers *gpu_ok = 0 for those, as it always has): for a caller
 * that sizes its slots by the descriptors' out_cap / file_bound -- the cut scan's are its geometry's, not the file's -- and clears the frame
 * behind coded_blocks of a file of one thread segment (lep_huffprog_image, above).  lep_decompress_batch is that caller. */
int lep_file_recode_plan_progressive_cut(lep_file *f, lep_huffprog_image *image, lep_huffprog_scan *scans, int cap, int *nscan, int *gpu_ok);
int lep_file_recode_finish_progressive(lep_file *f, const lep_bytes *scan_bytes, int nscan, lep_bytes *out);


/* .lep framing pieces, exposed for callers that assemble containers themselves */
typedef struct lep_handoff {           /* ThreadHandoff, src/lepton/thread_handoff.hh:8-39 */
    uint16_t luma_y_start, luma_y_end;
    uint32_t segment_size;
    uint8_t overhang_byte, num_overhang_bits;
    int16_t last_dc[4];
} lep_handoff;
/* 'H', n, then n 16-byte records (ThreadHandoff::serialize / deserialize, thread_handoff.cc:4-76) */
int lep_handoffs_serialize(const lep_handoff *h, int n, uint8_t *out, size_t out_cap);
int lep_handoffs_parse(const uint8_t *data, size_t len, lep_handoff *out, int out_cap);
/* lep_jpeg_plan's choice as hand-off records (what write_ujpg serialises into the header, jpgcoder.cc:3873-3934):
 * segment_size = the JPEG scan bytes each thread segment covers.  Returns the count, or -LEP_BUFFER_TOO_SMALL. */
int lep_jpeg_plan_handoffs(const lep_jpeg *j, int max_threads, lep_handoff *out, int cap);
/* MuxWriter policy (src/io/MuxReader.hh:336-522) fed in the encoder's slice order (vp8_encoder.cc:575-594) */
int lep_mux(const lep_bytes *streams, int nstreams, int version, lep_bytes *out);
/* MuxReader (src/io/MuxReader.hh:230-283): packets until the data runs out; streams[16] are malloc'd */
int lep_demux(const uint8_t *data, size_t len, lep_bytes *streams16);

/* ---- layer 3: whole files ------------------------------------------------------------------- */
int lep_compress(lep_gpu *g, const uint8_t *jpg, size_t len, lep_bytes *out);
/* `lepton -startbyte=<start_byte> -trunc=<trunc>` (jpgcoder.cc:1132-1140, 3801-3843; test_suite/test_2nd_block.sh): the .lep
 * restores bytes [start_byte, trunc) of the JPEG (trunc 0 = to the end) -- how a JPEG stored as fixed-size blocks is
 * compressed block by block.  Format flag 'Y': header segments reduced to the ones the scan needs, hand-off rows in front of
 * start_byte dropped, the bytes up to the first remaining MCU row kept verbatim.  lep_decompress reads such files like any
 * other.  Progressive files cannot be sliced (PROGRESSIVE_UNSUPPORTED), as in the reference.
 * One file per call, on the host parser; lep_compress_batch_slices takes many slices through the batch pipeline and gives the same bytes. */
int lep_compress_slice(lep_gpu *g, const uint8_t *jpg, size_t len, size_t start_byte, size_t trunc, lep_bytes *out);
int lep_decompress(lep_gpu *g, const uint8_t *lepdata, size_t len, lep_bytes *out);
/* .lep -> 8-bit sample planes: parse, decode on the device, lep_gpu_samples_device, the planes copied down -- no scan is written and no
 * JPEG byte crosses PCIe.  Takes every file lep_decompress takes (baseline, progressive, truncated, -startbyte / -trunc slices, embedded
 * files; of a chained stream the first file) and returns its codes for a file that does not parse or a stream that does not decode.
 * Blocks the file never coded -- the tail of a truncated file, the rows in front of a slice -- are zero in the frame and come out as 128.
 * scale: 1 or 8 (anything else: LEP_ASSERTION_FAILURE).  The planes are the components' block grids, not cropped to width x height. */
typedef struct lep_planes {
    int32_t width, height, ncomp, scale;          /* the image's size in pixels, as its frame header says */
    int32_t h_samp[3], v_samp[3];                 /* sampling factors */
    int32_t plane_width[3], plane_height[3], pitch[3];   /* samples stored: the block grid, not cropped */
    uint8_t *plane[3];                            /* one allocation; lep_free(plane[0]) */
} lep_planes;
int lep_decompress_planes(lep_gpu *g, const uint8_t *lepdata, size_t len, int scale, lep_planes *out);
/* .lep -> pixels: lep_decompress_planes's front at scale 1 (the same files, the same codes for a file that does not parse or a stream
 * that does not decode), then lep_gpu_rgb_device on the planes where they lie; only the pixels are copied down.  Blocks the file never
 * coded come out as the definition makes of 128-valued samples.  Which three-component files are converted from YCbCr is libjpeg's
 * rule, read from the file's header segments and component ids: a JFIF APP0 ("JFIF\0", 14 bytes of data or more) means YCbCr; else an
 * Adobe APP14 ("Adobe", 12 bytes or more) with transform byte 0 means R, G, B as they are, any other transform YCbCr; else the
 * component ids 'R', 'G', 'B' mean as they are; else YCbCr.  One component gives one byte per pixel.  LEP_UNSUPPORTED_JPEG with a
 * lep_gpu_last_error text, nothing launched for the pixels: two components, sampling factors that are no integral multiples. */
typedef struct lep_rgb {
    int32_t width, height, channels, pitch;       /* channels: 1 or 3; pitch = width * channels */
    uint8_t *pixels;                              /* one allocation; lep_free(pixels) */
} lep_rgb;
int lep_decompress_rgb(lep_gpu *g, const uint8_t *lepdata, size_t len, lep_rgb *out);
/* lep_decompress with the JPEG's bytes handed to `sink` as they become final, in file order.  Every single file the split re-coder plans
 * (lep_file_recode_plan says gpu_ok: a baseline file or a -startbyte / -trunc slice of one, 'Z' or 'Y', one scan of one, two or three
 * components, cut inside that scan or not, with or without restart intervals; lep_file_streams_in_session answers for a file)
 * is decoded in a session (lep_gpu_decode_rows_*), band_mcu_rows MCU rows per advance (<= 0: one advance): the header (a slice's prefix
 * bytes) goes out before
 * the first advance, then after every advance the MCU rows that have become complete are Huffman-coded on the host, segment by segment
 * from each segment's hand-off; segment 0's rows go out as they come, a later segment's bytes once the segments in front of it are done.
 * Every other file (progressive, sequential in several scans, cut with restart intervals, several files back to back, ...) is
 * lep_decompress and one sink call: stats->advances = 0.
 * The bytes sunk, concatenated, are lep_decompress's and the return value is the same; when a segment fails, what has been sunk by
 * then are bytes of rows in front of the failing block.  A sink that returns non-zero ends the call with LEP_OS_ERROR.  stats may be NULL. */
typedef int (*lep_sink)(void *user, const uint8_t *data, size_t len);
typedef struct lep_stream_stats {
    int32_t advances;                          /* lep_gpu_decode_rows_advance calls made */
    int32_t advances_before_first_scan_byte;   /* ... of them before the first byte of the scan reached the sink */
    uint64_t bytes_before_last_advance;        /* bytes the sink had when the last advance was launched */
} lep_stream_stats;
int lep_decompress_stream(lep_gpu *g, const uint8_t *lepdata, size_t len, int band_mcu_rows, lep_sink sink, void *user, lep_stream_stats *stats);
/* Host only: does lep_decompress_stream / lep_decompress_batch_stream decode this .lep in a session?  1 / 0, or the exit code (> 1) of a
 * file that does not parse.  (A parse that ends in LEP_ASSERTION_FAILURE, which is 1, answers 0: the file is not streamed.) */
int lep_file_streams_in_session(const uint8_t *lepdata, size_t len);
/* Host only: where the bytes [first, first + length) of the restored file lie.  A file that is decoded in a session is its head (what
 * stands in front of the scan; of a -startbyte / -trunc file, which counts in its own bytes, the prefix garbage), one extent per thread
 * segment and the tail (misplaced restart markers, the rest of the header, the garbage).  Every segment but the last writes exactly the
 * segment_size its hand-off records -- the finish holds it to that --, so seg_first[] and every seg_len[] but the last are the header's
 * (sizes_known = 0: a hand-off whose size the finish does not hold, or cannot be met; the extents are then a guess).  The last
 * segment's seg_len is "to the tail": right when the file has jpeg_size bytes and no bound cuts its tail, which the header does not
 * prove (last_len_known = 0, always); the segment's true end is found by decoding it.
 * length == 0: to the end.  The range is clipped to jpeg_size (`first`, `length` say how); first >= jpeg_size is an empty answer:
 * length 0, no segment, return value 0.  first_seg / last_seg: the segments the range touches (-1: none); win_skip / win_take: per
 * touched segment the window, from the segment's first byte -- the last segment's window is open to where the garbage starts (scan_bound),
 * its take may outlast the segment, and reaches_last says that the range reaches behind the last segment's start: that segment is then
 * touched even by a range that lies in the tail (win_take 0) and must be decoded, to its end when the window outlasts it.  A file that is not decoded in a session (in_session = 0: progressive, several scans, chained, ...)
 * has nseg = 0 and no extents; jpeg_size and the clipped range are filled.  Returns 0, or the exit code of a file that does not parse. */
typedef struct lep_range_plan {
    int32_t  in_session;                 /* what lep_file_streams_in_session answers */
    int32_t  nseg;
    uint64_t jpeg_size, head_len;
    uint64_t seg_first[16], seg_len[16];
    int32_t  sizes_known, last_len_known;
    uint64_t tail_len;                   /* the tail where no bound cuts it */
    uint64_t scan_bound;                 /* bytes the file may hold in front of its trailing garbage */
    uint64_t first, length;              /* the range, clipped */
    uint64_t head_bytes;                 /* bytes of the head it holds */
    int32_t  first_seg, last_seg;
    uint64_t win_skip[16], win_take[16];
    int32_t  reaches_last, pad;
} lep_range_plan;
int lep_file_range_plan(const uint8_t *lepdata, size_t len, uint64_t first, uint64_t length, lep_range_plan *out);

/* Whole batches of files as a pipeline (what `lepton -socket` workers / src/lepton/socket_serve.cc:312-390 would hand to
 * the GPU): JPEG parsing + Huffman scan decode on a host thread pool, coefficient frames over PCIe on a copy stream while
 * the previous chunk's coder kernels run, streams back, .lep containers written on the host pool -- and the mirror image
 * for decompression.  verify != 0 restores the reference's default round-trip check (src/lepton/validation.cc:97-218) on
 * the GPU: what was just encoded is decoded into a scratch frame and compared with the input frame before the .lep is
 * released; a mismatch gives that file status LEP_ROUNDTRIP_FAILURE.
 * status[i] = exit code of file i (0 = ok, outs[i] is malloc'd: release with lep_free); the return value is non-zero only
 * for failures of the machinery itself (LEP_GPU_ERROR). */
typedef struct lep_batch_options {
    int32_t host_threads;        /* 0 = the CPUs this process may use (affinity mask capped by the cgroup CPU quota) */
    int32_t verify;              /* compress: on-GPU round-trip verification */
    size_t chunk_frame_bytes;    /* cap on coefficient-frame bytes per pipeline chunk; 0 = 32 GiB (1024 4K frames) */
    int32_t host_huffman;        /* 1 = JPEG Huffman decode / re-encode on the host pool (frames cross PCIe) instead of on the GPU */
    int32_t chunk_images;        /* images per pipeline chunk; 0 = automatic: at most 1024 images and 8192 thread segments (the decoder
                                    wavefronts the chip holds at once), chunks of a call balanced.  The decode kernel takes as
                                    long for 100 segments as for 8192, so chunks must be this big */
    int32_t overlap_launches;    /* compress: consecutive chunks' coder kernels on two streams / two workspace sets (experimental; also
                                    LEP_BATCH_OVERLAP=1) */
} lep_batch_options;
typedef struct lep_batch_stats {
    double wall_s;               /* whole call */
    double pipeline_s;           /* first upload .. last container (excludes stream / buffer creation and the first parse) */
    double parse_s, stage_s, write_s;   /* host pool: parse, copies into pinned staging, container / Huffman re-code (summed) */
    double h2d_bytes, d2h_bytes; /* PCIe traffic */
    double alloc_s;              /* inside pipeline_s: (re)allocation of the pinned / device staging buffers (kept between calls) */
    double redone_files;         /* compress: files whose streams outgrew the space reserved from their JPEG size and went through lep_compress */
    double gpu_huffman_files;    /* files whose Huffman scans the GPU decoded (compress) / wrote (decompress); the rest took the host coder */
    double gpu_verified_scans;   /* compress with verify: thread segments (baseline) and scans (progressive) written again on the GPU from the
                                    device frame and compared with the file's own bytes -- the Huffman half of the round-trip check */
} lep_batch_stats;
int lep_compress_batch(lep_gpu *g, const lep_bytes *jpgs, int n, lep_bytes *outs, int32_t *status,
                       const lep_batch_options *opt, lep_batch_stats *stats);
/* The same pipeline for `-startbyte / -trunc` slices: jpgs[i] is the file from its first byte, slices[i] what lep_compress_slice takes as
 * start_byte / trunc ({0, 0} = the whole file; slices == NULL = lep_compress_batch).  outs[i] / status[i] are byte for byte what
 * lep_compress_slice returns for the same arguments, its refusal codes included.  Slices of the layouts the GPU scan decoder takes whole
 * are decoded there (stats->gpu_huffman_files counts them); with opt->verify their scan is written again on the GPU from the first kept
 * hand-off on and held to the file's bytes.  Everything else goes to the host parser inside the pipeline. */
typedef struct lep_slice { size_t start_byte, trunc; } lep_slice;
int lep_compress_batch_slices(lep_gpu *g, const lep_bytes *jpgs, const lep_slice *slices, int n, lep_bytes *outs, int32_t *status,
                              const lep_batch_options *opt, lep_batch_stats *stats);
int lep_decompress_batch(lep_gpu *g, const lep_bytes *leps, int n, lep_bytes *outs, int32_t *status,
                         const lep_batch_options *opt, lep_batch_stats *stats);
/* lep_decompress_batch with every file's bytes handed to `sink` as they become final.  The files lep_decompress_stream streams (every
 * single file the split re-coder plans: whole files and slices, one to three components, cut inside the scan or not; not chained) are decoded in
 * sessions (lep_gpu_decode_rows_*) of at most LEP_STREAM_SESSION_FILES files (environment, default 64) and 16384 thread segments, one session
 * after another: `begin` takes all files of a session as one launch, each file's header bytes go out before the first advance, and after
 * every advance of band_mcu_rows MCU rows (<= 0: one advance) ONE lep_gpu_huffman_encode_device launch writes the rows every segment
 * completed -- each segment from the end state of its band before, appended to its slot --, lep_gpu_pack_device moves the new bytes back to
 * back, and two copies bring them down (LEP_STREAM_PACK=0: one copy per segment).  Only scan bytes cross PCIe: frames and streams are device
 * memory of the call.  A file's front segment goes out as it comes, a later segment's bytes once the segments in front of it are complete.
 * At the end lep_file_recode_finish's checks run over the segments' bytes and end states and supply the tail; what went out must be the
 * front of that result (else LEP_ASSERTION_FAILURE).  A band of a one-component file is band_mcu_rows x (block rows per MCU row) block rows:
 * the writer's rows of such a file are block rows.  A band whose writer stops at the cut of a file cut inside its scan ends the file's last
 * segment when that segment's bytes have reached its byte bound by then (lep_file_recode_finish's condition, per band): such a file finishes
 * on the writer like any other and moves no frame.  A file whose writer outgrew its byte bound, or whose finish does not succeed (declined, or a
 * hand-off check that fails: any non-zero answer, as in lep_decompress_stream, so that exit codes stay lep_decompress's -- a check that failed on
 * good data would show only as frame_bytes_down > 0), has its frame
 * downloaded (stats->frame_bytes_down) and is finished by the host re-coder under the same check.  Every other file of the call goes through
 * ONE lep_decompress_batch call, after the sessions, and gets one sink call.
 * For every file with status[i] == 0 the pieces given to sink(user, i, ...) concatenate to what lep_decompress returns; status[i] is
 * lep_decompress's exit code.  A file that fails leaves the others untouched; what it has sunk by then are bytes of rows in front of the
 * failing block.  != 0 from the sink: that file's receiver is gone -- its remaining pieces are dropped, status[i] = LEP_OS_ERROR, the others go on.
 * Workspaces: a session holds the models, rings, descriptors and records of its arena set (coder launches and a second `begin` on that set are
 * refused); the scan writers', the scan decoders' and the pack kernels' workspaces of the same set stay usable, and this call uses them.
 * Sessions run one after another and do not overlap chunks as lep_decompress_batch does: the call buys time to first byte with throughput. */
typedef int (*lep_batch_sink)(void *user, int file, const uint8_t *data, size_t len);
typedef struct lep_batch_stream_stats {
    int32_t  files_streamed, files_whole;            /* through a session / through lep_decompress_batch, one piece */
    int32_t  sessions, advances, writer_launches;
    uint64_t scan_bytes_down, frame_bytes_down;      /* PCIe, device -> host */
    int32_t  files_first_scan_byte_before_last_advance;   /* streamed files whose first scan byte reached the sink before the last advance their
                                                             front segment took part in */
    double   wall_s, first_piece_s;                  /* first_piece_s: first piece of any file that holds scan bytes */
} lep_batch_stream_stats;
int lep_decompress_batch_stream(lep_gpu *g, const lep_bytes *leps, int n, int band_mcu_rows,
                                lep_batch_sink sink, void *user, int32_t *status,
                                const lep_batch_options *opt, lep_batch_stream_stats *stats);
/* Byte-range reads: outs[i] = the bytes [first, first + length) of what lep_decompress returns for leps[i] (length 0: to the end; clipped
 * to the file; first at or behind its end: an empty answer, status 0), restored from the thread segments the range touches and no others.
 * Thread segments are independent -- each resets its model, starts with no row above it, its scan writer starts from its own hand-off --
 * and the header says where every segment but the last starts and ends (lep_file_range_plan).  Which file goes where:
 *   - a file that is decoded in a session (lep_file_streams_in_session) whose range lies in its head is answered from the header: no
 *     segment is begun, nothing is launched (files_no_decode);
 *   - such a file whose range touches segments goes into a session with the touched segments ONLY (files_ranged; sessions of at most
 *     LEP_STREAM_SESSION_FILES files and 16384 segments).  Frames start zero-filled; rows of other segments are never read.  After every
 *     advance one scan-writer launch appends the rows every segment completed to its slot, the windowed pack brings down only the bytes
 *     inside each segment's window, and a segment whose written count has reached the end of its window is retired (in practice a file's
 *     last touched segment).  The MCU row at which a window ends is not in the file: bands find it.  band_mcu_rows > 0: bands of that
 *     height; <= 0: 1, 2, 4, ... MCU rows, doubling -- at most ceil(log2 rows) + 1 advances, fewer than twice the rows needed;
 *   - every other file (not decoded in a session; extents the header does not fix; a writer that declined or a cut the band rule does
 *     not cover, found during a session) takes ONE lep_decompress_batch call with the others of its kind and is cut on the host
 *     (files_whole): correct, not economical.
 * A touched segment that ran to its end is held to the next hand-off as the finish holds it (partial byte, bit count, last DCs, byte
 * count = segment_size: LEP_ASSERTION_FAILURE for that file); a decode that fails in a touched segment is that file's exit code; a range
 * that reaches the tail has the last segment run to its end and the tail glued behind it.  DAMAGE IN A SEGMENT THE RANGE DOES NOT TOUCH IS
 * NOT SEEN: such a range is answered with status 0 where lep_decompress fails.  Files fail alone; a file that does not parse gets
 * lep_decompress's code.  outs[i].data is malloc'd when status[i] == 0 (lep_free).  The return value is non-zero only when the machinery
 * failed.  stats may be NULL. */
typedef struct lep_range { uint64_t first, length; } lep_range;
typedef struct lep_range_stats {
    int32_t  files_ranged, files_whole, files_no_decode;   /* in sessions / through lep_decompress_batch and cut on the host / answered from the header alone */
    int32_t  sessions, advances, writer_launches;
    int32_t  segments_total, segments_begun, segments_retired;   /* thread segments of the ranged files / of them given to a session / retired */
    int64_t  mcu_rows_begun, mcu_rows_decoded;             /* planned rows of the begun segments / of them in the frame when their segment finished or was retired */
    uint64_t scan_bytes_down, frame_bytes_down;            /* PCIe, device -> host: window bytes / frames (always 0: no path of this call moves one) */
    double   wall_s;
} lep_range_stats;
int lep_decompress_batch_ranges(lep_gpu *g, const lep_bytes *leps, const lep_range *ranges, int n, int band_mcu_rows,
                                lep_bytes *outs, int32_t *status, const lep_batch_options *opt, lep_range_stats *stats);
int lep_decompress_range(lep_gpu *g, const uint8_t *lepdata, size_t len, uint64_t first, uint64_t length, lep_bytes *out);
/* the chunking lep_compress_batch will apply: file_bytes[i] / frame_bytes[i] (lep_jpeg_peek_frame_bytes; 0 = not a usable file)
 * -> chunk k holds files [chunk_first[k], chunk_first[k + 1]); returns the number of chunks (cap = entries of chunk_first) */
int lep_batch_plan(const size_t *file_bytes, const size_t *frame_bytes, int n, const lep_batch_options *opt, int *chunk_first, int cap);
/* progressive files on the GPU scan decoder: scans of its one-launch form that gave up waiting for a scan in front of them since
 * the process started (their files went to the host parser; expected 0 -- the wait cannot deadlock, the count is the safety net's) */
uint64_t lep_jpeg_gpu_scan_wait_timeouts(void);
/* sequential scans that lep_compress_batch handed to the single-wave kernel since the process started, after the lane-per-subsequence
 * decoder had answered with a status (subsequences that did not fall into step, or an irregular scan): each costs the lane passes and
 * the slowest scan decoder there is.  Whole files of every layout the parser takes are expected to count 0. */
uint64_t lep_batch_scan_second_chances(void);
void lep_batch_release(void);   /* frees the staging buffers the two calls above keep between invocations (not re-entrant) */
/* what the batch calls keep between invocations: pinned host bytes / device bytes of the large staging arenas (either pointer may be NULL) */
void lep_batch_footprint(size_t *pinned_bytes, size_t *device_bytes);
/* test hook: overwrite the pinned staging buffers kept between batch calls with `value` (stale-staging regression tests) */
void lep_batch_debug_poison(int value);
/* Test hooks for the round-trip check of lep_compress_batch with verify = 1.  A .lep is released only after three things held on the
 * device, one flag word per file: bit 0 (value 1) -- the streams decoded again into a scratch frame, and that frame differs from the
 * input frame (lep_compare_kernel); bit 1 (value 2) -- the scan written again from the frame differs from the file's own bytes
 * (lep_scan_check_bytes_kernel for a baseline file's thread segments, lep_scan_check_kernel for progressive scans); and every status
 * of the verification decode was zero.  Bit 0 or a status is LEP_ROUNDTRIP_FAILURE; bit 1 alone sends the file through the per-file path.
 * The two calls below run those kernels, with the pipeline's own launch geometry, on device buffers the caller gives (lep_gpu_malloc),
 * on the default stream, and wait for the result.
 * lep_batch_debug_compare: the first bytes / 16 units of 16 bytes of d_a and d_b (both 16-byte aligned); a difference ORs `value` into
 * *d_flag.  LEP_ASSERTION_FAILURE: a pointer that is not aligned. */
int lep_batch_debug_compare(lep_gpu *g, const void *d_a, const void *d_b, size_t bytes, uint32_t *d_flag, uint32_t value);
/* One check item: ref_len bytes of the output arena at out_off against as many of the reference arena at ref_off; item i's written
 * length is d_out_len[i].  `image` is the index of the flag word that gets bit 1.  LEP_SCAN_CHECK_PREFIX in `image` (the aligned form
 * only: the scan a file ends in, written whole): the length may exceed ref_len, bit 31 of it is not looked at, the first ref_len bytes
 * count.  Without it the length must equal ref_len, bit 31 (a writer that gave up) included. */
typedef struct lep_scan_check { uint64_t out_off, ref_off; uint32_t ref_len, image; } lep_scan_check;
#define LEP_SCAN_CHECK_PREFIX 0x80000000u
/* lep_batch_debug_scan_check: `items` is a host array of n entries.  bytes_form != 0: lep_scan_check_bytes_kernel, any alignment, no
 * prefix items; 0: lep_scan_check_kernel, d_out + out_off and d_ref + ref_off 16-byte aligned.  The call knows no buffer sizes: every
 * item must lie inside the buffers given, every `image` inside d_flags.  LEP_ASSERTION_FAILURE: a misaligned item or a prefix item
 * where the form takes none. */
int lep_batch_debug_scan_check(lep_gpu *g, int bytes_form, const uint8_t *d_out, const uint32_t *d_out_len, const uint8_t *d_ref,
                               const lep_scan_check *items, int n, uint32_t *d_flags);
/* Test hook, of lep_batch_debug_poison's standing (process-global, not re-entrant): arms ONE alteration for the next lep_compress_batch /
 * lep_compress_batch_slices call only -- one byte of a buffer the pipeline owns is XORed with xor_mask by a one-lane kernel, stream-
 * ordered on the compute stream of the chunk that holds `file` (the index in that call's input array):
 *   LEP_TAMPER_STREAM   the stream arena, `offset` into the file's first thread segment: behind the coder kernels, in front of the
 *                       verification decode (applied without verify too: the byte then reaches the .lep)
 *   LEP_TAMPER_SCRATCH  the file's scratch frame: behind the verification decode, in front of the frame comparison
 *   LEP_TAMPER_VSCAN    a baseline file's first check segment as written again: in front of lep_scan_check_bytes_kernel
 *   LEP_TAMPER_PSCAN    a progressive file's first check scan as written again: in front of lep_scan_check_kernel
 * `offset` is held on the host against a size known before anything is queued -- the segment's reservation in the stream arena, the
 * frame's exact bytes, the check segment's output cap -- and an offset outside, a file that is not in a chunk, or a buffer the call
 * does not have (no verify, no check segment) leaves the alteration unapplied: it never writes outside the buffer it names.  It is
 * disarmed when the call returns, applied or not; where = 0 disarms at once.  lep_batch_debug_tamper_applied: how often the last armed
 * alteration was applied, 0 or 1. */
enum { LEP_TAMPER_STREAM = 1, LEP_TAMPER_SCRATCH = 2, LEP_TAMPER_VSCAN = 3, LEP_TAMPER_PSCAN = 4 };
void lep_batch_debug_tamper(int where, int file, uint64_t offset, int xor_mask);
int lep_batch_debug_tamper_applied(void);
/* ... and what the check then said of the altered file in a call with verify (both 0 when the file's coder had refused it, or without
 * verify): its flag word, and the first status of its verification decode that was not zero.  Returns the applied count. */
int lep_batch_debug_tamper_seen(uint32_t *flags, int32_t *decode_status);

/* ---- serving surface ------------------------------------------------------------------------------
 * The `lepton -socket[=name] / -listen[=port]` protocol (src/lepton/socket_serve.cc:312-390, jpgcoder.cc:1162-1186):
 * a client connects, sends one whole file, half-closes (shutdown(SHUT_WR)) and reads the converted file until EOF --
 * JPEG in -> .lep out, .lep in -> JPEG out, chosen by the first two bytes (jpgcoder.cc:2178-2235).  The zlib socket
 * (<name>.z0 / -zliblisten) returns a decoded JPEG as a zlib stream of stored blocks (src/io/Zlib0.cc:36-120); so does a
 * .lep whose magic is 0xce 0xb6 (jpgcoder.cc:552).  A failed request gets no bytes, only the close; the exit code the
 * reference's forked child would have died with is logged and counted.  -timebound: time_bound_ms after a request's
 * first byte the connection is closed, answered or not (the reference's SIGALRM, jpgcoder.cc:1740-1752).
 * Where the reference forks one process per connection (accept_new_connection, socket_serve.cc:86-116) and bounds them
 * with -maxchildren, this server gathers the requests that arrive within batch_window_us (or until max_batch are
 * waiting) and hands them to lep_compress_batch / lep_decompress_batch as ONE GPU batch; max_connections plays
 * -maxchildren's part (further clients wait in the listen backlog).  One server per GPU: run one process per device. */
typedef int (*lep_serve_process_fn)(void *user, int kind /* 0: JPEG -> .lep, 1: .lep -> JPEG */, const lep_bytes *in, int n,
                                    lep_bytes *outs /* malloc'd by the callee */, int32_t *status);
/* stream_band_mcu_rows > 0: decompress requests that did not arrive on a zlib listener or under the ce b6 magic are answered through
 * lep_decompress_batch_stream, band by band: the batcher's sink appends to the connection's output, which is sent as it grows; the
 * connection is closed when its file is finished and everything is sent.  A file that fails after bytes went out gets the close and
 * counts as failed (the reference's worker dies the same way); a client that went away makes the sink return non-zero for that file only.
 * Compress requests and zlib answers take the whole-answer path, and so does everything when the option is 0.  Sessions run one after
 * another: the option trades throughput for time to first byte.  The test callback receives the files, a sink and its user, and fills status. */
typedef int (*lep_serve_stream_fn)(void *user, const lep_bytes *in, int n, lep_batch_sink sink, void *sink_user, int32_t *status);
typedef struct lep_serve_options {
    const char *uds_path;        /* -socket=<name>; the zlib socket is <name>.z0, the lock file <name>.lock; NULL = no UDS */
    const char *zlib_uds_path;   /* NULL = <uds_path>.z0 (the reference's random names are /tmp/<id>.uport and /tmp/<id>.z0) */
    int32_t tcp_port;            /* -listen=<port>; 0 = no TCP listener */
    int32_t zlib_tcp_port;       /* -zliblisten=<port>; 0 = none */
    int32_t listen_backlog;      /* -listenbacklog (default 16) */
    int32_t max_connections;     /* -maxchildren: connections in flight before accept() pauses; 0 = unbounded */
    uint32_t max_file_bytes;     /* larger uploads are dropped; 0 = 256 MiB */
    uint32_t time_bound_ms;      /* -timebound; 0 = none */
    int32_t max_batch;           /* files per GPU batch; 0 = 1024 */
    int32_t batch_window_us;     /* how long the batcher waits for company once a request is complete; 0 = 2000 */
    lep_gpu *gpu;                /* used by the default processor */
    lep_batch_options batch;     /* passed through to lep_*_batch (verify = the reference's default round-trip check) */
    lep_serve_process_fn process;   /* NULL = the GPU batch pipeline; tests substitute the CPU oracle here */
    void *process_user;
    int32_t stream_band_mcu_rows;   /* -streamband; 0 = off */
    lep_serve_stream_fn stream_process;   /* NULL = lep_decompress_batch_stream on gpu; tests substitute a callback.  The two callbacks go together: with
                                             `process` set and this one NULL there is no device to stream from, and the option is ignored (whole answers from `process`) */
    void *stream_user;
} lep_serve_options;
typedef struct lep_serve_stats {
    uint64_t accepted, answered, failed, timed_out, rejected;   /* connections */
    uint64_t batches, largest_batch;
    uint64_t bytes_in, bytes_out;
    int32_t last_failure_code;   /* exit code of the most recent failed request */
    uint64_t streamed;              /* connections answered in pieces */
    uint64_t bytes_out_before_done; /* bytes sent while the file's batch call had not yet returned */
} lep_serve_stats;
typedef struct lep_server lep_server;
/* binds and starts the IO + batcher threads; LEP_OS_ERROR if a socket cannot be bound (or the lock is held: another
 * server owns <name>, socket_serve.cc:331-356) */
int lep_serve_start(const lep_serve_options *opt, lep_server **out);
void lep_serve_get_stats(lep_server *s, lep_serve_stats *out);
void lep_serve_stop(lep_server *s);   /* closes listeners and connections, joins, removes the socket files it owns */
/* zlib stream of stored blocks exactly as Zlib0Writer emits it (src/io/Zlib0.cc) */
int lep_zlib0_wrap(const uint8_t *data, size_t len, lep_bytes *out);

void lep_free(void *p);   /* frees lep_bytes.data returned by this library */
const char *lep_version(void);

#ifdef __cplusplus
}
#endif
#endif
