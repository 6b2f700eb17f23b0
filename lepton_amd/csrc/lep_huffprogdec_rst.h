// lep_huffprogdec_rst.h -- PROGRESSIVE JPEG scans WITH RESTART INTERVALS decoded with one wavefront per PIECE of the scan
// (BASELINE.json configs[4], encode direction).  Same frames, records and refusals as lep_huffprogdec.h.
//
// A progressive scan is one dependent chain (lep_huffprogdec_win.h) -- except behind a restart marker: there the bit stream is byte
// aligned, the DC predictors and the end-of-band run are zero, and the block the interval starts with follows from its index (MCU
// i * rsti of an interleaved scan; the (i * rsti)-th block of the nch x ncv walk of a one-component scan).  The progressive files
// of phone cameras carry a DRI in front of every scan; their scans are not one chain but hundreds.
//
//   * A scan whose descriptor carries kHuffDecRstTable has the positions of its markers (uint32 offsets into the un-stuffed scan,
//     (units - 1) / rsti of them) behind its zero-padded slot, at scan + progdec_scan_room(scan_len).
//   * PIECE: a run of consecutive intervals of one scan, one wavefront.  The host cuts a scan into pieces of the same NUMBER of
//     intervals, as many as make kRstPieceFloor bytes at the scan's average interval length (prog_rst_plan): with a marker behind
//     every block a 4K luma scan has 130 k intervals of a few bytes, and a wavefront per interval would be all set-up (tables into
//     LDS: 4.6 KB; the ring primed: 2 KB).
//   * The wavefront is lep_huffprogdec_win.h's (ProgWinWave: stage / chain, ac_first_win / ac_refine_win, locate_dc) with its ring
//     pointed at the 16-byte boundary at or in front of the piece's first byte -- the reader keeps its aligned loads, bit positions
//     are relative to that boundary -- and walks its intervals one after the other: the walk over the blocks simply goes on, the
//     predictors and the run start again, the pad bits are collected, and the interval must end exactly where its marker stood.
//   * The MCU-row records of a file's first scan are written by the piece that decodes the row's first block; what is one value
//     per scan -- status, the pad bits every interval must agree on, the last DC -- leaves as one ProgRstOut per piece, and
//     prog_rst_reduce (one wavefront per scan, after the pieces) writes the scan's final record from them.
//   * No scan of this form waits for another: the launch code runs the levels of such a file one after the other on the stream.
//
// Not canonical -> a status on the scan, the host parser takes the file: a code that does not exist, an end-of-band run that reaches
// past its interval, an interval that ends anywhere but at its marker (5), pad bits that differ between intervals (3).
// SPMD layer of lep_wave.h: tests/emu steps it on the CPU against the host parser and against lep_huffprogdec.h.
#pragma once
#include "lep_huffprogdec_win.h"

namespace lephuff {

constexpr uint32_t kRstPieceFloor = 1024;   // bytes of scan a piece holds at least (on average); DESIGN.md 4.4 has the measurement
constexpr int32_t kProgDecRst = 2;          // ProgDecScan::pad: this form decodes the scan

// a progressive scan's slot: its bytes, zero padding (the window reader runs ahead of the data), a 16-byte multiple
WDEV uint32_t progdec_scan_room(uint32_t scan_len) { return (scan_len + 80u + 15u) & ~15u; }

struct ProgRstScan {        // one per scan of this form, device-visible
    uint32_t piece0;        // its first piece among the launch's (and its first ProgRstOut)
    uint32_t npieces;
    uint32_t ipp;           // intervals per piece (the last piece: what is left)
    uint32_t nint;          // intervals
};
struct ProgRstOut {         // one per piece
    uint32_t status;
    uint32_t pad_and, pad_or, pad_n;    // over the intervals that did not end on a byte boundary: their pad patterns and-ed / or-ed, their number
    int16_t last_dc[4];                 // as the piece's last interval left them
};

// restart intervals count MCUs in an interleaved scan and the component's nch x ncv blocks in a scan of one component
inline uint32_t prog_rst_units(const ProgDecScan& s) {
    const int c = s.cmp[0] & 3;
    return s.cmpc > 1 ? (uint32_t)s.t.mcuc : (uint32_t)s.nch[c] * (uint32_t)s.ncv[c];
}
// which scans this form takes: the caller has put the table of marker positions behind the scan's slot (kHuffDecRstTable)
inline bool prog_rst_takes(const ProgDecScan& s) {
    if (!(s.t.flags & kHuffDecRstTable) || progdec_is_sequential(s) || s.t.rsti <= 0 || s.cmpc < 1 || s.cmpc > 4) return false;
    if (s.t.mcuc <= 0 || s.nch[s.cmp[0] & 3] <= 0 || s.ncv[s.cmp[0] & 3] <= 0) return false;
    return prog_rst_units(s) > (uint32_t)s.t.rsti && s.t.scan_len < (1u << 27) && (reinterpret_cast<uintptr_t>(s.t.scan) & 15u) == 0;
}
// pieces of the same number of intervals, floor_bytes of scan each at the average interval length (1: a piece per interval)
inline ProgRstScan prog_rst_plan(const ProgDecScan& s, uint32_t floor_bytes, uint32_t piece0) {
    ProgRstScan p;
    p.nint = (prog_rst_units(s) - 1u) / (uint32_t)s.t.rsti + 1u;
    const uint64_t per = ((uint64_t)floor_bytes * p.nint + s.t.scan_len - 1u) / (s.t.scan_len ? s.t.scan_len : 1u);   // ceil(floor / (scan_len / nint))
    p.ipp = (uint32_t)(per < 1u ? 1u : (per > p.nint ? p.nint : per));
    p.npieces = (p.nint + p.ipp - 1u) / p.ipp;
    p.piece0 = piece0;
    return p;
}

struct ProgRstWave : ProgWinWave {
    LV(uint32_t, ends);                 // lane j: the byte at which interval (first + 64 * chunk + j) ends

    // the intervals [first, first + count) of `scan`
    WDEV void run_piece(const ProgDecScan* scan, ProgWinShared* shared, HuffDecRow* rows_arena, uint32_t nint, uint32_t first, uint32_t count, ProgRstOut* out) {
        deps = nullptr; progress = nullptr; self = 0; ready = 0;
        setup_win(scan, shared);
        const bool dc = scan->to == 0;
        const uint32_t rsti = (uint32_t)img->rsti, scan_len = img->scan_len;
        const uint32_t units = scan->cmpc > 1 ? (uint32_t)img->mcuc : (uint32_t)k.nch * (uint32_t)k.ncv;
        const uint32_t* tab = reinterpret_cast<const uint32_t*>(img->scan + progdec_scan_room(scan_len));
        int st = 0;
        uint32_t start = 0;
        if (count == 0 || first >= nint || count > nint - first || img->rsti <= 0 || (uint64_t)(nint - 1u) * rsti >= units) st = 5;
        else if (first) start = uni(lepwave::gld(tab + (first - 1u)));
        if (start > scan_len) st = 5;
        int lastdc[4] = {0, 0, 0, 0};
        uint32_t pad_and = 0xffu, pad_or = 0, pad_n = 0;
        if (!st) {
            // the ring at the 16-byte boundary in front of the piece: positions are bits behind `origin`
            const uint32_t origin = start & ~15u;
            k.scan = img->scan + origin; k.scan_len = scan_len - origin;
            base = (start - origin) * 8u; off = 0; ring_hi = 0;
            request(0);
            stage();
            HuffDecRow* rows = rows_arena + img->rows_off;
            const int mcuh = img->mcuh, sal = scan->sal;
            const uint32_t origin_bits = origin * 8u;
            eobrun = 0; peobrun = 0;
            // where the piece's first unit lies; from there the walk goes on from interval to interval
            const uint32_t u0 = first * rsti;
            // ... interleaved scans: MCU (mx, my), block q of an MCU at `where` / of kind `what` (lep_huffprogdec_win.h)
            LV(uint32_t, where); LV(uint32_t, what);
            uint32_t P = 0;
            int rowbase[4] = {0, 0, 0, 0}, stride[4] = {0, 0, 0, 0};
            int16_t* frame[4] = {nullptr, nullptr, nullptr, nullptr};
            int mx = 0, my = 0;
            if (scan->cmpc > 1) {
                LANES(l) { L(where) = 0; L(what) = 0; }
                for (int i = 0; i < scan->cmpc; ++i) {
                    const int c = scan->cmp[i];
                    const uint32_t hs = (uint32_t)img->hs[c], n = (uint32_t)scan->mbs[c], bch = (uint32_t)img->bch[c];
                    LANES(l) {
                        const uint32_t q = (uint32_t)l - P;
                        if ((uint32_t)l >= P && q < n) { L(where) = (q / hs) * bch + q % hs; L(what) = (uint32_t)c | (uint32_t)(scan->tbl[i] & 1) << 2 | (uint32_t)i << 3 | hs << 8; }
                    }
                    P += n;
                }
                my = (int)(u0 / (uint32_t)mcuh); mx = (int)(u0 - (uint32_t)my * (uint32_t)mcuh);
                for (int c = 0; c < 4; ++c) { stride[c] = img->vs[c] * img->bch[c]; frame[c] = img->blocks[c]; rowbase[c] = my * stride[c]; }
            } else P = 1;
            // ... one-component scans: block (col, row) of the component's nch x ncv blocks
            int row = (int)(u0 / (uint32_t)k.nch), col = (int)(u0 - (uint32_t)row * (uint32_t)k.nch);
            int dpos = row * k.bch + col, cur_row = -1;
            bool stray = false;
            for (uint32_t iv = first; iv < first + count; ++iv) {
                if (((iv - first) & 63u) == 0) {
                    LANES(l) { const uint32_t j = iv + (uint32_t)l; L(ends) = j + 1u < nint ? lepwave::gld(tab + j) : scan_len; }
                }
                const uint32_t end = lepwave::wave_read(ends, (int)((iv - first) & 63u));
                // (the window is never asked for bits behind the interval's marker plus one code: what stands there is the next
                // interval's, or the slot's zero padding)
                const uint32_t limit = end <= scan_len && end >= origin ? (end - origin) * 8u : 0u;
                uint32_t left = units - iv * rsti < rsti ? units - iv * rsti : rsti;   // units of this interval still to decode
                lastdc[0] = lastdc[1] = lastdc[2] = lastdc[3] = 0;
                eobrun = 0; peobrun = 0;
                int sta = 0;
                if (dc && scan->sah != 0) {
                    // DC refinement: a bit per block, 64 blocks per step
                    const uint32_t b0 = iv * rsti * P, nb = left * P;
                    for (uint32_t i0 = 0; i0 < nb; i0 += 64) {
                        const uint32_t n = nb - i0 < 64u ? nb - i0 : 64u;
                        if (off) stage();
                        LANES(l) {
                            if ((uint32_t)l < n && (L(win) >> 31)) {
                                int cmp, dp;
                                locate_dc(b0 + i0 + (uint32_t)l, P, &cmp, &dp);
                                int16_t* dst = img->blocks[cmp] + (int64_t)dp * 64 + 49;
                                lepwave::gst(dst, (int16_t)(lepwave::gld(dst) + (int16_t)(1u << sal)));
                            }
                        }
                        off = n;
                        if (pos() > limit) { sta = -1; break; }
                    }
                    if (!sta) sta = iv + 1u == nint ? 2 : 1;
                } else if (dc && scan->cmpc > 1) {
                    // DC first stage over MCUs
                    for (uint32_t m = 0; m < left && !sta; ++m) {
                        if (k.want_rows && mx == 0) {
                            const uint32_t bp = origin_bits + pos();
                            LANES(l) if (l == 0) { rows[my].bitpos = bp; for (int c = 0; c < 4; ++c) rows[my].last_dc[c] = (int16_t)lastdc[c]; rows[my].aux = 0; }
                        }
#pragma nounroll
                        for (uint32_t q = 0; q < P; ++q) {
                            const uint32_t wt = lepwave::wave_read(what, (int)q), wh = lepwave::wave_read(where, (int)q);
                            const int c = (int)(wt & 3u);
                            uint32_t len, sym, f16;
                            if (!code_at((int)((wt >> 2) & 1u), &len, &sym, &f16) || sym > 15u) { sta = -1; break; }
                            off += len + sym;
                            const int last = c == 0 ? lastdc[0] : (c == 1 ? lastdc[1] : (c == 2 ? lastdc[2] : lastdc[3]));
                            const int v = (int16_t)(devli(sym, sym ? f16 >> (16u - sym) : 0u) + last);
                            if (c == 0) lastdc[0] = v; else if (c == 1) lastdc[1] = v; else if (c == 2) lastdc[2] = v; else lastdc[3] = v;
                            const int rb = c == 0 ? rowbase[0] : (c == 1 ? rowbase[1] : (c == 2 ? rowbase[2] : rowbase[3]));
                            int16_t* fr = c == 0 ? frame[0] : (c == 1 ? frame[1] : (c == 2 ? frame[2] : frame[3]));
                            int16_t* dst = fr + (int64_t)(rb + mx * (int)(wt >> 8) + (int)wh) * 64 + 49;
                            LANES(l) if (l == 0) lepwave::gst(dst, (int16_t)((uint16_t)v << sal));
                            if (pos() > limit) { sta = -1; break; }
                        }
                        if (++mx == mcuh) { mx = 0; ++my; for (int c = 0; c < 4; ++c) rowbase[c] += stride[c]; }
                    }
                    if (!sta) sta = iv + 1u == nint ? 2 : 1;
                } else {
                    // one component: DC first stage or an AC scan (run_scan_win's walk, with the interval's units counted down)
                    while (sta == 0) {
                        if (row != cur_row) {
                            flush_store();
                            cur_row = row;
                            if (!dc && k.sah != 0) request_block(dpos);
                        }
                        if (dc) {
                            if (k.want_rows && col == 0 && (k.cmp == 0 || row == 0)) {
                                const uint32_t bp = origin_bits + pos();
                                LANES(l) if (l == 0) { rows[row].bitpos = bp; for (int c = 0; c < 4; ++c) rows[row].last_dc[c] = (int16_t)lastdc[c]; rows[row].aux = 0; }
                            }
                            uint32_t len, sym, f16;
                            if (!code_at(k.tbl0, &len, &sym, &f16) || sym > 15u) { sta = -1; break; }
                            off += len + sym;
                            const int v = (int16_t)(devli(sym, sym ? f16 >> (16u - sym) : 0u) + lastdc[0]);
                            lastdc[0] = v;
                            int16_t* dst = k.blocks + (int64_t)dpos * 64 + 49;
                            LANES(l) if (l == 0) lepwave::gst(dst, (int16_t)((uint16_t)v << sal));
                        } else {
                            const int rc = k.sah == 0 ? ac_first_win(dpos) : ac_refine_win(dpos, col + 1 < k.nch);
                            if (rc < 0) { sta = -1; break; }
                            if (k.sah == 0 && eobrun) {          // a run: its blocks are passed as a whole
                                if (!stray && col + (int)eobrun < k.nch && eobrun < left) { col += (int)eobrun; dpos += (int)eobrun; left -= eobrun; eobrun = 0; }
                                else {                           // skip_eobrun's own arithmetic, the interval's bound included
                                    int rstw = (int)left;
                                    sta = skip_run(k.cmp, &dpos, &rstw);
                                    left = (uint32_t)rstw;
                                    row = dpos / k.bch; col = dpos - row * k.bch;
                                    if (row >= k.ncv || col >= k.nch) stray = true;
                                }
                            }
                        }
                        if (sta == 0) {
                            if (stray) {
                                int rstw = (int)left;
                                sta = next_noninterleaved(k.cmp, &dpos, &rstw);
                                left = (uint32_t)rstw;
                                row = dpos / k.bch; col = dpos - row * k.bch;
                            } else {
                                ++col; ++dpos;
                                if (col >= k.nch) { col = 0; ++row; dpos = row * k.bch; }
                                if (row >= k.ncv) sta = 2;
                                else if (--left == 0) sta = 1;
                            }
                        }
                        if (pos() > limit) { sta = -1; break; }
                    }
                    if (sta > 0 && eobrun > 0) sta = -1;         // a run that reaches past the end of its interval
                }
                if (sta == -1) { st = 1; break; }
                const int got = unpad_win(255);                  // (255: the interval ends on a byte boundary and says nothing about the pad bits)
                if (got != 255) { pad_and &= (uint32_t)got; pad_or |= (uint32_t)got; ++pad_n; }
                if (pos() != limit || end > scan_len || end < origin) { st = 5; break; }   // the marker stood elsewhere
                if ((sta == 2) != (iv + 1u == nint)) { st = 2; break; }                    // the walk and the interval count disagree
            }
            flush_store();
            if (dc && scan->sah == 0 && scan->cmpc == 1) { const int v = lastdc[0]; lastdc[0] = 0; lastdc[k.cmp & 3] = v; }
        }
        LANES(l) if (l == 0) {
            out->status = (uint32_t)st; out->pad_and = pad_and; out->pad_or = pad_or; out->pad_n = pad_n;
            for (int c = 0; c < 4; ++c) out->last_dc[c] = (int16_t)lastdc[c];
        }
    }
};

// the scan's final record from what its pieces left (one wavefront per scan, behind the pieces)
WDEV void prog_rst_reduce(const ProgDecScan* scan, const ProgRstScan* plan, const ProgRstOut* outs, HuffDecRow* rows_arena) {
    const ProgRstOut* o = outs + plan->piece0;
    const uint32_t n = plan->npieces;
    LV(int, stv); LV(int, cnt); LV(uint32_t, pa); LV(uint32_t, po);
    LANES(l) {
        int s = 0, c = 0;
        uint32_t a = 0xffu, r = 0;
        for (uint32_t i = (uint32_t)l; i < n; i += 64) {
            const uint32_t si = lepwave::gld(&o[i].status);
            s = (int)si > s ? (int)si : s;
            a &= lepwave::gld(&o[i].pad_and); r |= lepwave::gld(&o[i].pad_or); c += (int)lepwave::gld(&o[i].pad_n);
        }
        L(stv) = s; L(cnt) = c; L(pa) = a; L(po) = r;
    }
    int status = lepwave::wave_max(stv);
    const int npad = lepwave::wave_sum(cnt);
    uint32_t pad_and = 0, pad_or = 0;
    for (int b = 0; b < 8; ++b) {
        LV(int, one); LV(int, zero);
        LANES(l) { L(one) = (int)((L(po) >> b) & 1u); L(zero) = (int)(((L(pa) >> b) & 1u) ^ 1u); }
        if (lepwave::wave_ballot(one)) pad_or |= 1u << b;
        if (!lepwave::wave_ballot(zero)) pad_and |= 1u << b;
    }
    int padbit = -1;
    if (npad) {
        if (pad_and != pad_or) { if (!status) status = 3; }   // "inconsistent use of padbits"
        else padbit = (int)pad_and;
    }
    HuffDecRow* fin = rows_arena + scan->result_off;
    const uint32_t bp = status ? 0u : scan->t.scan_len * 8u;   // (every interval ended at its marker, the last one at the scan's end)
    LANES(l) if (l == 0) {
        fin->bitpos = bp;
        for (int c = 0; c < 4; ++c) fin->last_dc[c] = n ? lepwave::gld(&o[n - 1u].last_dc[c]) : (int16_t)0;
        fin->aux = (padbit & 255) | (status << 8);
    }
}

}  // namespace lephuff
