// lep_huffprog_simt_rst.h -- PROGRESSIVE scans WITH A RESTART INTERVAL written with one lane per run of blocks: lep_huffprog_simt.h's passes
// (count / place / assign / zero / code / stuff) with a unit map that never straddles an interval's end.  Same bytes as ProgWave::run_scan
// (lep_huffprog.h), which restates the reference's scan loop (src/lepton/jpgcoder.cc:3309-3716, encode_eobrun, encode_crbits).
//
// A restart interval makes the lane form easier, not harder: where an interval ends the end-of-band run is written, the correction bits
// it held back are out, the stream is padded to a byte, the marker FF D0+(k & 7) follows (k counts the scan's intervals from 0; none behind
// the scan's last interval) and the DC predictors are zero again.  So
//   * unit map      a restart unit is one MCU for an interleaved (DC) scan and one block for a one-component scan; an interval of R restart
//                   units is cut into ceil(R / 32) units of blocks (ceil(R / 8) of MCUs), the last as short as it comes out; a unit's
//                   range is a closed form of its index (ProgRstUnitMap);
//   * count / code  prog_simt_walk of lep_huffprog_simt.h; a unit an interval starts with starts from zero predictors; the unit an interval
//                   ends with inside the scan appends, in the code pass, the pad bits to the byte boundary and the marker's 16 bits and
//                   names the marker's FF in the marker map behind the bit buffer (one bit per buffer byte, as lep_huff_simt.h does);
//   * place         the run state is cut at the intervals' ends: `la` stops at the end of the unit's interval, `cin` counts from the
//                   interval's first block at the earliest; the prefix sum adds the pad bits and the 16 behind every interval that ends
//                   inside the scan (an interval starts on a byte, so its pad is minus its own bit count modulo eight).  Summed in 64
//                   bits: a scan of more than 2^32 - 1 bits gets no buffer and answers "outgrew" (ProgSimtScan.refused);
//   * assign, zero, stuff   lep_huffprog_simt.h's, which know the marker map (ProgSimtScan.rsti / map_bytes).
// SPMD layer of lep_wave.h: tests/emu/prog_simt_rst_emu.cc steps every pass on the CPU against lep_huffprog.h, byte for byte.
#pragma once
#include "lep_huffprog_simt.h"

namespace lephuff {

// Which restart units (blocks of a one-component scan, MCUs of an interleaved DC scan) a unit codes: interval iv = u / per_interval holds
// [iv * rsti, min((iv + 1) * rsti, n)), cut into runs of `per` from its first.
struct ProgRstUnitMap {
    uint32_t n, rsti, per, per_interval;
    LEPH_BOTH void set(uint32_t nblocks, uint32_t interval, bool mcus) {
        n = nblocks; rsti = interval; per = mcus ? (uint32_t)kProgDcMcus : (uint32_t)kProgUnit;
        per_interval = (uint32_t)(((uint64_t)rsti + per - 1) / per);
    }
    LEPH_BOTH uint64_t count() const { return (uint64_t)(n / rsti) * per_interval + ((uint64_t)(n % rsti) + per - 1) / per; }
    // unit u: [*a0, *a1), the first restart unit of its interval and the interval's end
    LEPH_BOTH void span(uint32_t u, uint32_t* a0, uint32_t* a1, uint32_t* ibegin, uint32_t* iend) const {
        const uint32_t iv = u / per_interval, k = u - iv * per_interval;
        const uint32_t b = iv * rsti, e = n - b < rsti ? n : b + rsti, from = b + k * per;
        *a0 = from; *a1 = e - from < per ? e : from + per; *ibegin = b; *iend = e;
    }
    LEPH_BOTH uint32_t interval_first_unit(uint32_t u) const { return u - u % per_interval; }
};

// which scans this form takes (those with a restart interval that lep_huffprog_simt.h's would take without one), and how many units it cuts
// one into
inline bool prog_simt_rst_takes(const ProgImage& im, const ProgScan& sc, uint32_t* nblocks, uint32_t* nunits, uint32_t* rsti) {
    const int r = prog_scan_rsti(im, sc);
    if (r <= 0 || prog_is_sequential(sc)) return false;
    ProgScan plain = sc;
    plain.rsti = 0;
    uint32_t nb = 0, nu = 0;
    if (!prog_simt_takes(im, plain, &nb, &nu)) return false;
    ProgRstUnitMap map;
    map.set(nb, (uint32_t)r, sc.to == 0 && sc.cmpc > 1);
    const uint64_t units = map.count();
    if (units == 0 || units > 0x3fffffffu) return false;
    *nblocks = nb; *nunits = (uint32_t)units; *rsti = (uint32_t)r;
    return true;
}

// passes 1 and 3: lanes = units first_unit .. of scan `ps`
template <bool WRITE>
WDEV void prog_simt_rst_units(const ProgImage* images, const ProgScan* scans, const ProgSimtScan* psp, ProgSimtShared* sh, ProgSimtUnits U, uint8_t* scratch, uint32_t first_unit) {
    const ProgSimtScan ps = *psp;
    const ProgScan* sc = scans + ps.scan;
    const ProgImage* pim = images + sc->image;
    prog_simt_tables(sc, sh);
    ProgRstUnitMap map;
    map.set(ps.nblocks, ps.rsti, sc->to == 0 && sc->cmpc > 1);
    LANES(l) {
        const uint32_t u = first_unit + (uint32_t)l;
        if (u < ps.nunits) {
            uint32_t a0, a1, ibegin, iend;
            map.span(u, &a0, &a1, &ibegin, &iend);
            ProgSimtLane<WRITE> d;
            d.pim = pim; d.sc = sc; d.sh = sh; d.from = sc->from; d.to = sc->to; d.sal = sc->sal;
            const size_t gu = (size_t)ps.first_unit + u;
            d.sink.start(WRITE ? U.bits[gu] : 0u, reinterpret_cast<uint32_t*>(scratch + ps.buf_off), ps.buf_bytes >> 2);
            uint32_t nonE = 0, pmask = 0;
            prog_simt_walk<WRITE>(d, a0, a1, a0 == ibegin, U, gu, &nonE, &pmask);
            if (WRITE && a1 == iend && iend < ps.nblocks) {   // the interval ends with this unit, inside the scan: abitwriter::pad, then the marker
                const uint32_t n = (0u - d.sink.bitpos()) & 7u;
                uint32_t v = 0;
                for (uint32_t j = 0; j < n; ++j) v = (v << 1) | (uint32_t)((pim->padbit >> j) & 1);
                d.sink.put(v, n);
                const uint32_t q = d.sink.bitpos() >> 3;   // the buffer byte the marker's FF becomes
                if (q < ps.buf_bytes && ps.map_bytes) simt_or_word(reinterpret_cast<uint32_t*>(scratch + ps.buf_off + ps.buf_bytes) + (q >> 5), 1u << (q & 31u));
                d.sink.put(0xffd0u | ((ibegin / ps.rsti) & 7u), 16);
            }
            d.sink.finish();
            if (!WRITE) { U.bits[gu] = d.sink.total; U.nonE[gu] = nonE; U.pmask[gu] = pmask; }
        }
    }
}

// pass 2: one wavefront per scan
WDEV void prog_simt_rst_place(const ProgScan* scans, ProgSimtScan* psp, ProgSimtUnits U) {
    const ProgSimtScan ps = *psp;
    const ProgScan* sc = scans + ps.scan;
    const bool ac = sc->to != 0;
    const uint32_t nunits = ps.nunits, fu = ps.first_unit, max = (uint32_t)sc->max_eobrun;
    ProgRstUnitMap map;
    map.set(ps.nblocks, ps.rsti, !ac && sc->cmpc > 1);
    if (ac) {
        // (a) la: empty-band blocks behind every unit = min(first coding block at or after the next unit, end of the unit's interval) - the
        //     unit's end.  Suffix minimum, batches of 64 units from the back.
        uint32_t carry = ps.nblocks;   // first coding block at or after the batch behind this one
        for (uint32_t top = nunits; top > 0;) {
            const uint32_t base = top > 64 ? top - 64 : 0, cnt = top - base;
            LV(int, v); LV(int, sm);
            LANES(l) {
                const uint32_t nx = base + (uint32_t)l + 1;   // lane l looks at its unit's successor
                int first = (int)kProgNone;
                if ((uint32_t)l < cnt && nx < nunits) {
                    const uint32_t m = U.nonE[fu + nx];
                    if (m) { uint32_t a0, a1, ib, ie; map.span(nx, &a0, &a1, &ib, &ie); first = (int)(a0 + (uint32_t)__builtin_ctz(m)); }
                }
                L(v) = first;
            }
            lepwave::wave_suffix_min(v, sm);
            LANES(l) {
                const uint32_t u = base + (uint32_t)l;
                if ((uint32_t)l < cnt) {
                    uint32_t a0, a1, ib, ie;
                    map.span(u, &a0, &a1, &ib, &ie);
                    uint32_t nn = (uint32_t)L(sm) < carry ? (uint32_t)L(sm) : carry;
                    if (ie < nn) nn = ie;
                    U.la[fu + u] = nn - a1;
                }
            }
            {   // the batch in front needs the first coding block at or after unit `base`
                const uint32_t sm0 = lepwave::wave_read((const uint32_t*)sm, 0);
                uint32_t own = kProgNone;
                const uint32_t m = U.nonE[fu + base];
                if (m) { uint32_t a0, a1, ib, ie; map.span(base, &a0, &a1, &ib, &ie); own = a0 + (uint32_t)__builtin_ctz(m); }
                const uint32_t c2 = sm0 < carry ? sm0 : carry;
                carry = own < c2 ? own : c2;
            }
            top = base;
        }
        LSYNC();
        // (b) cin: block x stands (x - B) mod max blocks into a run, B = the last coding block in front of it if that one left its band
        //     open, the block behind it if it closed it -- and the first block of x's interval at the earliest.  Prefix maximum over the units.
        uint32_t bcarry = 0;
        for (uint32_t base = 0; base < nunits; base += 64) {
            LV(int, v); LV(int, pm);
            LANES(l) {
                const uint32_t u = base + (uint32_t)l;   // lane l looks at its unit's predecessor
                int b = 0;
                if (u < nunits && u > 0) {
                    const uint32_t m = U.nonE[fu + u - 1];
                    if (m) {
                        uint32_t a0, a1, ib, ie;
                        map.span(u - 1, &a0, &a1, &ib, &ie);
                        const uint32_t i = 31u - (uint32_t)__builtin_clz(m);
                        b = (int)(a0 + i + (((U.pmask[fu + u - 1] >> i) & 1u) ? 0u : 1u));
                    }
                }
                L(v) = b;
            }
            lepwave::wave_prefix_max(v, pm);
            LANES(l) {
                const uint32_t u = base + (uint32_t)l;
                if (u < nunits) {
                    uint32_t a0, a1, ib, ie;
                    map.span(u, &a0, &a1, &ib, &ie);
                    uint32_t B = (uint32_t)L(pm) > bcarry ? (uint32_t)L(pm) : bcarry;
                    if (B < ib) B = ib;
                    U.cin[fu + u] = (a0 - B) % max;
                }
            }
            const uint32_t last = lepwave::wave_read((const uint32_t*)pm, 63);
            bcarry = last > bcarry ? last : bcarry;
        }
        LSYNC();
    }
    // (c) the EOBn codes' bits, then the exclusive prefix sum of the units' bits without pads and markers
    uint64_t run = 0;
    for (uint32_t base = 0; base < nunits; base += 64) {
        LV(int, nb); LV(int, ex);
        LANES(l) {
            const uint32_t u = base + (uint32_t)l;
            uint32_t b = 0;
            if (u < nunits) {
                b = U.bits[fu + u];
                if (ac) {
                    uint32_t a0, a1, ib, ie;
                    map.span(u, &a0, &a1, &ib, &ie);
                    const uint32_t n = a1 - a0, nonE = U.nonE[fu + u], pmask = U.pmask[fu + u], la = U.la[fu + u];
                    uint32_t c = U.cin[fu + u];
                    for (uint32_t i = 0; i < n; ++i) {
                        const int type = (nonE >> i) & 1u ? (((pmask >> i) & 1u) ? 1 : 2) : 0;
                        if (type == 1 || (type == 0 && c == 0)) {
                            const uint32_t rest = i + 1 < 32u ? nonE >> (i + 1) : 0u;
                            const uint32_t follow = rest ? (uint32_t)__builtin_ctz(rest) : n - 1 - i + la;
                            uint32_t bits, nn;
                            prog_eob_code(sc->code[0], follow + 1 < max ? follow + 1 : max, &bits, &nn);
                            b += nn;
                        }
                        if (type) c = type == 1 ? 1u : 0u; else ++c;
                        if (c == max) c = 0;
                    }
                }
            }
            L(nb) = (int)b;
        }
        const int t = lepwave::wave_excl_scan(nb, ex);
        LANES(l) { const uint32_t u = base + (uint32_t)l; if (u < nunits) U.plain[fu + u] = (uint32_t)run + (uint32_t)L(ex); }
        run += (uint64_t)(uint32_t)t;
    }
    const uint64_t plain_total = run;
    LSYNC();
    // (d) ... plus, behind every interval that ends inside the scan, its pad bits and the sixteen of its marker.  (Modulo 2^32 as long as
    //     nothing is known; a scan whose total does not fit is refused below and nothing of it is written.)
    uint64_t extra = 0;
    for (uint32_t base = 0; base < nunits; base += 64) {
        LV(int, xb); LV(int, ex); LV(uint32_t, plain);
        LANES(l) {
            const uint32_t u = base + (uint32_t)l;
            int x = 0;
            uint32_t p = 0;
            if (u < nunits) {
                p = U.plain[fu + u];
                uint32_t a0, a1, ib, ie;
                map.span(u, &a0, &a1, &ib, &ie);
                if (a1 == ie && ie < ps.nblocks) {
                    const uint32_t next = u + 1 < nunits ? U.plain[fu + u + 1] : (uint32_t)plain_total;
                    x = (int)((0u - (next - U.plain[fu + map.interval_first_unit(u)])) & 7u) + 16;
                }
            }
            L(xb) = x; L(plain) = p;
        }
        const int t = lepwave::wave_excl_scan(xb, ex);
        LANES(l) { const uint32_t u = base + (uint32_t)l; if (u < nunits) U.bits[fu + u] = L(plain) + (uint32_t)extra + (uint32_t)L(ex); }
        extra += (uint64_t)(uint32_t)t;
    }
    const uint64_t total = plain_total + extra;
    LANES(l) if (l == 0) { psp->total_bits = total > 0xffffffffull ? 0xffffffffu : (uint32_t)total; psp->refused = total > 0xffffffffull ? 1u : 0u; }
}

}  // namespace lephuff
