// jpegprog_core.h -- the per-thread work of jpegprog.hip's entropy stage (aej_jpegprog_*): the four progressive decoders of T.81 G.1.2 / G.2,
// written as host + device functions beside jpegdec_core.h so that the same decode can be stepped through on the CPU
// (aej_test_jpegprog_coefs_host).  Everything is bounded by what it is given: every bit read by the restart segment's end, every
// coefficient store by the scan's unit count and the file's block count.
#pragma once
#include "jpegdec_core.h"

namespace aej {

enum { kJpDcFirst = 0, kJpAcFirst = 1, kJpDcRefine = 2, kJpAcRefine = 3 };
constexpr int kJpItem = 64;            // restart segments (DC refinement: units) one workgroup serves

// one scan of one file, as the decoders see it (host-computed, uploaded once per call; ordered by dependency level)
struct JpScan {
    int file, kind, level;
    int ncomp, comp0;                  // components in the scan; the first (the only one of a non-interleaved scan)
    int ss, se, al;
    int nf, hs, vs, mcux, bpm;         // the frame: components, luma sampling, MCUs per row, blocks per MCU
    int units_x, units_y;              // what the scan walks: the MCU grid (interleaved) or the component's own block grid
    int restart_interval, n_segments;
    long long seg_base;                // first restart segment (global index)
    long long blk_base, n_blocks;      // the file's coefficient blocks, MCU order
    int h3, v3;                        // component 3's sampling factors (aej_jpeg_adobe), 0 unless the file has four components
};

struct JpItem { int scan, first; };    // a workgroup's share of a level: kJpItem segments (units) of one scan from `first` on

AEJ_HD inline int jp_blocks_per_unit(const JpScan &s) { return s.ncomp > 1 ? s.bpm : 1; }

// block `k` of unit `u` of the scan -> its index among the file's blocks (MCU order, the layout k_jd_idct reads); -1 outside the file
// kFour (here and below: a call with a four-component file): component 3 sampled as component 0 walks its own block grid, and its
// blocks follow the MCU's others
template <bool kFour = false>
AEJ_HD inline long long jp_slot(const JpScan &s, long long u, int k)
{
    long long b;
    if (s.ncomp > 1 || s.nf == 1) {
        b = u * s.bpm + k;
    } else {
        const long long by = u / s.units_x, bx = u % s.units_x;
        if (s.comp0 == 0) b = ((by / s.vs) * s.mcux + bx / s.hs) * s.bpm + (by % s.vs) * s.hs + bx % s.hs;
        else if (kFour && s.comp0 == 3 && s.h3 == s.hs && s.v3 == s.vs)
            b = ((by / s.vs) * s.mcux + bx / s.hs) * s.bpm + s.hs * s.vs + 2 + (by % s.vs) * s.hs + bx % s.hs;
        else b = (by * s.mcux + bx) * s.bpm + s.hs * s.vs + s.comp0 - 1;
    }
    return b >= 0 && b < s.n_blocks ? b : -1;
}

// bit cursor over one restart segment: no read at or past `end`
struct JpBits {
    JdBits br;
    long long pos, end;
    AEJ_HD JpBits(const unsigned char *clean, long long start_bit, long long end_bit) : br(clean), pos(start_bit), end(end_bit) {}
    AEJ_HD inline bool bit(int &b)
    {
        if (pos >= end) return false;
        b = (int)(br.peek32(pos) >> 31);
        pos++;
        return true;
    }
    // one Huffman symbol and `extra(sym)` raw bits after it (at most 15): rc kJdRunStop, or why not
    template <class Extra>
    AEJ_HD inline int symbol(const aej_jpegdec_huff &h, int &sym, unsigned &bits, Extra extra)
    {
        if (pos >= end) return kJdRunOutOfBits;
        const unsigned win = br.peek32(pos);
        int len;
        const int rc = jd_symbol(h, win, end - pos, len, sym);      // (the bits behind `end` decide nothing: jpegdec_core.h)
        if (rc != kJdRunStop) return rc;
        const int nb = extra(sym);
        if (nb < 0) return kJdRunBadDc;
        if (pos + len + nb > end) return kJdRunOutOfBits;
        bits = nb ? (win << len) >> (32 - nb) : 0u;
        pos += len + nb;
        return kJdRunStop;
    }
};

AEJ_HD inline int jp_extend(unsigned bits, int sz) { return sz == 0 ? 0 : bits < (1u << (sz - 1)) ? (int)bits - (1 << sz) + 1 : (int)bits; }

// DC first scan (G.1.2.1): units [u0, u0 + nu) of the scan from one restart segment; tab[i]: the table of the scan's component i
template <bool kFour = false>
AEJ_HD inline int jp_dc_first(const JpScan &s, const aej_jpegdec_huff *tab, JpBits &b, long long u0, int nu, short *coef)
{
    int pred[kFour ? 4 : 3] = {};
    const int bpu = jp_blocks_per_unit(s);
    for (int u = 0; u < nu; u++)
        for (int k = 0; k < bpu; k++) {
            int ci = s.ncomp > 1 ? (k < s.hs * s.vs ? 0 : k - s.hs * s.vs + 1) : 0;
            if (kFour && ci > 3) ci = 3;
            int sym;
            unsigned bits;
            const int rc = b.symbol(tab[ci], sym, bits, [](int v) { return v > 11 ? -1 : v; });
            if (rc != kJdRunStop) return rc;
            pred[ci] += jp_extend(bits, sym);
            const long long slot = jp_slot<kFour>(s, u0 + u, k);
            if (slot >= 0) coef[slot * 64] = (short)(pred[ci] * (1 << s.al));
        }
    return kJdRunStop;
}

// AC first scan (G.1.2.2): one component, band ss..se, EOB runs across blocks
template <bool kFour = false>
AEJ_HD inline int jp_ac_first(const JpScan &s, const aej_jpegdec_huff &tab, JpBits &b, long long u0, int nu, short *coef)
{
    int eobrun = 0;
    for (int u = 0; u < nu; u++) {
        if (eobrun > 0) { eobrun--; continue; }
        const long long slot = jp_slot<kFour>(s, u0 + u, 0);
        for (int k = s.ss; k <= s.se; k++) {
            int sym;
            unsigned bits;
            const int rc = b.symbol(tab, sym, bits, [](int v) { return (v & 15) ? (v & 15) : (v >> 4) < 15 ? (v >> 4) : 0; });
            if (rc != kJdRunStop) return rc;
            const int r = sym >> 4, sz = sym & 15;
            if (sz) {
                k += r;
                if (k > s.se) return kJdRunPast63;
                if (slot >= 0) coef[slot * 64 + jd_natural(k)] = (short)(jp_extend(bits, sz) * (1 << s.al));
            } else if (r == 15) {
                k += 15;
                if (k > s.se) return kJdRunPast63;
            } else {
                eobrun = (1 << r) + (int)bits - 1;       // this block ends here; eobrun more blocks are empty in the band
                break;
            }
        }
    }
    return kJdRunStop;
}

// zigzag positions of the band ss..se whose coefficient is non-zero, as a bit mask (bit z): the history that decides which
// positions of a refinement scan carry a correction bit.  The 64 loads do not depend on each other.
AEJ_HD inline unsigned long long jp_nonzero_mask(const short *blk, int ss, int se)
{
    unsigned long long m = 0;
    for (int z = 1; z < 64; z++) m |= (unsigned long long)(blk[jd_natural(z)] != 0) << z;
    const unsigned long long band = (se >= 63 ? ~0ULL : (1ULL << (se + 1)) - 1) & ~((1ULL << ss) - 1);
    return m & band;
}

AEJ_HD inline void jp_correct(short *c, int al)       // a set correction bit: one more bit of magnitude, away from zero
{
    const int v = *c, p1 = 1 << al;
    if ((v & p1) == 0) *c = (short)(v >= 0 ? v + p1 : v - p1);
}

// AC refinement scan (G.1.2.3): correction bits of the coefficients already non-zero interleaved with new +-1 coefficients
template <bool kFour = false>
AEJ_HD inline int jp_ac_refine(const JpScan &s, const aej_jpegdec_huff &tab, JpBits &b, long long u0, int nu, short *coef)
{
    int eobrun = 0;
    const int p1 = 1 << s.al;
    for (int u = 0; u < nu; u++) {
        const long long slot = jp_slot<kFour>(s, u0 + u, 0);
        if (slot < 0) return kJdRunOutOfBits;                  // cannot happen with the host's geometry; never touch another file
        short *blk = coef + slot * 64;
        const unsigned long long nz = jp_nonzero_mask(blk, s.ss, s.se);
        int k = s.ss, bitv;
        if (eobrun == 0) {
            for (; k <= s.se; k++) {
                int sym;
                unsigned bits;
                const int rc = b.symbol(tab, sym, bits, [](int v) { return (v & 15) ? 1 : (v >> 4) < 15 ? (v >> 4) : 0; });
                if (rc != kJdRunStop) return rc;
                int r = sym >> 4, val = 0;
                if (sym & 15) {
                    val = bits ? p1 : -p1;              // a size other than 1 is taken as 1, as libjpeg does after its warning
                } else if (r != 15) {
                    eobrun = (1 << r) + (int)bits;      // includes this block
                    break;
                }
                for (; k <= s.se; k++) {                // skip r zero-history positions, correcting the others on the way
                    if ((nz >> k) & 1) {
                        if (!b.bit(bitv)) return kJdRunOutOfBits;
                        if (bitv) jp_correct(blk + jd_natural(k), s.al);
                    } else if (--r < 0) {
                        break;
                    }
                }
                if (val) {
                    if (k > s.se) return kJdRunPast63;
                    blk[jd_natural(k)] = (short)val;
                }
            }
        }
        if (eobrun > 0) {                               // the rest of the band: correction bits only
            for (; k <= s.se; k++)
                if ((nz >> k) & 1) {
                    if (!b.bit(bitv)) return kJdRunOutOfBits;
                    if (bitv) jp_correct(blk + jd_natural(k), s.al);
                }
            eobrun--;
        }
    }
    return kJdRunStop;
}

// DC refinement (G.1.2.1): block i of a restart segment is bit i of it
template <bool kFour = false>
AEJ_HD inline int jp_dc_refine_unit(const JpScan &s, const unsigned char *clean, const JdSeg &sg, long long u, short *coef)
{
    const int bpu = jp_blocks_per_unit(s);
    const long long local = u - sg.first_mcu;
    if (local < 0 || local >= sg.n_mcu) return kJdRunStop;
    const unsigned *w = reinterpret_cast<const unsigned *>(clean);
    for (int k = 0; k < bpu; k++) {
        const long long bit = local * bpu + k;
        if (bit >= sg.nbytes * 8) return kJdRunOutOfBits;
        const long long pos = sg.start * 8 + bit;
        const long long slot = jp_slot<kFour>(s, u, k);
        if (((js_bswap(w[pos >> 5]) >> (31 - (int)(pos & 31))) & 1) && slot >= 0) coef[slot * 64] |= (short)(1 << s.al);
    }
    return kJdRunStop;
}

AEJ_HD inline int jp_status(int rc)
{
    return rc == kJdRunStop ? AEJ_JPEGDEC_OK : rc == kJdRunOutOfBits ? AEJ_JPEGDEC_TRUNCATED : rc == kJdRunBadCode ? AEJ_JPEGDEC_BAD_CODE
         : rc == kJdRunPast63 ? AEJ_JPEGDEC_RUN_PAST_63 : AEJ_JPEGDEC_BAD_DC;
}

}  // namespace aej
