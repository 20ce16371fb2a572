// jfif_prog_core.h -- what one block gives a Huffman-coded JPEG scan, written once as host + device functions: the sequential block
// of Annex F.1.2 (je_block_seq: every baseline writer of jfif.hip -- histogram, bit count, the quantiser's Annex K count, emitter) and
// the Annex G (progressive) coder as libjpeg's jcphuff.c runs it (jfifprog.hip).  A sequential block is the progressive pieces at
// Al = 0 -- je_dc_first, je_ac_first over 1 .. 63, the EOB symbol -- so both coders and both host testing entries
// (aej_test_jfif_seq_scan_host, aej_test_jfif_prog_scan_host) step through one text.  The sinks a block is coded into (nothing, a
// histogram, a bit count, the bit writer) and the DC predictor with its restart rule (je_dc_pred) are here too.
//
// libjpeg codes a progressive scan serially: an end-of-band run (EOBRUN) and the correction bits deferred behind it (BE) pass from block
// to block.
// Here a block is coded on its own (je_dc_*, je_ac_first, je_ac_refine report what it emits to a sink and what it leaves pending), and
// the state between blocks is a partition of the scan into pieces:
//   a block "joins" when it ends with zeros or deferred bits pending (r > 0 || BR > 0); a block that emits no symbol always joins;
//   a chain is a joining block followed by the blocks that emit nothing, up to the next block that emits; libjpeg's run cannot
//   outlive the chain, because a block's first symbol flushes it;
//   within a chain libjpeg flushes when the run reaches 0x7FFF blocks or more than 937 deferred bits are pending; each flush ends a
//   piece (je_chain_end, je_piece_end: binary searches over an exclusive prefix sum of packed (break, BR) values, je_pack);
//   the stream is then, block after block: the block's own symbols, the EOBn symbol of the piece it opens, its deferred bits.
#pragma once
#include <stdint.h>

#include "jfif_restart_core.h"
#include "jfif_stream_core.h"

namespace aej {

constexpr int kJeMaxRun = 0x7FFF;      // blocks in one end-of-band run
constexpr int kJeMaxDeferred = 937;    // MAX_CORR_BITS - DCTSIZE2 + 1: a run is flushed once more bits than this are deferred
constexpr int kJeMaxCoef = 2047;       // |coefficient| the bit bounds below hold for (8-bit JPEG stays within 1023 AC, 1024 DC)
constexpr int kJeBrShift = 36;         // je_pack: deferred bits in the low 36 bits, breaks above

struct JeBlock {
    int e, r, br;                      // emits a symbol; zeros pending at the end of the band; correction bits pending
    unsigned long long brbits;         // those bits, the first one highest
};

// bits that bound one block of a scan (|coefficients| <= kJeMaxCoef): DC first 16 + 12; DC refinement 1; AC first 16 + 11 per
// coefficient (a ZRL stands for 16 of them); AC refinement 16 + 1 per coefficient; the EOBn symbol 16 + 14
AEJ_HD inline int je_block_bound(int Ss, int Se, int Ah)
{
    if (Ss == 0) return Ah ? 1 : 28;
    return (Ah ? 17 : 27) * (Se - Ss + 1) + 30;
}

// A sink takes sym(s, n = 1): the Huffman symbol s, n >= 0 times in a row (the ZRLs of a zero run); bits(v, n): n <= 16 raw bits; many(v, n): n <= 63 raw bits, the first one highest.  Its
// member `codes` is the table its symbols index (code words, or a histogram's counters): the caller points it at the DC or the AC table.
template <class Sink>
AEJ_HD inline void je_dc_first(int cur, int prev, int Al, Sink &s)      // prev: the component's block before in scan order (0 at the start)
{
    const int diff = (cur >> Al) - (prev >> Al), n = js_nbits(diff);
    s.sym(n);
    if (n) s.bits((unsigned)(diff < 0 ? diff - 1 : diff) & ((1u << n) - 1), n);
}
template <class Sink>
AEJ_HD inline void je_dc_refine(int cur, int Al, Sink &s) { s.bits((unsigned)(cur >> Al) & 1u, 1); }

// c: anything indexable that yields the coefficients (a const short *, or a source that computes them): every index Ss .. Se is read
// exactly once, in increasing order, so a source may do its work -- quantise, store -- inside operator[]
template <class Src, class Sink>
AEJ_HD inline JeBlock je_ac_first(Src c, int Ss, int Se, int Al, Sink &s)
{
    JeBlock b = { 0, 0, 0, 0 };
    int r = 0;
    for (int k = Ss; k <= Se; k++) {
        const int v = c[k], t = (v < 0 ? -v : v) >> Al;
        if (t == 0) { r++; continue; }
        b.e = 1;                                             // here libjpeg flushes the run before: it ended with the block before
        s.sym(0xF0, r >> 4);                                 // the run's ZRLs in one call, often none: a length sink multiplies, no branch, no loop
        r &= 15;
        const int n = js_nbits(t);
        s.sym((r << 4) | n);
        s.bits((unsigned)(v < 0 ? ~t : t) & ((1u << n) - 1), n);
        r = 0;
    }
    b.r = r;
    return b;
}

template <class Sink>
AEJ_HD inline JeBlock je_ac_refine(const short *c, int Ss, int Se, int Al, Sink &s)
{
    JeBlock b = { 0, 0, 0, 0 };
    int eob = -1, r = 0, br = 0;
    unsigned long long bb = 0;
    for (int k = Ss; k <= Se; k++) {
        const int v = c[k];
        if (((v < 0 ? -v : v) >> Al) == 1) eob = k;
    }
    for (int k = Ss; k <= Se; k++) {
        const int v = c[k], a = (v < 0 ? -v : v) >> Al;
        if (a == 0) { r++; continue; }
        while (r > 15 && k <= eob) {                         // a ZRL that cannot be folded into the end of band takes the buffered bits
            b.e = 1;
            s.sym(0xF0);
            r -= 16;
            s.many(bb, br);
            bb = 0; br = 0;
        }
        if (a > 1) {                                         // already non-zero: its next bit waits for the next symbol
            bb = (bb << 1) | (unsigned)(a & 1);
            br++;
            continue;
        }
        b.e = 1;
        s.sym((r << 4) | 1);
        s.bits(v < 0 ? 0u : 1u, 1);
        s.many(bb, br);
        bb = 0; br = 0; r = 0;
    }
    b.r = r; b.br = br; b.brbits = bb;
    return b;
}

template <class Sink>
AEJ_HD inline void je_eobrun(int run, Sink &s)              // the EOBn symbol of a piece of `run` >= 1 blocks
{
    const int n = js_nbits(run) - 1;
    s.sym(n << 4);
    if (n) s.bits((unsigned)run & ((1u << n) - 1), n);
}

// One block of a sequential scan (Annex F.1.2: baseline, and the optimised files' own tables): the DC difference against `pred`, the
// run-length walk over coefficients 1 .. 63 of c (read as je_ac_first reads them; c[0] is not read), EOB if zeros are pending.
// dc_codes / ac_codes: the block's two tables, as the sink's `codes`.
template <class Src, class Tab, class Sink>
AEJ_HD inline void je_block_seq(int dc, int pred, Src c, Tab dc_codes, Tab ac_codes, Sink &s)
{
    s.codes = dc_codes;
    je_dc_first(dc, pred, 0, s);
    s.codes = ac_codes;
    if (je_ac_first(c, 1, 63, 0, s).r) s.sym(0x00);
}

// the DC predictor of block k of MCU m in an interleaved scan (NL luma blocks of BPM per MCU, restart interval R, 0: none) over the
// coefficients `coef` of the scan's blocks in MCU order: the DC of the component's block before, 0 at the start of the scan and of
// every restart interval
AEJ_HD inline int je_dc_pred(const short *coef, int NL, int BPM, long long m, int k, int R)
{
    const long long pb = js_prev(NL, BPM, m, k);
    return pb < 0 || jr_resets(m, pb, BPM, R) ? 0 : coef[pb * 64];
}

// ---- the partition -------------------------------------------------------------------------------------------------------------------
// value of one block of an AC scan for the prefix sum: a break (the block does not continue the chain of the block before: it is the
// first of the scan, it emits, or the block before left nothing pending) and its pending correction bits
AEJ_HD inline unsigned long long je_pack(bool first, bool e, bool prev_joins, int br)
{
    return ((unsigned long long)(first || e || !prev_joins) << kJeBrShift) | (unsigned long long)br;
}
// P: exclusive prefix sums of je_pack over the n blocks of a scan, n + 1 entries (only differences are used, so P may be a window
// of a longer sum).  The chain that starts at block s ends before the first break after s.
AEJ_HD inline long long je_chain_end(const unsigned long long *P, long long s, long long n)
{
    const unsigned long long base = P[s + 1] >> kJeBrShift;
    long long lo = s + 1, hi = n;                           // the answer lies in [lo, hi]
    while (lo < hi) {
        const long long mid = lo + (hi - lo) / 2;
        if ((P[mid + 1] >> kJeBrShift) != base) hi = mid; else lo = mid + 1;
    }
    return lo;
}
// the piece that opens at block p of a chain ending before ce: -> the block after its last.  why: 1 the run reached kJeMaxRun,
// 2 more than kJeMaxDeferred bits were pending, 0 the chain ended
AEJ_HD inline long long je_piece_end(const unsigned long long *P, long long p, long long ce, int *why)
{
    const unsigned long long mask = (1ull << kJeBrShift) - 1, base = P[p] & mask;
    const bool full = ce - p >= kJeMaxRun;
    const long long lim = full ? p + kJeMaxRun : ce;
    long long lo = p, hi = lim;                             // the first j in [p, lim) with more than kJeMaxDeferred bits in p .. j, else lim
    for (long long step = 16; lo + step < hi; step *= 2) {  // gallop first: where bits are deferred at all the cut is near (from 15 blocks on)
        if ((P[lo + step] & mask) - base > (unsigned long long)kJeMaxDeferred) { hi = lo + step - 1; break; }
        lo += step;                                          // blocks p .. lo - 1 hold no cut
    }
    while (lo < hi) {
        const long long mid = lo + (hi - lo) / 2;
        if ((P[mid + 1] & mask) - base > (unsigned long long)kJeMaxDeferred) hi = mid; else lo = mid + 1;
    }
    if (lo < lim) {
        *why = (lo + 1 == lim && full) ? 1 : 2;
        return lo + 1;
    }
    *why = full ? 1 : 0;
    return lim;
}

// ---- sinks.  codes: (code << 8) | length per symbol (jh_codes); JeEmit writes through JeBits (jfif_stream_core.h)
struct JeNull {
    AEJ_HD inline void sym(int, int = 1) {}
    AEJ_HD inline void bits(unsigned, int) {}
    AEJ_HD inline void many(unsigned long long, int) {}
};
// symbol counts: T unsigned in LDS on the device (counted atomically: a wave shares one), unsigned long long on the host
template <class T>
struct JeHist {
    T *codes;
    AEJ_HD inline void sym(int s, int n = 1)
    {
        if (n == 0) return;
#if defined(__HIP_DEVICE_COMPILE__)
        atomicAdd(codes + s, (T)n);
#else
        codes[s] += (T)n;
#endif
    }
    AEJ_HD inline void bits(unsigned, int) {}
    AEJ_HD inline void many(unsigned long long, int) {}
};
struct JeLen {
    const unsigned *codes;
    int total;
    AEJ_HD inline void sym(int s, int n = 1) { total += n * (int)(codes[s] & 255); }
    AEJ_HD inline void bits(unsigned, int n) { total += n; }
    AEJ_HD inline void many(unsigned long long, int n) { total += n; }
};
struct JeEmit {
    const unsigned *codes;
    JeBits bw;
    AEJ_HD inline void sym(int s, int n = 1)
    {
        for (; n > 0; n--) bw.put(codes[s] >> 8, (int)(codes[s] & 255));
    }
    AEJ_HD inline void bits(unsigned v, int n) { bw.put(v, n); }
    AEJ_HD inline void many(unsigned long long v, int n)
    {
        if (n > 32) {
            bw.put((unsigned)(v >> 32), n - 32);
            n = 32;
        }
        bw.put((unsigned)(v & 0xFFFFFFFFull), n);
    }
};

}  // namespace aej
