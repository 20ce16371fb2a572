// jfif_restart_core.h -- the index rules of restart markers (DRI / RSTn) as libjpeg's encoders apply them, written once, host + device,
// in the way of jfif_many_core.h: the baseline chain (jfif.hip), the progressive chain (jfifprog.hip) and the host entry
// aej_jfif_restart_map_host step through this text.
//
// A scan's restart interval R counts MCUs of that scan (0: no restarts).  The scan's MCUs fall into ceil(n / R) intervals of R MCUs, the
// last one shorter; before the first MCU of interval k >= 1 the coder flushes what is pending, pads the byte with 1-bits, writes the
// marker FF D0 + ((k - 1) & 7) and sets every DC predictor to 0.  The writers here keep every interval byte-aligned in the unstuffed
// stream (its bytes are ceil(bits / 8), the last block pads) and never store a marker there: a prefix sum over the intervals' byte
// lengths gives their starts, and the scatter that stuffs 0xFF bytes inserts each marker before its interval's first byte.  Where an
// item (a block of a scan) lands in such a stream (jr_place) and the stuffing copy of a chunk of it (jr_stuff_chunk) are here as well:
// both chains' emit and scatter kernels and the host entry aej_test_jfif_seq_scan_host call them.
#pragma once
#include <stdint.h>

#include "jfif_stream_core.h"

namespace aej {

constexpr int kJrMaxInterval = 65535;  // a DRI segment holds 16 bits
constexpr int kJrDriBytes = 6;         // FF DD 00 04 Rhi Rlo

// R of a scan whose rows hold per_row MCUs: rows > 0 overrides blocks and is clamped, as libjpeg's per-scan set-up does
AEJ_HD inline int jr_interval(int blocks, int rows, long long per_row)
{
    if (rows > 0) {
        const long long r = rows * per_row;
        return r > kJrMaxInterval ? kJrMaxInterval : (int)r;
    }
    return blocks;
}
// intervals of a scan of n MCUs (R > 0)
AEJ_HD inline long long jr_count(long long n, int R) { return (n + R - 1) / R; }
// the interval of MCU m (R > 0)
AEJ_HD inline long long jr_interval_of(long long m, int R) { return m / R; }
// js_prev's answer pb for a block of MCU m, bpm blocks per MCU: is the predictor 0 because that block lies in an earlier interval?
// (pb is a block of MCU m or of MCU m - 1, so it is earlier exactly when it is not of m and m opens an interval)
AEJ_HD inline bool jr_resets(long long m, long long pb, int bpm, int R) { return R > 0 && pb >= 0 && pb / bpm != m && m % R == 0; }
// second byte of the marker before interval k >= 1
AEJ_HD inline int jr_marker(long long k) { return 0xD0 + (int)((k - 1) & 7); }
// write the DRI segment of interval R at o
AEJ_HD inline void jr_dri(unsigned char *o, int R)
{
    o[0] = 0xFF; o[1] = 0xDD; o[2] = 0; o[3] = 4; o[4] = (unsigned char)(R >> 8); o[5] = (unsigned char)(R & 255);
}

// starts: niv + 1 increasing byte positions, starts[k] - starts[0] the first byte of interval k in the scan's unstuffed stream (every
// interval holds at least one byte, so they increase strictly).  -> the first k in [1, niv] whose interval starts at or after byte p
// (niv: none does).  The markers before byte p are those of intervals 1 .. jr_first_from(p + 1) - 1, so a chunk that starts at byte lo
// lies 2 (jr_first_from(lo) - 1) bytes further on, and the marker of an interval that starts inside the chunk is written with it.
AEJ_HD inline long long jr_first_from(const unsigned long long *starts, long long niv, long long p)
{
    long long lo = 1, hi = niv;
    while (lo < hi) {
        const long long mid = lo + (hi - lo) / 2;
        if ((long long)(starts[mid] - starts[0]) >= p) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// js_stuff_copy of the bytes [lo, hi) with the markers that fall among them; k = jr_first_from(starts, niv, lo); dst is where byte lo
// goes once the 0x00 bytes and the 2 (k - 1) marker bytes before it are counted.  Many boundaries may fall in the range, or none.
AEJ_HD inline void jr_stuff_copy(unsigned char *dst, const unsigned char *src, long long lo, long long hi, const unsigned long long *starts,
                                 long long niv, long long k)
{
    for (long long i = lo; i < hi; i++) {
        if (k < niv && (long long)(starts[k] - starts[0]) == i) {
            *dst++ = 0xFF;
            *dst++ = (unsigned char)jr_marker(k);
            k++;
        }
        const unsigned char v = src[i];
        *dst++ = v;
        if (v == 0xFF) *dst++ = 0;
    }
}

// the bytes [lo, hi) of a scan's unstuffed stream with a 0x00 after every 0xFF, and with the scan's markers if it has intervals (niv > 0;
// starts as above); dst is where byte lo goes once the 0x00 bytes before it are counted -- the marker bytes before it are counted here
AEJ_HD inline void jr_stuff_chunk(unsigned char *dst, const unsigned char *src, long long lo, long long hi, const unsigned long long *starts,
                                  long long niv)
{
    if (niv == 0) {
        js_stuff_copy(dst, src, lo, hi);
        return;
    }
    const long long k = jr_first_from(starts, niv, lo);
    jr_stuff_copy(dst + 2 * (k - 1), src, lo, hi, starts, niv, k);
}

// Item i of a scan of n items whose restart intervals hold `per` items each (the last one fewer).  P: the scan's n + 1 exclusive prefix
// sums of the items' bits, starts: the byte starts of its intervals (both may be windows of longer sums: only differences are used)
// -> the item's bit position in the scan's stream of byte-aligned intervals, the bits of its interval, whether it is the interval's last
struct JrPlace {
    long long pos, total;
    bool last;
};
AEJ_HD inline JrPlace jr_place(long long i, long long per, long long n, const unsigned long long *P, const unsigned long long *starts)
{
    const long long iv = i / per, lo = iv * per, hi = lo + per < n ? lo + per : n;
    return JrPlace{ 8 * (long long)(starts[iv] - starts[0]) + (long long)(P[i] - P[lo]), (long long)(P[hi] - P[lo]), i == hi - 1 };
}

}  // namespace aej
