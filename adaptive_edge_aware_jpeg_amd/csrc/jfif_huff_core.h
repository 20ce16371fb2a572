// jfif_huff_core.h -- one optimal Huffman table from the counts of its symbols (T.81 Annex K.2 as libjpeg's jpeg_gen_optimal_table does
// it), written as a host + device function so that aej_jfif_huffman_host runs the code k_jfif_tables (jfif.hip) runs.  The caller
// supplies the work arrays (LDS on the device, the stack on the host); nothing here indexes a private array dynamically.
#pragma once
#include <stdint.h>

#ifndef AEJ_HD
#define AEJ_HD __host__ __device__
#endif

namespace aej {

constexpr int kJhSymbols = 257;        // 256 symbols and the reserved one that keeps the all-ones code out of the table
constexpr int kJhMaxLen = 96;          // code lengths before the adjustment to 16: counts that sum below 2^63 stay below 92

struct JhWork {
    long long freq[kJhSymbols];
    short codesize[kJhSymbols], others[kJhSymbols];
    int nlen[kJhMaxLen + 1];           // codes of every length
};

// freq[0..255] hold the counts (>= 0, not all zero).  -> number of symbols; bits[0..15] = BITS[1..16]; huffval[0..n-1] sorted by
// code length, then value.  Ties between equal counts go to the larger symbol index.
AEJ_HD inline int jh_build(JhWork &w, unsigned char *bits, unsigned char *huffval)
{
    w.freq[256] = 1;
    for (int i = 0; i < kJhSymbols; i++) { w.codesize[i] = 0; w.others[i] = -1; }
    for (int i = 0; i <= kJhMaxLen; i++) w.nlen[i] = 0;
    for (;;) {
        int c1 = -1, c2 = -1;
        long long v = INT64_MAX;
        for (int i = 0; i < kJhSymbols; i++)
            if (w.freq[i] && w.freq[i] <= v) { v = w.freq[i]; c1 = i; }
        v = INT64_MAX;
        for (int i = 0; i < kJhSymbols; i++)
            if (w.freq[i] && w.freq[i] <= v && i != c1) { v = w.freq[i]; c2 = i; }
        if (c2 < 0) break;
        w.freq[c1] += w.freq[c2];
        w.freq[c2] = 0;
        w.codesize[c1]++;                                    // every symbol of both trees moves one level down
        while (w.others[c1] >= 0) { c1 = w.others[c1]; w.codesize[c1]++; }
        w.others[c1] = (short)c2;                            // and c2's chain is appended to c1's
        w.codesize[c2]++;
        while (w.others[c2] >= 0) { c2 = w.others[c2]; w.codesize[c2]++; }
    }
    int longest = 0;
    for (int i = 0; i < kJhSymbols; i++) {
        const int n = w.codesize[i] < kJhMaxLen ? w.codesize[i] : kJhMaxLen;
        if (n) w.nlen[n]++;
        longest = n > longest ? n : longest;
    }
    for (int i = longest; i > 16; i--)                       // K.3: move pairs of the longest codes up until none exceeds 16 bits
        while (w.nlen[i] > 0) {
            int j = i - 2;
            while (w.nlen[j] == 0) j--;
            w.nlen[i] -= 2;
            w.nlen[i - 1]++;
            w.nlen[j + 1] += 2;
            w.nlen[j]--;
        }
    int i = 16;
    while (i > 0 && w.nlen[i] == 0) i--;
    if (i > 0) w.nlen[i]--;                                  // the reserved symbol leaves the longest length in use
    for (int k = 0; k < 16; k++) bits[k] = (unsigned char)w.nlen[k + 1];
    int p = 0;
    for (int n = 1; n <= longest; n++)
        for (int j = 0; j < 256; j++)
            if (w.codesize[j] == n) huffval[p++] = (unsigned char)j;
    return p;
}

// (code << 8) | length of every symbol of a (BITS, HUFFVAL) table into codes[256] (Annex C); symbols not in the table keep 0
AEJ_HD inline void jh_codes(const unsigned char *bits, const unsigned char *huffval, unsigned *codes)
{
    unsigned code = 0;
    int k = 0;
    for (int len = 1; len <= 16; len++) {
        for (int n = 0; n < bits[len - 1]; n++) codes[huffval[k++]] = (code++ << 8) | (unsigned)len;
        code <<= 1;
    }
}

}  // namespace aej
