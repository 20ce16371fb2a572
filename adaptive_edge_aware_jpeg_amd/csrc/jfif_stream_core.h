// jfif_stream_core.h -- what every standard-JPEG stream writer and reader here shares, written once: the byte swap and magnitude category,
// the big-endian bit writer, 0xFF counting and stuffing of a byte range, the predecessor of a block in an interleaved scan, and the
// segmented prefix-sum kernel.  jfif.hip (baseline, optimised), jfifprog.hip (progressive) and through them the ragged encoder, the
// transcoder and the transforms write their streams with these; the decoders' bit windows take js_bswap.  Host + device where the host
// testing entries step through the same text (aej_test_jfif_seq_scan_host, aej_test_jfif_prog_scan_host).  Every piece must stay
// bit-exact with libjpeg-turbo: the Pillow byte-for-byte suites (tests/test_gpu_jfif*.py) pin all callers at once.
// Who includes what: jfif_restart_core.h (restart index rules, an item's place in its interval, the stuffing copy with markers) includes
// this file; jfif_prog_core.h (the block coders je_block_seq / je_dc_* / je_ac_*, their sinks, the DC predictor) includes both; jfif.hip
// and jfifprog.hip include all three, api_jpeg.hip this file and jfif_restart_core.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef AEJ_HD
#define AEJ_HD __host__ __device__
#endif

namespace aej {

constexpr int kJsScanThreads = 1024;

AEJ_HD inline unsigned js_bswap(unsigned v) { return __builtin_bswap32(v); }

// magnitude category of a coefficient or difference: the bits of |v| (0 for 0)
AEJ_HD inline int js_nbits(int v)
{
    const unsigned a = v < 0 ? 0u - (unsigned)v : (unsigned)v;
    return a ? 32 - __builtin_clz(a) : 0;
}

// interleaved scan of MCUs of BPM blocks, the first NL of them luma in raster order, then one per chroma component: the block of the
// same component before block k of MCU m in scan order, -1 at the start of the scan
AEJ_HD inline long long js_prev(int NL, int BPM, long long m, int k)
{
    if (k >= 1 && k < NL) return m * BPM + k - 1;
    if (m == 0) return -1;
    return (m - 1) * BPM + (k == 0 ? NL - 1 : k);
}

// ---- 0xFF stuffing of the bytes [lo, hi) of a stream: how many 0x00 they gain, and the copy that carries them
AEJ_HD inline int js_stuff_count(const unsigned char *src, long long lo, long long hi)
{
    int n = 0;
    for (long long i = lo; i < hi; i++) n += src[i] == 0xFF;
    return n;
}
AEJ_HD inline void js_stuff_copy(unsigned char *dst, const unsigned char *src, long long lo, long long hi)
{
    for (long long i = lo; i < hi; i++) {
        const unsigned char v = src[i];
        *dst++ = v;
        if (v == 0xFF) *dst++ = 0;
    }
}

// ---- big-endian bit writer into zeroed 32-bit words (stream byte order in memory); on the device words shared with neighbouring
// blocks are ORed in atomically; stores beyond `limit` words are dropped
struct JeBits {
    unsigned *w;
    long long wi, limit;
    unsigned long long acc;
    int n;
    AEJ_HD JeBits(unsigned *words, long long pos, long long lim) : w(words), wi(pos >> 5), limit(lim), acc(0), n((int)(pos & 31)) {}
    AEJ_HD inline void word(unsigned v)
    {
        if (v != 0 && wi < limit) {                          // the words start as 0: an item that writes no bit touches no memory
#if defined(__HIP_DEVICE_COMPILE__)
            atomicOr(w + wi, js_bswap(v));
#else
            w[wi] |= js_bswap(v);
#endif
        }
        wi++;
    }
    AEJ_HD inline void put(unsigned code, int len)          // len <= 32, code < 2^len
    {
        if (len == 0) return;
        acc = (acc << len) | code;
        n += len;
        if (n >= 32) {
            n -= 32;
            word((unsigned)(acc >> n));
            acc &= (1ull << n) - 1;
        }
    }
    AEJ_HD inline void pad_ones(long long total_bits)       // after the last bit of a byte-aligned run of total_bits bits: 1-bits up to its last byte's end
    {
        const int pad = (int)((8 - (total_bits & 7)) & 7);
        put((1u << pad) - 1, pad);
    }
    AEJ_HD inline void finish()
    {
        if (n > 0) word((unsigned)(acc << (32 - n)));
    }
};

// ---- exclusive prefix sums of n values per segment, one workgroup of kJsScanThreads per segment -> n + 1 entries, the last one the
// segment's total.  In: value i of the whole launch (segment seg holds [seg * n, seg * n + n)) as unsigned 64-bit; JsInts reads int32.
// Tiles of kJsScanThreads values: coalesced loads, a shuffle scan per wave, the waves' sums through LDS.
struct JsInts {
    const int *v;
    __device__ __forceinline__ unsigned long long operator()(long long i) const { return (unsigned long long)v[i]; }
};
template <class In>
__global__ __launch_bounds__(kJsScanThreads) void k_js_scan(In in, long long n, unsigned long long *__restrict__ out)
{
    constexpr int kWaves = kJsScanThreads / 64;
    __shared__ unsigned long long wsum[2][kWaves];
    const long long seg = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long carry = 0;
    unsigned long long *dst = out + seg * (n + 1);
    int par = 0;
    for (long long base = 0; base < n; base += kJsScanThreads, par ^= 1) {
        const long long i = base + threadIdx.x;
        const unsigned long long v = i < n ? in(seg * n + i) : 0;
        unsigned long long x = v;
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (lane == 63) wsum[par][wave] = x;
        __syncthreads();                                     // wsum alternates, so one barrier per tile is enough
        unsigned long long before = 0, all = 0;
        for (int w = 0; w < kWaves; w++) {
            const unsigned long long t = wsum[par][w];
            before += w < wave ? t : 0;
            all += t;
        }
        if (i < n) dst[i] = carry + before + x - v;
        carry += all;
    }
    if (threadIdx.x == 0) dst[n] = carry;
}

}  // namespace aej
