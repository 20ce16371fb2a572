// inflate.hip -- zlib (RFC 1950 / 1951) decoder for many streams at once: the device half of Jpeg.decompress_many's entropy stage.
//
// One wave64 per stream.  The decode itself is serial (one symbol after another, the bit buffer and all decoder state wave-uniform); the
// lanes share the parallel parts: building the Huffman lookup tables, copying matches 64 bytes per step, and the stores to global memory,
// which leave in whole-wave 256-byte pieces.  The 32 KiB window is a ring in LDS, so a match never reads back what this wave has just
// stored to global memory.  Every loop is bounded by the stream's input length or its output capacity: a corrupt stream ends with a
// status, never a hang or a write outside [out_off, out_off + out_cap).
#include "aej_launch.h"

namespace aej {

namespace {

constexpr int kWin = 32768;            // RFC 1951 window; the ring holds exactly this many bytes
constexpr int kFastBits = 10;          // first-level lookup: codes of up to 10 bits in one LDS read
constexpr int kFlush = 256;            // bytes per whole-wave store (64 lanes x 4)

// status values (include/aej.h, AEJ_INFLATE_*)
enum { kOk = 0, kBadHeader = 1, kBadBlockType = 2, kBadCodeLengths = 3, kBadSymbol = 4, kTooFar = 5, kStoredLen = 6,
       kTruncated = 7, kOverCapacity = 8, kAdler = 9, kBadArg = 10 };

__constant__ unsigned short kLenBase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163,
                                            195, 227, 258};
__constant__ unsigned char kLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__constant__ unsigned short kDistBase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049,
                                             3073, 4097, 6145, 8193, 12289, 16385, 24577};
__constant__ unsigned char kDistExtra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
__constant__ unsigned char kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// A canonical Huffman code in LDS: the first-level table (entry = len << 9 | symbol, 0 = longer code or no code), the number of codes of
// each length and the symbols sorted by (length, value) -- the slow path for codes longer than kFastBits (puff.c's decode).
template <int NSYM>
struct Huff {
    unsigned short fast[1 << kFastBits];
    unsigned short count[16];
    unsigned short offs[16];     // build scratch
    unsigned short sym[NSYM];
};

struct InflateLds {
    unsigned char ring[kWin];
    Huff<288> lit;
    Huff<32> dist;          // also the code-length code while a dynamic header is read
    unsigned char lens[320];
    int err;                // result of the lane-0 part of a table build
};

// Wave-uniform LSB-first bit reader.  Bytes past the end read as zero; `overrun()` says whether any of them has been consumed.
struct Bits {
    const unsigned char *p;
    long long len, pos;
    unsigned long long buf;
    int cnt;

    __device__ void refill()
    {
        if (cnt > 56) return;
        if (pos + 8 <= len) {
            // two aligned dword loads give at least 5 bytes from `pos` on (the stream base is 4-byte aligned: aej_inflate_batch checks)
            long long a = pos & ~3LL;
            int sh = (int)(pos & 3) * 8;
            const unsigned *w = reinterpret_cast<const unsigned *>(p + a);
            unsigned long long v = (((unsigned long long)w[1] << 32) | w[0]) >> sh;
            int take = (64 - cnt) >> 3, avail = (64 - sh) >> 3;
            if (take > avail) take = avail;
            if (take < 8) v &= (1ull << (8 * take)) - 1;
            buf |= v << cnt;
            cnt += 8 * take;
            pos += take;
            return;
        }
        while (cnt <= 56) {
            unsigned long long b = pos < len ? p[pos] : 0;
            pos++;
            buf |= b << cnt;
            cnt += 8;
        }
    }
    __device__ unsigned get(int n)
    {
        refill();
        unsigned v = (unsigned)(buf & ((1ull << n) - 1));
        buf >>= n;
        cnt -= n;
        return v;
    }
    __device__ bool overrun() const { return pos * 8 - cnt > len * 8; }
};

// Canonical decode of the bits `v` (LSB first) with at most `maxlen` bits: -> len << 9 | symbol, or 0 when no code of <= maxlen bits matches.
template <int NSYM>
__device__ unsigned slow_decode(const Huff<NSYM> &h, unsigned v, int maxlen)
{
    int code = 0, first = 0, index = 0;
    for (int len = 1; len <= maxlen; len++) {
        code |= (v >> (len - 1)) & 1;
        int count = h.count[len];
        if (code - count < first) return ((unsigned)len << 9) | h.sym[index + (code - first)];
        index += count;
        first += count;
        first <<= 1;
        code <<= 1;
    }
    return 0;
}

// Build a code from lens[0..n).  kind 0: literal / length or distance code, 1: the code-length code.  Validity as zlib's inflate_table
// judges it: over-subscribed is an error; incomplete is an error except for a literal / distance code whose longest code has one bit,
// and an empty literal / distance code is allowed (decoding from it fails).  Returns 0 or kBadCodeLengths.  All lanes call it.
template <int NSYM>
__device__ int build_huff(Huff<NSYM> &h, const unsigned char *lens, int n, int kind, int *err)
{
    const int lane = threadIdx.x;
    if (lane == 0) {
        for (int l = 0; l < 16; l++) h.count[l] = 0;
        for (int s = 0; s < n; s++) h.count[lens[s]]++;
        h.count[0] = 0;
        int left = 1, max = 0, bad = 0;
        for (int l = 1; l < 16; l++) {
            left <<= 1;
            left -= h.count[l];
            if (left < 0) bad = 1;
            if (h.count[l]) max = l;
        }
        if (!bad && max == 0 && kind == 1) bad = 1;
        if (!bad && max > 0 && left > 0 && (kind == 1 || max != 1)) bad = 1;
        if (!bad) {
            h.offs[1] = 0;
            for (int l = 1; l < 15; l++) h.offs[l + 1] = h.offs[l] + h.count[l];
            for (int s = 0; s < n; s++)
                if (lens[s]) h.sym[h.offs[lens[s]]++] = (unsigned short)s;
        }
        *err = bad;
    }
    __syncthreads();
    if (*err) return kBadCodeLengths;
    for (int e = lane; e < (1 << kFastBits); e += 64) h.fast[e] = (unsigned short)slow_decode(h, (unsigned)e, kFastBits);
    __syncthreads();
    return 0;
}

template <int NSYM>
__device__ __forceinline__ unsigned decode_sym(const Huff<NSYM> &h, Bits &in)
{
    in.refill();
    unsigned e = h.fast[in.buf & ((1u << kFastBits) - 1)];
    if (!e) e = slow_decode(h, (unsigned)(in.buf & 0x7fff), 15);
    if (e) {
        int len = e >> 9;
        in.buf >>= len;
        in.cnt -= len;
    }
    return e;       // 0: no symbol
}

struct Out {
    unsigned char *dst;          // the stream's first output byte (4-byte aligned)
    long long cap, pos, flushed;
    unsigned a, b;               // Adler-32 halves
};

// Adler-32 of `n` bytes held 4 per lane (lane k: bytes 4k .. 4k+3 of the piece), appended to (a, b).
__device__ void adler_piece(Out &o, unsigned word, int n)
{
    const int lane = threadIdx.x;
    unsigned s = 0, ws = 0;
    for (int j = 0; j < 4; j++) {
        int i = 4 * lane + j;
        unsigned c = i < n ? (word >> (8 * j)) & 0xff : 0;
        s += c;
        ws += (unsigned)(n - i) * c;
    }
    s = (unsigned)wave_total((int)s);
    ws = (unsigned)wave_total((int)ws);
    o.b = (o.b + (unsigned)n * o.a + ws) % 65521u;
    o.a = (o.a + s) % 65521u;
}

// Store the ring's bytes [flushed, flushed + 256) to global memory, one dword per lane.
__device__ void flush_full(InflateLds &L, Out &o)
{
    const int lane = threadIdx.x;
    unsigned w = *reinterpret_cast<const unsigned *>(&L.ring[(o.flushed + 4 * lane) & (kWin - 1)]);
    *reinterpret_cast<unsigned *>(o.dst + o.flushed + 4 * lane) = w;
    adler_piece(o, w, kFlush);
    o.flushed += kFlush;
}

__device__ __forceinline__ void flush_ready(InflateLds &L, Out &o)
{
    while (o.pos - o.flushed >= kFlush) flush_full(L, o);
}

// The last, partial piece (fewer than 256 bytes): byte stores.
__device__ void flush_tail(InflateLds &L, Out &o)
{
    const int lane = threadIdx.x;
    int n = (int)(o.pos - o.flushed);
    unsigned w = *reinterpret_cast<const unsigned *>(&L.ring[(o.flushed + 4 * lane) & (kWin - 1)]);
    for (int j = 0; j < 4; j++)
        if (4 * lane + j < n) o.dst[o.flushed + 4 * lane + j] = (unsigned char)(w >> (8 * j));
    adler_piece(o, w, n);
    o.flushed += n;
}

__device__ int inflate_one(InflateLds &L, Bits &in, Out &o)
{
    const int lane = threadIdx.x;
    if (in.len < 2) return kTruncated;
    unsigned cmf = in.get(8), flg = in.get(8);
    if ((cmf & 15) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31 != 0 || (flg & 0x20)) return kBadHeader;
    for (;;) {
        unsigned hdr = in.get(3);
        if (in.overrun()) return kTruncated;
        unsigned type = hdr >> 1;
        if (type == 0) {
            // stored: to the byte boundary, LEN / NLEN, then LEN raw bytes straight from the input
            in.get(in.cnt & 7);
            unsigned len = in.get(16), nlen = in.get(16);
            if (in.overrun()) return kTruncated;
            if ((len ^ 0xffffu) != nlen) return kStoredLen;
            long long src = in.pos - in.cnt / 8;          // the bit buffer holds whole bytes now: give them back
            in.pos = src;
            in.buf = 0;
            in.cnt = 0;
            if (src + len > in.len) return kTruncated;
            if (o.pos + len > o.cap) return kOverCapacity;
            for (unsigned done = 0; done < len; done += 64) {
                if (done + lane < len) L.ring[(o.pos + lane) & (kWin - 1)] = in.p[src + done + lane];
                o.pos += len - done < 64 ? len - done : 64;
                flush_ready(L, o);
            }
            in.pos = src + len;
        } else if (type == 1 || type == 2) {
            if (type == 1) {
                if (lane == 0) {
                    for (int s = 0; s < 288; s++) L.lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
                    for (int s = 0; s < 32; s++) L.lens[288 + s] = 5;
                }
                __syncthreads();
                build_huff(L.lit, L.lens, 288, 0, &L.err);
                build_huff(L.dist, L.lens + 288, 32, 0, &L.err);
            } else {
                int hlit = (int)in.get(5) + 257, hdist = (int)in.get(5) + 1, hclen = (int)in.get(4) + 4;
                if (in.overrun()) return kTruncated;
                if (hlit > 286 || hdist > 30) return kBadCodeLengths;
                if (lane == 0)
                    for (int s = 0; s < 19; s++) L.lens[s] = 0;
                __syncthreads();
                for (int i = 0; i < hclen; i++) {
                    unsigned v = in.get(3);
                    if (lane == 0) L.lens[kClOrder[i]] = (unsigned char)v;
                }
                __syncthreads();
                if (in.overrun()) return kTruncated;
                if (build_huff(L.dist, L.lens, 19, 1, &L.err)) return kBadCodeLengths;
                // the code lengths of both codes; lens[] is rewritten from index 0 on, past the 19 the code-length code was built from
                int n = 0, total = hlit + hdist;
                unsigned char prev = 0;
                while (n < total) {
                    unsigned e = decode_sym(L.dist, in);
                    if (in.overrun()) return kTruncated;
                    if (!e) return kBadCodeLengths;
                    int s = e & 511;
                    if (s < 16) {
                        if (lane == 0) L.lens[n] = (unsigned char)s;
                        prev = (unsigned char)s;
                        n++;
                        continue;
                    }
                    int rep;
                    unsigned char val = 0;
                    if (s == 16) {
                        if (n == 0) return kBadCodeLengths;
                        val = prev;
                        rep = 3 + (int)in.get(2);
                    } else if (s == 17) {
                        rep = 3 + (int)in.get(3);
                    } else {
                        rep = 11 + (int)in.get(7);
                    }
                    if (in.overrun()) return kTruncated;
                    if (n + rep > total) return kBadCodeLengths;
                    for (int i = lane; i < rep; i += 64) L.lens[n + i] = val;
                    prev = val;
                    n += rep;
                }
                __syncthreads();
                if (L.lens[256] == 0) return kBadCodeLengths;
                if (build_huff(L.lit, L.lens, hlit, 0, &L.err)) return kBadCodeLengths;
                if (build_huff(L.dist, L.lens + hlit, hdist, 0, &L.err)) return kBadCodeLengths;
            }
            for (;;) {
                unsigned e = decode_sym(L.lit, in);
                if (in.overrun()) return kTruncated;
                if (!e) return kBadSymbol;
                int s = e & 511;
                if (s < 256) {
                    if (o.pos >= o.cap) return kOverCapacity;
                    if (lane == 0) L.ring[o.pos & (kWin - 1)] = (unsigned char)s;
                    o.pos++;
                    flush_ready(L, o);
                    continue;
                }
                if (s == 256) break;
                s -= 257;
                if (s >= 29) return kBadSymbol;
                int len = kLenBase[s] + (int)in.get(kLenExtra[s]);
                unsigned d = decode_sym(L.dist, in);
                if (in.overrun()) return kTruncated;
                if (!d) return kBadSymbol;
                int ds = d & 511;
                if (ds >= 30) return kBadSymbol;
                int dist = kDistBase[ds] + (int)in.get(kDistExtra[ds]);
                if (in.overrun()) return kTruncated;
                if (dist > o.pos) return kTooFar;
                if (o.pos + len > o.cap) return kOverCapacity;
                // lane k copies byte k of each 64-byte step; for dist < 64 the source repeats with period dist
                const int rel = lane % dist;
                for (int done = 0; done < len; done += 64) {
                    long long p = o.pos + done;
                    unsigned char v = L.ring[(p - dist + rel) & (kWin - 1)];
                    if (done + lane < len) L.ring[(p + lane) & (kWin - 1)] = v;
                }
                o.pos += len;
                flush_ready(L, o);
            }
        } else {
            return kBadBlockType;
        }
        if (hdr & 1) break;          // BFINAL
    }
    // Adler-32 trailer, big-endian, on the next byte boundary
    in.get(in.cnt & 7);
    unsigned t = in.get(8) << 24;
    t |= in.get(8) << 16;
    t |= in.get(8) << 8;
    t |= in.get(8);
    if (in.overrun()) return kTruncated;
    flush_tail(L, o);
    if (t != ((o.b << 16) | o.a)) return kAdler;
    return kOk;
}

__global__ __launch_bounds__(64) void inflate_kernel(const unsigned char *__restrict__ src, const long long *__restrict__ desc, int n,
                                                     unsigned char *__restrict__ dst, long long dst_bytes, long long *__restrict__ out_bytes,
                                                     int *__restrict__ status)
{
    __shared__ InflateLds L;
    const int i = blockIdx.x;
    if (i >= n) return;
    const long long in_off = desc[4 * i], in_len = desc[4 * i + 1], out_off = desc[4 * i + 2], out_cap = desc[4 * i + 3];
    int st;
    Out o{};
    o.a = 1;
    if (in_off < 0 || in_len < 0 || (in_off & 3) || out_off < 0 || out_cap < 0 || (out_off & 3) || out_off + out_cap > dst_bytes) {
        st = kBadArg;
    } else {
        Bits in{src + in_off, in_len, 0, 0, 0};
        o.dst = dst + out_off;
        o.cap = out_cap;
        st = inflate_one(L, in, o);
        if (st != kOk) {
            // what was decoded before the error reached the ring only; nothing past `flushed` is stored (all of it lies inside the capacity)
            o.pos = o.flushed;
        }
    }
    if (threadIdx.x == 0) {
        out_bytes[i] = o.pos;
        status[i] = st;
    }
}

}  // namespace

void launch_inflate(hipStream_t st, const unsigned char *src, const long long *desc, int n, unsigned char *dst, long long dst_bytes,
                    long long *out_bytes, int *status)
{
    if (n > 0) hipLaunchKernelGGL(inflate_kernel, dim3(n), dim3(64), 0, st, src, desc, n, dst, dst_bytes, out_bytes, status);
}

}  // namespace aej
