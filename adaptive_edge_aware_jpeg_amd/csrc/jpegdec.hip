// jpegdec.hip -- baseline JPEG files decoded on the device, pixel-identical to Pillow with libjpeg-turbo (aej_jpegdec_*, include/aej.h).
// The host reads the markers up to SOS (aej_jpegdec_parse_host); everything after that runs here, one launch per stage over the whole call:
//   k_jd_count      one thread per 64-byte chunk of a scan: data bytes, RSTn markers and whether the scan ends in it (jd_byte_class)
//   k_jd_scan_chunks one workgroup per file: exclusive scan of those counts, the clean length; restart-marker count check
//   k_jd_scatter    one thread per chunk: the chunk's data bytes at their place in the clean stream (0x00 after 0xFF removed), the start
//                   of the restart segment after each RSTn, RSTn numbers checked
//   k_jd_segments   one thread per restart segment: its bit length, subsequences of S bits and their slots
//   k_jd_init       one thread per subsequence slot: Huffman decode from a guessed state (the exact one for a segment's first
//                   subsequence) up to the first symbol boundary at or past the subsequence's end; exit state, blocks started, DC sums
//   k_jd_sync       the same from the predecessor's exit state, for slots whose entry changed; relaunched by the host (no workgroup
//                   waits on another) until a round changes nothing -- that fixed point is the sequential decode.  A round that finds
//                   the previous one changed nothing returns at once.
//   k_jd_scan_slots one workgroup per file: block and DC-sum prefixes over the subsequences, restarting at every segment
//   k_jd_write      one thread per slot: the decode again, now storing coefficients and DC values (prefix + own differences); errors of
//                   blocks the segment needs, and a segment that ends before its last block, go to the file's status
//   k_jd_idct       one thread per real block: dequantise, islow IDCT, range limit -> sample planes
//   k_jd_rgb        one thread per pixel: up-sampling (h2v2 / h2v1 fancy, replication when the chroma is <= 2 wide) and YCbCr -> RGB
// Bounds: every index derives from the host-computed JdFile layout; a file's reads stay inside its scan and its clean stream, decode loops
// are bounded by their subsequence's bits, and coefficient writes by the segment's block count.
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "aej_common.h"
#include "aej_launch.h"

namespace aej {

constexpr int kJdThreads = 256;
constexpr int kJdScanThreads = 1024;

// index i of the last element with (base array member) <= t, over n files
template <long long JdFile::*M>
__device__ __forceinline__ int jd_find_file(const JdFile *f, int n, long long t)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (f[mid].*M <= t) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ int jd_find_seg(const JdSeg *s, int n, long long t)      // last segment whose slot_base <= t
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (s[mid].slot_base <= t) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ void jd_fail(int *status, int f, int code) { atomicCAS(status + f, 0, code); }

// ---- un-stuffing ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kJdThreads) void k_jd_count(const JdFile *__restrict__ files, int n, long long n_chunks, const unsigned char *__restrict__ scans,
                                                         int *__restrict__ cnt)
{
    const long long idx = (long long)blockIdx.x * kJdThreads + threadIdx.x;
    if (idx >= n_chunks) return;
    const int f = jd_find_file<&JdFile::chunk_base>(files, n, idx);
    const JdFile &F = files[f];
    const unsigned char *s = scans + F.scan_off;
    const long long lo = (idx - F.chunk_base) * kJdChunk, hi = min(F.scan_len, lo + kJdChunk);
    int data = 0, rst = 0, end = 0;
    for (long long p = lo; p < hi; p++) {
        const int c = jd_byte_class(s, F.scan_len, p);
        if (c == kJdByteEnd) { end = 1; break; }
        data += c == kJdByteData;
        rst += c == kJdByteRst;
    }
    cnt[idx * 3] = data;
    cnt[idx * 3 + 1] = rst;
    cnt[idx * 3 + 2] = end;
}

// exclusive scan of 3 values over [0, m) by one workgroup (each thread walks a contiguous range, a Hillis-Steele scan joins them)
__global__ __launch_bounds__(kJdScanThreads) void k_jd_scan_chunks(const JdFile *__restrict__ files, const aej_jpegdec_desc *__restrict__ descs,
                                                                   const int *__restrict__ cnt, long long *__restrict__ pre, long long *__restrict__ clean_len,
                                                                   JdSeg *__restrict__ segs, int *__restrict__ status)
{
    __shared__ long long sh[3][kJdScanThreads];
    const int f = blockIdx.x;
    const JdFile &F = files[f];
    const long long m = F.n_chunks, per = (m + kJdScanThreads - 1) / kJdScanThreads;
    const long long lo = min(m, threadIdx.x * per), hi = min(m, lo + per);
    const int *c = cnt + F.chunk_base * 3;
    long long a[3] = { 0, 0, 0 };
    for (long long i = lo; i < hi; i++)
        for (int v = 0; v < 3; v++) a[v] += c[i * 3 + v];
    for (int v = 0; v < 3; v++) sh[v][threadIdx.x] = a[v];
    __syncthreads();
    for (int off = 1; off < kJdScanThreads; off <<= 1) {
        long long t[3];
        for (int v = 0; v < 3; v++) t[v] = threadIdx.x >= off ? sh[v][threadIdx.x - off] : 0;
        __syncthreads();
        for (int v = 0; v < 3; v++) sh[v][threadIdx.x] += t[v];
        __syncthreads();
    }
    long long run[3];
    for (int v = 0; v < 3; v++) run[v] = sh[v][threadIdx.x] - a[v];
    long long *o = pre + F.chunk_base * 3;
    for (long long i = lo; i < hi; i++) {
        for (int v = 0; v < 3; v++) o[i * 3 + v] = run[v];
        if (run[2] == 0 && c[i * 3 + 2]) {            // the chunk where the scan ends: clean length and restart count
            clean_len[f] = run[0] + c[i * 3];
            if (run[1] + c[i * 3 + 1] != descs[f].n_segments - 1) jd_fail(status, f, AEJ_JPEGDEC_BAD_RESTART);
        }
        for (int v = 0; v < 3; v++) run[v] += c[i * 3 + v];
    }
    if (threadIdx.x == kJdScanThreads - 1 && sh[2][kJdScanThreads - 1] == 0) {      // no marker after the data: the scan runs to the end
        clean_len[f] = sh[0][kJdScanThreads - 1];
        if (sh[1][kJdScanThreads - 1] != descs[f].n_segments - 1) jd_fail(status, f, AEJ_JPEGDEC_BAD_RESTART);
    }
    JdSeg *sg = segs + F.seg_base;
    for (long long g = threadIdx.x; g < descs[f].n_segments; g += kJdScanThreads) sg[g].start = g == 0 ? 0 : -1;
}

__global__ __launch_bounds__(kJdThreads) void k_jd_scatter(const JdFile *__restrict__ files, const aej_jpegdec_desc *__restrict__ descs, int n,
                                                           long long n_chunks, const unsigned char *__restrict__ scans,
                                                           const long long *__restrict__ pre, unsigned char *__restrict__ clean,
                                                           JdSeg *__restrict__ segs, int *__restrict__ status)
{
    const long long idx = (long long)blockIdx.x * kJdThreads + threadIdx.x;
    if (idx >= n_chunks) return;
    const long long *q = pre + idx * 3;
    if (q[2] != 0) return;                            // after the end of the scan
    const int f = jd_find_file<&JdFile::chunk_base>(files, n, idx);
    const JdFile &F = files[f];
    const int nseg = descs[f].n_segments;
    const unsigned char *s = scans + F.scan_off;
    unsigned char *dst = clean + F.clean_off;
    long long o = q[0], r = q[1];
    const long long lo = (idx - F.chunk_base) * kJdChunk, hi = min(F.scan_len, lo + kJdChunk);
    for (long long p = lo; p < hi; p++) {
        const int c = jd_byte_class(s, F.scan_len, p);
        if (c == kJdByteEnd) break;
        if (c == kJdByteData) dst[o++] = s[p];
        else if (c == kJdByteRst) {
            if (r >= nseg - 1 || (s[p] & 7) != (r & 7)) jd_fail(status, f, AEJ_JPEGDEC_BAD_RESTART);
            else segs[F.seg_base + r + 1].start = o;
            r++;
        }
    }
}

__global__ __launch_bounds__(kJdThreads) void k_jd_segments(const JdFile *__restrict__ files, const aej_jpegdec_desc *__restrict__ descs, int n,
                                                            long long n_segs, const long long *__restrict__ clean_len, JdSeg *__restrict__ segs,
                                                            int S, int *__restrict__ status)
{
    const long long idx = (long long)blockIdx.x * kJdThreads + threadIdx.x;
    if (idx >= n_segs) return;
    const int f = jd_find_file<&JdFile::seg_base>(files, n, idx);
    const JdFile &F = files[f];
    const aej_jpegdec_desc &d = descs[f];
    const int g = (int)(idx - F.seg_base);
    JdSeg &sg = segs[idx];
    const long long len = min(clean_len[f], F.scan_len);
    long long start = sg.start < 0 ? len : min(sg.start, len);
    long long end = g + 1 < d.n_segments ? segs[idx + 1].start : len;
    end = end < 0 ? len : min(max(end, start), len);
    sg.start = start;
    sg.nbytes = end - start;
    sg.slot_base = g + start * 8 / S;
    long long ns = max(1LL, (sg.nbytes * 8 + S - 1) / S);
    if (sg.slot_base + ns > F.n_slots) {              // cannot happen with the host's bound; never decode outside the slots
        ns = max(0LL, F.n_slots - sg.slot_base);
        jd_fail(status, f, AEJ_JPEGDEC_TRUNCATED);
    }
    sg.n_sub = (int)ns;
    const long long total = (long long)d.mcux * d.mcuy, ri = d.restart_interval ? d.restart_interval : total;
    sg.first_mcu = (int)min((long long)g * ri, total);
    sg.n_mcu = (int)min(ri, total - sg.first_mcu);
}

// ---- Huffman decode --------------------------------------------------------------------------------------------------------------------
struct JdSlotPos {
    int f;
    const JdSeg *seg;
    long long j;                          // subsequence within the segment; -1: idle slot
};

__device__ __forceinline__ JdSlotPos jd_slot(const JdFile *files, const aej_jpegdec_desc *descs, int n, const JdSeg *segs, long long t)
{
    JdSlotPos p;
    p.f = jd_find_file<&JdFile::slot_base>(files, n, t);
    const JdFile &F = files[p.f];
    const long long s = t - F.slot_base;
    const int nseg = descs[p.f].n_segments;
    const JdSeg *sg = segs + F.seg_base;
    const int g = jd_find_seg(sg, nseg, s);
    p.seg = sg + g;
    p.j = s - p.seg->slot_base;
    if (s >= F.n_slots || p.j < 0 || p.j >= p.seg->n_sub) p.j = -1;
    return p;
}

__device__ __forceinline__ unsigned long long jd_guess(const JdSeg &sg, long long j, int S) { return jd_pack(sg.start * 8 + j * S, 0, 0, 0); }

// one sync-mode decode of slot (seg, j) from `entry`; returns the exit state
__device__ __forceinline__ unsigned long long jd_decode_slot(const aej_jpegdec_desc &d, const unsigned char *clean, const JdSeg &sg, long long j, int S,
                                                             unsigned long long entry, int out[4])
{
    JdBits br(clean);
    long long pos = jd_pos(entry);
    int k = jd_k(entry), z = jd_z(entry);
    const long long seg_end = (sg.start + sg.nbytes) * 8;
    const long long stop = j + 1 == sg.n_sub ? seg_end : sg.start * 8 + (j + 1) * S;
    int nstart = 0, dc[3] = { 0, 0, 0 }, pred[3];
    long long next = 0;
    const int rc = jd_run<false>(d, br, pos, k, z, stop, seg_end, nstart, dc, nullptr, next, 0, pred);
    out[0] = nstart; out[1] = dc[0]; out[2] = dc[1]; out[3] = dc[2];
    return jd_pack(pos, k, z, rc != kJdRunStop);
}

__global__ __launch_bounds__(kJdThreads) void k_jd_init(const JdFile *__restrict__ files, const aej_jpegdec_desc *__restrict__ descs, int n,
                                                        long long n_slots, const JdSeg *__restrict__ segs, const unsigned char *__restrict__ clean,
                                                        JdSlots sl, int S, int *__restrict__ last_change)
{
    const long long t = (long long)blockIdx.x * kJdThreads + threadIdx.x;
    if (t >= n_slots) return;
    const JdSlotPos p = jd_slot(files, descs, n, segs, t);
    int out[4] = { 0, 0, 0, 0 };
    unsigned long long entry = jd_pack(0, 0, 0, 1), exit = entry;
    if (p.j >= 0) {
        entry = jd_guess(*p.seg, p.j, S);
        exit = jd_decode_slot(descs[p.f], clean + files[p.f].clean_off, *p.seg, p.j, S, entry, out);
        if (p.j > 0) atomicMax(last_change, 0);
    }
    sl.state[t] = exit;
    sl.used[t] = entry;
    for (int v = 0; v < 4; v++) sl.cnt[t * 4 + v] = out[v];
    sl.first[t] = p.j == 0;
}

__global__ __launch_bounds__(kJdThreads) void k_jd_sync(const JdFile *__restrict__ files, const aej_jpegdec_desc *__restrict__ descs, int n,
                                                        long long n_slots, const JdSeg *__restrict__ segs, const unsigned char *__restrict__ clean,
                                                        JdSlots sl, int S, int round, int *__restrict__ last_change)
{
    if (__hip_atomic_load(last_change, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < round - 1) return;      // converged
    const long long t = (long long)blockIdx.x * kJdThreads + threadIdx.x;
    if (t >= n_slots) return;
    const JdSlotPos p = jd_slot(files, descs, n, segs, t);
    if (p.j <= 0) return;
    const unsigned long long prev = __hip_atomic_load(sl.state + t - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long entry = jd_err(prev) ? jd_guess(*p.seg, p.j, S) : prev;
    if (entry == sl.used[t]) return;
    int out[4];
    const unsigned long long exit = jd_decode_slot(descs[p.f], clean + files[p.f].clean_off, *p.seg, p.j, S, entry, out);
    sl.used[t] = entry;
    bool changed = exit != sl.state[t];
    for (int v = 0; v < 4; v++) changed |= out[v] != sl.cnt[t * 4 + v];
    if (!changed) return;
    for (int v = 0; v < 4; v++) sl.cnt[t * 4 + v] = out[v];
    __hip_atomic_store(sl.state + t, exit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    atomicMax(last_change, round);
}

// segmented exclusive scan over a file's slots (reset where a segment starts): blocks started and the three DC sums
__global__ __launch_bounds__(kJdScanThreads) void k_jd_scan_slots(const JdFile *__restrict__ files, JdSlots sl)
{
    __shared__ long long sh[4][kJdScanThreads];
    __shared__ int shf[kJdScanThreads];
    const JdFile &F = files[blockIdx.x];
    const long long m = F.n_slots, per = (m + kJdScanThreads - 1) / kJdScanThreads;
    const long long lo = min(m, threadIdx.x * per), hi = min(m, lo + per);
    const long long b = F.slot_base;
    long long a[4] = { 0, 0, 0, 0 };
    int fl = 0;
    for (long long i = lo; i < hi; i++) {
        if (sl.first[b + i]) { fl = 1; for (int v = 0; v < 4; v++) a[v] = 0; }
        for (int v = 0; v < 4; v++) a[v] += sl.cnt[(b + i) * 4 + v];
    }
    for (int v = 0; v < 4; v++) sh[v][threadIdx.x] = a[v];
    shf[threadIdx.x] = fl;
    __syncthreads();
    for (int off = 1; off < kJdScanThreads; off <<= 1) {      // (flag, sum) pairs: a later reset discards what came before
        long long t[4];
        int tf = 0;
        if (threadIdx.x >= off) { for (int v = 0; v < 4; v++) t[v] = sh[v][threadIdx.x - off]; tf = shf[threadIdx.x - off]; }
        __syncthreads();
        if (threadIdx.x >= off && !shf[threadIdx.x]) {
            for (int v = 0; v < 4; v++) sh[v][threadIdx.x] += t[v];
            shf[threadIdx.x] = tf;
        }
        __syncthreads();
    }
    long long run[4] = { 0, 0, 0, 0 };
    if (threadIdx.x > 0) for (int v = 0; v < 4; v++) run[v] = sh[v][threadIdx.x - 1];
    for (long long i = lo; i < hi; i++) {
        if (sl.first[b + i]) for (int v = 0; v < 4; v++) run[v] = 0;
        sl.blk_pre[b + i] = run[0];
        for (int v = 0; v < 3; v++) sl.dc_pre[(b + i) * 3 + v] = (int)run[v + 1];
        for (int v = 0; v < 4; v++) run[v] += sl.cnt[(b + i) * 4 + v];
    }
}

__global__ __launch_bounds__(kJdThreads) void k_jd_write(const JdFile *__restrict__ files, const aej_jpegdec_desc *__restrict__ descs, int n,
                                                         long long n_slots, const JdSeg *__restrict__ segs, const unsigned char *__restrict__ clean,
                                                         JdSlots sl, int S, short *__restrict__ coef, int *__restrict__ status)
{
    const long long t = (long long)blockIdx.x * kJdThreads + threadIdx.x;
    if (t >= n_slots) return;
    const JdSlotPos p = jd_slot(files, descs, n, segs, t);
    if (p.j < 0) return;
    const JdSeg &sg = *p.seg;
    const aej_jpegdec_desc &d = descs[p.f];
    const JdFile &F = files[p.f];
    unsigned long long entry = jd_guess(sg, p.j, S);
    if (p.j > 0 && !jd_err(sl.state[t - 1])) entry = sl.state[t - 1];
    JdBits br(clean + F.clean_off);
    long long pos = jd_pos(entry);
    int k = jd_k(entry), z = jd_z(entry);
    const long long seg_end = (sg.start + sg.nbytes) * 8;
    const long long stop = p.j + 1 == sg.n_sub ? seg_end : sg.start * 8 + (p.j + 1) * S;
    const long long seg_blocks = (long long)sg.n_mcu * d.blocks_per_mcu;
    int nstart = 0, dc[3] = { 0, 0, 0 };
    int pred[3] = { sl.dc_pre[t * 3], sl.dc_pre[t * 3 + 1], sl.dc_pre[t * 3 + 2] };
    long long next = sl.blk_pre[t];
    short *c = coef + (F.blk_base + (long long)sg.first_mcu * d.blocks_per_mcu) * 64;
    const int rc = jd_run<true>(d, br, pos, k, z, stop, seg_end, nstart, dc, c, next, seg_blocks, pred);
    const long long cur = z == 0 ? next : next - 1;      // the block being decoded (or the next one) when the loop stopped
    if (rc == kJdRunDone) return;
    if (rc == kJdRunStop) {
        if (p.j + 1 == sg.n_sub && cur < seg_blocks) jd_fail(status, p.f, AEJ_JPEGDEC_TRUNCATED);
        return;
    }
    if (cur >= seg_blocks) return;                    // past the blocks the segment holds (padding)
    jd_fail(status, p.f, rc == kJdRunOutOfBits ? AEJ_JPEGDEC_TRUNCATED : rc == kJdRunBadCode ? AEJ_JPEGDEC_BAD_CODE
                         : rc == kJdRunPast63 ? AEJ_JPEGDEC_RUN_PAST_63 : AEJ_JPEGDEC_BAD_DC);
}

// ---- reconstruction --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kJdThreads) void k_jd_idct(const JdFile *__restrict__ files, const aej_jpegdec_desc *__restrict__ descs, int n,
                                                        long long n_blocks, const short *__restrict__ coef, unsigned char *__restrict__ planes)
{
    const long long idx = (long long)blockIdx.x * kJdThreads + threadIdx.x;
    if (idx >= n_blocks) return;
    const int f = jd_find_file<&JdFile::blk_base>(files, n, idx);
    const JdFile &F = files[f];
    const aej_jpegdec_desc &d = descs[f];
    const long long b = idx - F.blk_base, mcu = b / d.blocks_per_mcu;
    const int k = (int)(b % d.blocks_per_mcu), my = (int)(mcu / d.mcux), mx = (int)(mcu % d.mcux);
    const int c = jd_comp(d, k);
    unsigned char *pl = planes + F.plane_off;
    long long stride, y0, x0;
    if (c == 0) {
        const int by = d.ncomp == 1 ? my : my * d.vs + k / d.hs, bx = d.ncomp == 1 ? mx : mx * d.hs + k % d.hs;
        if (by >= (d.height + 7) / 8 || bx >= (d.width + 7) / 8) return;     // dummy block of an edge MCU
        stride = F.pw0; y0 = by * 8; x0 = bx * 8;
    } else {
        pl += (long long)F.pw0 * F.ph0 + (long long)(c - 1) * F.pw1 * F.ph1;
        stride = F.pw1; y0 = my * 8; x0 = mx * 8;
    }
    jd_idct_block(coef + idx * 64, d.qt[c], pl + y0 * stride + x0, stride);
}

__global__ __launch_bounds__(kJdThreads) void k_jd_rgb(const JdFile *__restrict__ files, const aej_jpegdec_desc *__restrict__ descs, int n,
                                                       long long n_px, const unsigned char *__restrict__ planes, unsigned char *__restrict__ out)
{
    const long long idx = (long long)blockIdx.x * kJdThreads + threadIdx.x;
    if (idx >= n_px) return;
    const int f = jd_find_file<&JdFile::px_base>(files, n, idx);
    const JdFile &F = files[f];
    const aej_jpegdec_desc &d = descs[f];
    const long long r = idx - F.px_base;
    const int y = (int)(r / d.width), x = (int)(r % d.width);
    const unsigned char *pl = planes + F.plane_off;
    unsigned char *o = out + F.out_off + r * 3;
    const int Y = pl[(long long)y * F.pw0 + x];
    if (d.ncomp == 1) { o[0] = o[1] = o[2] = (unsigned char)Y; return; }
    const unsigned char *cb = pl + (long long)F.pw0 * F.ph0, *cr = cb + (long long)F.pw1 * F.ph1;
    const int wc = (d.width + d.hs - 1) / d.hs, hc = (d.height + d.vs - 1) / d.vs;
    jd_rgb(Y, jd_chroma(cb, F.pw1, d.hs, d.vs, wc, hc, y, x), jd_chroma(cr, F.pw1, d.hs, d.vs, wc, hc, y, x), o);
}

// ---- host: the header parser ---------------------------------------------------------------------------------------------------------
// libjpeg's jpeg_make_d_derived_tbl: canonical codes, over-subscription check, then the decode tables
bool jd_build_huff(const JdHuffSrc &s, aej_jpegdec_huff &h)
{
    memset(&h, 0, sizeof h);
    int size[257], code[257], p = 0;
    for (int l = 1; l <= 16; l++)
        for (int i = 0; i < s.bits[l]; i++) size[p++] = l;
    size[p] = 0;
    int c = 0, si = size[0];
    p = 0;
    while (size[p]) {
        while (size[p] == si) code[p++] = c++;
        if (c >= (1 << si)) return false;
        c <<= 1;
        si++;
    }
    p = 0;
    for (int l = 1; l <= 16; l++) {
        if (s.bits[l]) {
            h.valoff[l] = p - code[p];
            p += s.bits[l];
            h.maxcode[l] = code[p - 1];
        } else {
            h.maxcode[l] = -1;
        }
    }
    h.maxcode[17] = -1;
    memcpy(h.vals, s.vals, sizeof h.vals);
    p = 0;
    for (int l = 1; l <= 9; l++)
        for (int i = 0; i < s.bits[l]; i++, p++) {
            const int lo = code[p] << (9 - l);
            for (int e = 0; e < (1 << (9 - l)); e++) h.lut[lo + e] = (uint16_t)((l << 8) | s.vals[p]);
        }
    return true;
}

int jpegdec_parse(const unsigned char *b, unsigned long long n, aej_jpegdec_desc &d, std::string &msg)
{
    memset(&d, 0, sizeof d);
    auto bad = [&](const std::string &m) { msg = m; return -1; };
    auto unsup = [&](const std::string &m) { msg = m; return -5; };
    if (!b || n < 4 || b[0] != 0xFF || b[1] != 0xD8) return bad("not a JPEG file (no SOI marker)");
    uint16_t qt[4][64];
    bool qdef[4] = {}, q16[4] = {}, sof = false, jfif = false, adobe = false;
    int adobe_transform = -1, ri = 0, nf = 0;
    JdHuffSrc hs[2][4];
    unsigned long long p = 2;
    for (;;) {
        if (p >= n) return bad("no SOS marker (the file ends in its header)");
        if (b[p] != 0xFF) return bad("bytes between markers in the header");
        while (p < n && b[p] == 0xFF) p++;
        if (p >= n) return bad("no SOS marker (the file ends in its header)");
        const int m = b[p++];
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
        if (m == 0xD8) return bad("second SOI marker");
        if (m == 0xD9) return bad("EOI before SOS");
        if (p + 2 > n) return bad("truncated marker segment");
        const unsigned L = (unsigned)b[p] << 8 | b[p + 1];
        if (L < 2 || p + L > n) return bad("truncated marker segment");
        const unsigned char *s = b + p + 2;
        const unsigned len = L - 2;
        switch (m) {
        case 0xC0: case 0xC1: {
            if (sof) return bad("two SOF markers");
            if (len < 6) return bad("truncated SOF segment");
            if (s[0] != 8) return unsup("sample precision " + std::to_string(s[0]) + " (only 8-bit)");
            d.height = s[1] << 8 | s[2];
            d.width = s[3] << 8 | s[4];
            nf = s[5];
            if (len != 6u + 3u * nf) return bad("SOF length does not match its component count");
            if (d.height == 0) return unsup("DNL (height defined after the scan)");
            if (d.width == 0) return bad("zero image width");
            if (nf != 1 && nf != 3) return unsup(std::to_string(nf) + " components (only 1 or 3)");
            for (int i = 0; i < nf; i++) {
                d.comp_id[i] = s[6 + 3 * i];
                d.comp_h[i] = s[7 + 3 * i] >> 4;
                d.comp_v[i] = s[7 + 3 * i] & 15;
                d.comp_tq[i] = s[8 + 3 * i];
                if (d.comp_h[i] < 1 || d.comp_h[i] > 4 || d.comp_v[i] < 1 || d.comp_v[i] > 4 || d.comp_tq[i] > 3)
                    return bad("bad component sampling factor or table index");
            }
            d.sof = m;
            sof = true;
            break;
        }
        case 0xC2: return unsup("progressive JPEG (SOF2)");
        case 0xC3: return unsup("lossless JPEG (SOF3)");
        case 0xC5: case 0xC6: case 0xC7: return unsup("hierarchical JPEG (SOF" + std::to_string(m - 0xC0) + ")");
        case 0xC9: case 0xCA: case 0xCB: case 0xCD: case 0xCE: case 0xCF: case 0xCC:
            return unsup("arithmetic coding (" + std::string(m == 0xCC ? "DAC" : "SOF" + std::to_string(m - 0xC0)) + ")");
        case 0xDC: return unsup("DNL marker");
        case 0xC4: {
            unsigned i = 0;
            while (i < len) {
                const int tc = s[i] >> 4, th = s[i] & 15;
                if (tc > 1 || th > 3) return bad("bad DHT table class or index");
                if (i + 17 > len) return bad("truncated DHT segment");
                JdHuffSrc &t = hs[tc][th];
                int cnt = 0;
                for (int l = 1; l <= 16; l++) { t.bits[l] = s[i + l]; cnt += s[i + l]; }
                if (cnt > 256 || i + 17 + cnt > len) return bad("bad DHT symbol count");
                memset(t.vals, 0, sizeof t.vals);
                memcpy(t.vals, s + i + 17, cnt);
                t.count = cnt;
                if (tc == 0)
                    for (int v = 0; v < cnt; v++) if (t.vals[v] > 15) return bad("DC Huffman symbol above 15");
                aej_jpegdec_huff tmp;
                if (!jd_build_huff(t, tmp)) return bad("over-subscribed Huffman table");
                t.defined = true;
                i += 17 + cnt;
            }
            break;
        }
        case 0xDB: {
            unsigned i = 0;
            while (i < len) {
                const int pq = s[i] >> 4, tq = s[i] & 15;
                if (pq > 1 || tq > 3) return bad("bad DQT precision or index");
                const unsigned need = 1 + 64u * (pq + 1);
                if (i + need > len) return bad("truncated DQT segment");
                for (int z = 0; z < 64; z++)
                    qt[tq][jd_natural(z)] = pq ? (uint16_t)(s[i + 1 + 2 * z] << 8 | s[i + 2 + 2 * z]) : s[i + 1 + z];
                qdef[tq] = true;
                q16[tq] = pq == 1;
                i += need;
            }
            break;
        }
        case 0xDD:
            if (len != 2) return bad("bad DRI length");
            ri = s[0] << 8 | s[1];
            break;
        case 0xE0:
            if (len >= 5 && !memcmp(s, "JFIF\0", 5)) jfif = true;
            break;
        case 0xEE:
            if (len >= 12 && !memcmp(s, "Adobe", 5)) { adobe = true; adobe_transform = s[11]; }
            break;
        case 0xDA: {
            if (!sof) return bad("SOS before SOF");
            if (len < 1) return bad("truncated SOS segment");
            const int ns = s[0];
            if (len != 4u + 2u * ns || ns < 1) return bad("SOS length does not match its component count");
            if (ns < nf) return unsup("multi-scan sequential JPEG (the first scan holds " + std::to_string(ns) + " of " + std::to_string(nf) + " components)");
            if (ns != nf) return bad("SOS lists more components than the frame");
            for (int i = 0; i < ns; i++)
                if (s[1 + 2 * i] != d.comp_id[i]) return unsup("scan components in another order than the frame's");
            if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) return bad("bad spectral selection / approximation for a sequential scan");
            if (nf == 3) {
                const bool rgb_ids = d.comp_id[0] == 'R' && d.comp_id[1] == 'G' && d.comp_id[2] == 'B';
                if (!jfif && adobe && adobe_transform == 0) return unsup("Adobe APP14 transform 0 (RGB colour)");
                if (!jfif && !adobe && rgb_ids) return unsup("component ids 'R','G','B' without JFIF (RGB colour)");
                const int h0 = d.comp_h[0], v0 = d.comp_v[0];
                if (d.comp_h[1] != 1 || d.comp_v[1] != 1 || d.comp_h[2] != 1 || d.comp_v[2] != 1 ||
                    !((h0 == 1 && v0 == 1) || (h0 == 2 && v0 == 1) || (h0 == 2 && v0 == 2)))
                    return unsup("sampling factors " + std::to_string(h0) + "x" + std::to_string(v0) + "," + std::to_string(d.comp_h[1]) + "x" +
                                 std::to_string(d.comp_v[1]) + "," + std::to_string(d.comp_h[2]) + "x" + std::to_string(d.comp_v[2]));
                d.hs = h0; d.vs = v0;
                d.mcux = (d.width + 8 * h0 - 1) / (8 * h0);
                d.mcuy = (d.height + 8 * v0 - 1) / (8 * v0);
                d.blocks_per_mcu = h0 * v0 + 2;
            } else {                                     // one component: a non-interleaved scan, whatever its sampling factors say
                d.hs = d.vs = 1;
                d.mcux = (d.width + 7) / 8;
                d.mcuy = (d.height + 7) / 8;
                d.blocks_per_mcu = 1;
            }
            for (int i = 0; i < nf; i++) {
                const int tq = d.comp_tq[i], td = s[2 + 2 * i] >> 4, ta = s[2 + 2 * i] & 15;
                if (!qdef[tq]) return bad("undefined quantisation table " + std::to_string(tq));
                if (td > 3 || ta > 3 || !hs[0][td].defined || !hs[1][ta].defined) return bad("undefined Huffman table");
                memcpy(d.qt[i], qt[tq], sizeof d.qt[i]);
                d.precision16 |= q16[tq];
                jd_build_huff(hs[0][td], d.dc[i]);
                jd_build_huff(hs[1][ta], d.ac[i]);
            }
            const long long mcus = (long long)d.mcux * d.mcuy;
            d.restart_interval = ri;
            d.n_segments = ri ? (int)((mcus + ri - 1) / ri) : 1;
            d.ncomp = nf;
            d.scan_offset = (long long)(p + L);
            d.scan_length = (long long)(n - (p + L));
            return 0;
        }
        default:
            break;                                   // APPn, COM, JPGn, ...
        }
        p += L;
    }
}

// ---- host: layout and launch sequence ----------------------------------------------------------------------------------------------------
static long long jd_align(long long v, long long a) { return (v + a - 1) / a * a; }

long long jpegdec_layout(const aej_jpegdec_desc *descs, int n, int S, std::vector<JdFile> &files, JdBufSizes &z)
{
    files.assign(n, JdFile{});
    z = JdBufSizes{};
    for (int i = 0; i < n; i++) {
        const aej_jpegdec_desc &d = descs[i];
        JdFile &F = files[i];
        F.scan_len = d.scan_length;
        F.clean_off = z.clean;
        z.clean += jd_align(d.scan_length, 4) + 16;
        F.chunk_base = z.chunks;
        F.n_chunks = (d.scan_length + kJdChunk - 1) / kJdChunk;
        z.chunks += F.n_chunks;
        F.seg_base = z.segs;
        z.segs += d.n_segments;
        F.slot_base = z.slots;
        F.n_slots = d.n_segments + (d.scan_length * 8 + S - 1) / S + 1;
        z.slots += F.n_slots;
        F.blk_base = z.blocks;
        F.n_blocks = (long long)d.mcux * d.mcuy * d.blocks_per_mcu;
        z.blocks += F.n_blocks;
        F.pw0 = d.mcux * 8 * d.hs; F.ph0 = d.mcuy * 8 * d.vs;
        F.pw1 = d.ncomp == 3 ? d.mcux * 8 : 0; F.ph1 = d.ncomp == 3 ? d.mcuy * 8 : 0;
        F.plane_off = z.planes;
        z.planes += jd_align((long long)F.pw0 * F.ph0 + 2LL * F.pw1 * F.ph1, 256);
        F.px_base = z.px;
        z.px += (long long)d.width * d.height;
    }
    return 0;
}

unsigned long long jpegdec_carve(void *base, int n, const JdBufSizes &z, JdBufs &w)
{
    unsigned long long off = 0;
    auto take = [&](unsigned long long bytes) { void *p = base ? (char *)base + off : nullptr; off += (bytes + 255) / 256 * 256; return p; };
    w.files = (JdFile *)take(sizeof(JdFile) * n + sizeof(aej_jpegdec_desc) * n + 16);
    w.descs = base ? (aej_jpegdec_desc *)((char *)w.files + sizeof(JdFile) * n) : nullptr;
    w.last_change = base ? (int *)((char *)w.descs + sizeof(aej_jpegdec_desc) * n) : nullptr;
    w.cnt = (int *)take(z.chunks * 3 * 4);
    w.pre = (long long *)take(z.chunks * 3 * 8);
    w.clean_len = (long long *)take(n * 8);
    w.segs = (JdSeg *)take(z.segs * sizeof(JdSeg));
    w.clean = (unsigned char *)take(z.clean);
    w.sl.state = (unsigned long long *)take(z.slots * 8);
    w.sl.used = (unsigned long long *)take(z.slots * 8);
    w.sl.cnt = (int *)take(z.slots * 16);
    w.sl.first = (unsigned char *)take(z.slots);
    w.sl.blk_pre = (long long *)take(z.slots * 8);
    w.sl.dc_pre = (int *)take(z.slots * 12);
    w.coef = (short *)take(z.blocks * 128);
    w.planes = (unsigned char *)take(z.planes);
    return off;
}

static unsigned jd_grid(long long n) { return (unsigned)((n + kJdThreads - 1) / kJdThreads); }

// everything up to the first read-back: upload, un-stuffing, segments, first guesses
hipError_t launch_jpegdec_begin(hipStream_t st, int n, const JdBufSizes &z, const JdBufs &w, const void *blob_host, unsigned long long blob_bytes,
                                const unsigned char *scans, int S, int *status)
{
    hipError_t e = hipMemcpyAsync(w.files, blob_host, blob_bytes, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return e;
    if ((e = launch_jpegdec_unstuff(st, n, z, w, scans, S, status)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_jd_init, dim3(jd_grid(z.slots)), dim3(kJdThreads), 0, st, w.files, w.descs, n, z.slots, w.segs, w.clean, w.sl, S,
                       w.last_change);
    return hipGetLastError();
}

// un-stuffing and restart segments of n streams (files here; the scans of progressive files in jpegprog.hip); zeroes status first
hipError_t launch_jpegdec_unstuff(hipStream_t st, int n, const JdBufSizes &z, const JdBufs &w, const unsigned char *scans, int S, int *status)
{
    hipError_t e = hipMemsetAsync(status, 0, sizeof(int) * n, st);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(w.clean_len, 0, 8 * n, st)) != hipSuccess) return e;
    if (z.chunks > 0) hipLaunchKernelGGL(k_jd_count, dim3(jd_grid(z.chunks)), dim3(kJdThreads), 0, st, w.files, n, z.chunks, scans, w.cnt);
    hipLaunchKernelGGL(k_jd_scan_chunks, dim3(n), dim3(kJdScanThreads), 0, st, w.files, w.descs, w.cnt, w.pre, w.clean_len, w.segs, status);
    if (z.chunks > 0)
        hipLaunchKernelGGL(k_jd_scatter, dim3(jd_grid(z.chunks)), dim3(kJdThreads), 0, st, w.files, w.descs, n, z.chunks, scans, w.pre, w.clean,
                           w.segs, status);
    hipLaunchKernelGGL(k_jd_segments, dim3(jd_grid(z.segs)), dim3(kJdThreads), 0, st, w.files, w.descs, n, z.segs, w.clean_len, w.segs, S, status);
    return hipGetLastError();
}

hipError_t launch_jpegdec_sync(hipStream_t st, int n, const JdBufSizes &z, const JdBufs &w, int S, int first_round, int rounds)
{
    for (int r = first_round; r < first_round + rounds; r++)
        hipLaunchKernelGGL(k_jd_sync, dim3(jd_grid(z.slots)), dim3(kJdThreads), 0, st, w.files, w.descs, n, z.slots, w.segs, w.clean, w.sl, S, r,
                           w.last_change);
    return hipGetLastError();
}

// after the last sync round: the coefficients of every file (natural order, MCU order, dummy blocks included) and the decode's status words
hipError_t launch_jpegdec_write(hipStream_t st, int n, const JdBufSizes &z, const JdBufs &w, int S, int *status)
{
    hipError_t e = hipMemsetAsync(w.coef, 0, (size_t)z.blocks * 128, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_jd_scan_slots, dim3(n), dim3(kJdScanThreads), 0, st, w.files, w.sl);
    hipLaunchKernelGGL(k_jd_write, dim3(jd_grid(z.slots)), dim3(kJdThreads), 0, st, w.files, w.descs, n, z.slots, w.segs, w.clean, w.sl, S, w.coef,
                       status);
    return hipGetLastError();
}

hipError_t launch_jpegdec_finish(hipStream_t st, int n, const JdBufSizes &z, const JdBufs &w, int S, unsigned char *out, int *status)
{
    const hipError_t e = launch_jpegdec_write(st, n, z, w, S, status);
    if (e != hipSuccess) return e;
    return launch_jpegdec_recon(st, n, z, w, out);
}

// coefficients (natural order, MCU order) -> RGB, for n files
hipError_t launch_jpegdec_recon(hipStream_t st, int n, const JdBufSizes &z, const JdBufs &w, unsigned char *out)
{
    hipLaunchKernelGGL(k_jd_idct, dim3(jd_grid(z.blocks)), dim3(kJdThreads), 0, st, w.files, w.descs, n, z.blocks, w.coef, w.planes);
    hipLaunchKernelGGL(k_jd_rgb, dim3(jd_grid(z.px)), dim3(kJdThreads), 0, st, w.files, w.descs, n, z.px, w.planes, out);
    return hipGetLastError();
}

}  // namespace aej
