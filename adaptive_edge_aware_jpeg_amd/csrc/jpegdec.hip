// jpegdec.hip -- baseline JPEG files decoded on the device, pixel-identical to Pillow with libjpeg-turbo (aej_jpegdec_*, include/aej.h).
// The host reads the markers up to SOS (aej_jpegdec_parse_host, jpegparse.hip); everything after that runs here, one launch per stage over
// the whole call:
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
//   k_jd_rgb        one thread per pixel: up-sampling (jd_chroma: the one rule of jpegdec_core.h, jd_up_chroma, at full size) and
//                   YCbCr -> RGB
//   k_jd_scaled     files decoded at scale 2, 4 or 8 (Pillow's draft()) in the place of the two above: one workgroup per run of kJdRun
//                   MCUs of one MCU row -- reduced IDCTs into LDS, colour into LDS, then the run's output rows stored as whole dwords.
//                   No sample planes: 4:2:0 chroma comes out of a twice-as-large IDCT at luma resolution, and the one neighbour sample
//                   jd_up_chroma reads for a 4:2:2 file on either side comes from the chroma blocks of the two adjacent MCUs
//   k_jd_scaled_h1v2 the same for 4:4:0 files (luma 1 x 2), whose chroma IDCT stays at the luma block's size at every scale and is
//                   up-sampled vertically: the neighbour rows the h1v2 filter needs come from the chroma blocks of the MCU rows above
//                   and below the run (a vertical halo).  A kernel of its own, so that k_jd_scaled compiles as it did without it
//   k_jd_luma       files that leave as their luma plane alone, [oh][ow] (libjpeg's out_color_space = JCS_GRAYSCALE; a one-component
//                   file's samples), at scale 1, 2, 4 or 8, in the place of all of the above: k_jd_scaled's plan, luma blocks only
//   k_jd_sbox       files of which a box is decoded, in the place of every reconstruction kernel above: of the full-size image (box= of the
//                   Python call, the _box entries; <0>) or of the image at scale 2, 4 or 8 (scaled_box=, the _sbox entries; <1..3>).  One
//                   workgroup per tile of the box -- IDCTs, at m = 8 >> shift samples per block side, of the tile's luma blocks and of its
//                   chroma blocks plus a ring of neighbour blocks into LDS, then jd_up_chroma / jd_rgb on the LDS planes, and only the
//                   box's pixels stored.  No sample planes.  In a call with such a file k_jd_init / k_jd_sync / k_jd_write run as their
//                   <true> instantiation: a restart segment of a boxed file that holds no MCU of the window's MCU rows is an idle slot
//                   to them, and only those rows' coefficients are stored (both work in MCUs, whatever the scale)
//   k_jd_init4 / k_jd_sync4 / k_jd_scan_slots4 / k_jd_write4   the slot kernels of a call that has a four-component (CMYK, YCCK) or RGB-coded
//                   file (aej_jpegdec_batch_adobe), or a YCbCr file whose three components share one table pair (jd_four), for all of its files: a fourth DC sum and prefix per slot, a 4-bit block slot in the packed
//                   state, component 3 under the tables of the file's aej_jpeg_adobe; k_jd_fix4 between two k_jd_scan_slots4 for the files
//                   whose components share one table pair (JdFile::uniform), where the block slot comes from the block counts
//   k_jd_idct4      k_jd_idct for those files: four sample planes
//   k_jd_adobe      those files in the place of k_jd_rgb: four pixels per thread -- every sub-sampled plane, K included, up-sampled by
//                   jd_chroma's rules, the colour model's rule (jd_adobe_pixel), whole-dword stores of 3 or 4 channels
// Bounds: every index derives from the host-computed JdFile layout; a file's reads stay inside its scan and its clean stream, decode loops
// are bounded by their subsequence's bits, and coefficient writes by the segment's block count.
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "aej_ctx.h"

namespace aej {

constexpr int kJdThreads = 256;
constexpr int kJdScanThreads = 1024;
constexpr int kJdRun = 64;                 // MCUs of one MCU row that a workgroup of k_jd_scaled reconstructs

// index i of the last of n files whose member M is <= t (find_last, aej_launch.h)
template <long long JdFile::*M>
__device__ __forceinline__ int jd_find_file(const JdFile *f, int n, long long t)
{
    return find_last(f, n, t, [](const JdFile &F) { return F.*M; });
}

// the file whose workgroups contain `blockIdx.x`, in the grid of the kernel whose first workgroup of a file is M[k] (an array member)
template <class A>
__device__ __forceinline__ int jd_group_file(const JdFile *f, int n, A JdFile::*M, int k)
{
    return find_last(f, n, (long long)blockIdx.x, [=](const JdFile &F) { return (F.*M)[k]; });
}

// Rows 0 .. nrows - 1 of nbytes bytes each leave LDS for global memory, row r to gp0 + r * pitch: whole dwords inside a row, single
// bytes at its unaligned ends, so only the row's own bytes are written.  kPlaced: the row sits in LDS as it does in its dwords -- at
// lds + r * stride + (its address & 3), lds and stride dword-aligned -- and a dword is one LDS read; else the row starts at
// lds + r * stride, wherever that is, and a dword is put together from four bytes.
template <bool kPlaced>
__device__ __forceinline__ void jd_store_rows(unsigned char *gp0, int pitch, const unsigned char *lds, int stride, int nrows, int nbytes)
{
    const int nslots = (nbytes + 6) / 4;              // dwords a row can touch: up to 3 bytes of shift
    for (int p = threadIdx.x; p < nrows * nslots; p += kJdThreads) {
        const int r = p / nslots, k = p % nslots;
        unsigned char *gp = gp0 + (long long)r * pitch;
        const int a = (int)((uintptr_t)gp & 3), b0 = max(4 * k, a), b1 = min(4 * k + 4, a + nbytes);
        const unsigned char *s = lds + r * stride - (kPlaced ? 0 : a);      // s[b]: the byte at place b of the row's dwords (read for a <= b < a + nbytes only)
        if (b1 - b0 != 4) { for (int b = b0; b < b1; b++) gp[b - a] = s[b]; continue; }      // the ends of a row: its own bytes only
        unsigned *g = reinterpret_cast<unsigned *>(gp + (4 * k - a));
        if (kPlaced) *g = *reinterpret_cast<const unsigned *>(s + 4 * k);
        else *g = (unsigned)s[4 * k] | ((unsigned)s[4 * k + 1] << 8) | ((unsigned)s[4 * k + 2] << 16) | ((unsigned)s[4 * k + 3] << 24);
    }
}

__device__ __forceinline__ int jd_find_seg(const JdSeg *s, int n, long long t)      // last segment whose slot_base <= t
{
    return find_last(s, n, t, [](const JdSeg &S) { return S.slot_base; });
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

// kBox: the slots of a boxed file's segment [first_mcu, first_mcu + n_mcu) that does not meet the window's MCU rows are idle
template <bool kBox>
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
    if (kBox && (F.shift & kJdBox)) {
        const long long mcux = descs[p.f].mcux, first = p.seg->first_mcu;
        if (first >= F.win[3] * mcux || first + p.seg->n_mcu <= F.win[1] * mcux) p.j = -1;
    }
    return p;
}

template <bool kFour = false>
__device__ __forceinline__ unsigned long long jd_guess(const JdSeg &sg, long long j, int S) { return jd_pack<kFour>(sg.start * 8 + j * S, 0, 0, 0); }

// one sync-mode decode of slot (seg, j) from `entry`; returns the exit state.  out: blocks started and the DC sums (kFour: of four
// components; x: the file's aej_jpeg_adobe)
template <bool kFour = false>
__device__ __forceinline__ unsigned long long jd_decode_slot(const aej_jpegdec_desc &d, const unsigned char *clean, const JdSeg &sg, long long j, int S,
                                                             unsigned long long entry, int *out, const aej_jpeg_adobe *x = nullptr, int k_given = -1)
{
    constexpr int kNc = kFour ? 4 : 3;
    JdBits br(clean);
    long long pos = jd_pos<kFour>(entry);
    int k = kFour && k_given >= 0 ? k_given : jd_k<kFour>(entry), z = jd_z(entry);
    const long long seg_end = (sg.start + sg.nbytes) * 8;
    const long long stop = j + 1 == sg.n_sub ? seg_end : sg.start * 8 + (j + 1) * S;
    int nstart = 0, dc[kNc] = {}, pred[kNc];
    long long next = 0;
    const int rc = jd_run<false, false, kFour>(d, br, pos, k, z, stop, seg_end, nstart, dc, nullptr, next, 0, pred, 0, x);
    out[0] = nstart;
    for (int v = 0; v < kNc; v++) out[v + 1] = dc[v];
    return jd_pack<kFour>(pos, k, z, rc != kJdRunStop);
}

// The three slot kernels as functions of <kBox, kFour>: k_jd_init / k_jd_sync / k_jd_write <kBox> are their <kBox, false> forms; the
// <true, true> forms are k_jd_init4 / k_jd_sync4 / k_jd_write4, which a call with a four-component or RGB-coded file runs for all of
// its files (kFour: jd_pack's 4-bit block slot, a fourth DC sum per slot, component 3 under the tables of adobe[file]).
template <bool kBox, bool kFour>
__device__ __forceinline__ void jd_init_slot(const JdFile *__restrict__ files, const aej_jpegdec_desc *__restrict__ descs, int n,
                                             long long n_slots, const JdSeg *__restrict__ segs, const unsigned char *__restrict__ clean,
                                             JdSlots sl, int S, int *__restrict__ last_change, const aej_jpeg_adobe *__restrict__ adobe)
{
    constexpr int kNv = kFour ? 5 : 4;
    const long long t = (long long)blockIdx.x * kJdThreads + threadIdx.x;
    if (t >= n_slots) return;
    const JdSlotPos p = jd_slot<kBox>(files, descs, n, segs, t);
    int out[kNv] = {};
    unsigned long long entry = jd_pack<kFour>(0, 0, 0, 1), exit = entry;
    if (p.j >= 0) {
        entry = jd_guess<kFour>(*p.seg, p.j, S);
        exit = jd_decode_slot<kFour>(descs[p.f], clean + files[p.f].clean_off, *p.seg, p.j, S, entry, out, kFour ? adobe + p.f : nullptr);
        if (p.j > 0) atomicMax(last_change, 0);
    }
    sl.state[t] = exit;
    sl.used[t] = entry;
    for (int v = 0; v < kNv; v++) sl.cnt[t * kNv + v] = out[v];
    sl.first[t] = p.j == 0;
}

template <bool kBox>
__global__ __launch_bounds__(kJdThreads) void k_jd_init(const JdFile *__restrict__ files, const aej_jpegdec_desc *__restrict__ descs, int n,
                                                        long long n_slots, const JdSeg *__restrict__ segs, const unsigned char *__restrict__ clean,
                                                        JdSlots sl, int S, int *__restrict__ last_change)
{
    jd_init_slot<kBox, false>(files, descs, n, n_slots, segs, clean, sl, S, last_change, nullptr);
}

__global__ __launch_bounds__(kJdThreads) void k_jd_init4(const JdFile *__restrict__ files, const aej_jpegdec_desc *__restrict__ descs, int n,
                                                         long long n_slots, const JdSeg *__restrict__ segs, const unsigned char *__restrict__ clean,
                                                         JdSlots sl, int S, int *__restrict__ last_change, const aej_jpeg_adobe *__restrict__ adobe)
{
    jd_init_slot<true, true>(files, descs, n, n_slots, segs, clean, sl, S, last_change, adobe);
}

template <bool kBox, bool kFour>
__device__ __forceinline__ void jd_sync_slot(const JdFile *__restrict__ files, const aej_jpegdec_desc *__restrict__ descs, int n,
                                             long long n_slots, const JdSeg *__restrict__ segs, const unsigned char *__restrict__ clean,
                                             JdSlots sl, int S, int round, int *__restrict__ last_change, const aej_jpeg_adobe *__restrict__ adobe)
{
    constexpr int kNv = kFour ? 5 : 4;
    if (__hip_atomic_load(last_change, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < round - 1) return;      // converged
    const long long t = (long long)blockIdx.x * kJdThreads + threadIdx.x;
    if (t >= n_slots) return;
    const JdSlotPos p = jd_slot<kBox>(files, descs, n, segs, t);
    if (p.j <= 0) return;
    const unsigned long long prev = __hip_atomic_load(sl.state + t - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned long long entry = jd_err<kFour>(prev) ? jd_guess<kFour>(*p.seg, p.j, S) : prev;
    if (kFour && files[p.f].uniform) entry &= ~(15ULL << 6);      // one table for all components: the decode does not depend on the block slot, and
                                                                 // nothing in the bits would ever correct a wrong one -- slot 0 here, k_jd_fix4 later
    if (entry == sl.used[t]) return;
    int out[kNv];
    const unsigned long long exit = jd_decode_slot<kFour>(descs[p.f], clean + files[p.f].clean_off, *p.seg, p.j, S, entry, out, kFour ? adobe + p.f : nullptr);
    sl.used[t] = entry;
    bool changed = exit != sl.state[t];
    for (int v = 0; v < kNv; v++) changed |= out[v] != sl.cnt[t * kNv + v];
    if (!changed) return;
    for (int v = 0; v < kNv; v++) sl.cnt[t * kNv + v] = out[v];
    __hip_atomic_store(sl.state + t, exit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    atomicMax(last_change, round);
}

template <bool kBox>
__global__ __launch_bounds__(kJdThreads) void k_jd_sync(const JdFile *__restrict__ files, const aej_jpegdec_desc *__restrict__ descs, int n,
                                                        long long n_slots, const JdSeg *__restrict__ segs, const unsigned char *__restrict__ clean,
                                                        JdSlots sl, int S, int round, int *__restrict__ last_change)
{
    jd_sync_slot<kBox, false>(files, descs, n, n_slots, segs, clean, sl, S, round, last_change, nullptr);
}

__global__ __launch_bounds__(kJdThreads) void k_jd_sync4(const JdFile *__restrict__ files, const aej_jpegdec_desc *__restrict__ descs, int n,
                                                         long long n_slots, const JdSeg *__restrict__ segs, const unsigned char *__restrict__ clean,
                                                         JdSlots sl, int S, int round, int *__restrict__ last_change,
                                                         const aej_jpeg_adobe *__restrict__ adobe)
{
    jd_sync_slot<true, true>(files, descs, n, n_slots, segs, clean, sl, S, round, last_change, adobe);
}

// segmented exclusive scan over a file's slots (reset where a segment starts): blocks started and the three DC sums (kFour: four)
template <bool kFour>
__device__ __forceinline__ void jd_scan_slots(const JdFile *__restrict__ files, JdSlots sl, long long (*sh)[kJdScanThreads], int *shf)
{
    constexpr int kNv = kFour ? 5 : 4;
    const JdFile &F = files[blockIdx.x];
    const long long m = F.n_slots, per = (m + kJdScanThreads - 1) / kJdScanThreads;
    const long long lo = min(m, threadIdx.x * per), hi = min(m, lo + per);
    const long long b = F.slot_base;
    long long a[kNv] = {};
    int fl = 0;
    for (long long i = lo; i < hi; i++) {
        if (sl.first[b + i]) { fl = 1; for (int v = 0; v < kNv; v++) a[v] = 0; }
        for (int v = 0; v < kNv; v++) a[v] += sl.cnt[(b + i) * kNv + v];
    }
    for (int v = 0; v < kNv; v++) sh[v][threadIdx.x] = a[v];
    shf[threadIdx.x] = fl;
    __syncthreads();
    for (int off = 1; off < kJdScanThreads; off <<= 1) {      // (flag, sum) pairs: a later reset discards what came before
        long long t[kNv];
        int tf = 0;
        if (threadIdx.x >= off) { for (int v = 0; v < kNv; v++) t[v] = sh[v][threadIdx.x - off]; tf = shf[threadIdx.x - off]; }
        __syncthreads();
        if (threadIdx.x >= off && !shf[threadIdx.x]) {
            for (int v = 0; v < kNv; v++) sh[v][threadIdx.x] += t[v];
            shf[threadIdx.x] = tf;
        }
        __syncthreads();
    }
    long long run[kNv] = {};
    if (threadIdx.x > 0) for (int v = 0; v < kNv; v++) run[v] = sh[v][threadIdx.x - 1];
    for (long long i = lo; i < hi; i++) {
        if (sl.first[b + i]) for (int v = 0; v < kNv; v++) run[v] = 0;
        sl.blk_pre[b + i] = run[0];
        for (int v = 0; v < kNv - 1; v++) sl.dc_pre[(b + i) * (kNv - 1) + v] = (int)run[v + 1];
        for (int v = 0; v < kNv; v++) run[v] += sl.cnt[(b + i) * kNv + v];
    }
}

// the block slot of a uniform file's slot t at its entry, from the blocks started before it in the segment (which begins an MCU): the
// block in progress when z != 0, else the next one
__device__ __forceinline__ int jd_slot_k(long long blk_pre, int z, int bpm)
{
    const long long cur = z == 0 ? blk_pre : blk_pre - 1;
    return (int)((cur > 0 ? cur : 0) % bpm);
}

// After the first k_jd_scan_slots4 of a kFour call, for the slots of uniform files alone: the decode once more, now from the right block
// slot, so that every DC difference is summed under its own component; a second k_jd_scan_slots4 then gives the DC prefixes.  (The
// blocks started, the exit position and the zigzag index do not depend on the slot and stay as the sync rounds left them.)
__global__ __launch_bounds__(kJdThreads) void k_jd_fix4(const JdFile *__restrict__ files, const aej_jpegdec_desc *__restrict__ descs, int n,
                                                        long long n_slots, const JdSeg *__restrict__ segs, const unsigned char *__restrict__ clean,
                                                        JdSlots sl, int S, const aej_jpeg_adobe *__restrict__ adobe)
{
    const long long t = (long long)blockIdx.x * kJdThreads + threadIdx.x;
    if (t >= n_slots) return;
    const JdSlotPos p = jd_slot<true>(files, descs, n, segs, t);
    if (p.j < 0 || !files[p.f].uniform) return;
    unsigned long long entry = jd_guess<true>(*p.seg, p.j, S);
    if (p.j > 0 && !jd_err<true>(sl.state[t - 1])) entry = sl.state[t - 1];
    int out[5];
    jd_decode_slot<true>(descs[p.f], clean + files[p.f].clean_off, *p.seg, p.j, S, entry, out, adobe + p.f,
                         jd_slot_k(sl.blk_pre[t], jd_z(entry), descs[p.f].blocks_per_mcu));
    for (int v = 1; v < 5; v++) sl.cnt[t * 5 + v] = out[v];
}

__global__ __launch_bounds__(kJdScanThreads) void k_jd_scan_slots(const JdFile *__restrict__ files, JdSlots sl)
{
    __shared__ long long sh[4][kJdScanThreads];
    __shared__ int shf[kJdScanThreads];
    jd_scan_slots<false>(files, sl, sh, shf);
}

__global__ __launch_bounds__(kJdScanThreads) void k_jd_scan_slots4(const JdFile *__restrict__ files, JdSlots sl)
{
    __shared__ long long sh[5][kJdScanThreads];
    __shared__ int shf[kJdScanThreads];
    jd_scan_slots<true>(files, sl, sh, shf);
}

template <bool kBox, bool kFour>
__device__ __forceinline__ void jd_write_slot(const JdFile *__restrict__ files, const aej_jpegdec_desc *__restrict__ descs, int n,
                                              long long n_slots, const JdSeg *__restrict__ segs, const unsigned char *__restrict__ clean,
                                              JdSlots sl, int S, short *__restrict__ coef, int *__restrict__ status,
                                              const aej_jpeg_adobe *__restrict__ adobe)
{
    constexpr int kNc = kFour ? 4 : 3;
    const long long t = (long long)blockIdx.x * kJdThreads + threadIdx.x;
    if (t >= n_slots) return;
    const JdSlotPos p = jd_slot<kBox>(files, descs, n, segs, t);
    if (p.j < 0) return;
    const JdSeg &sg = *p.seg;
    const aej_jpegdec_desc &d = descs[p.f];
    const JdFile &F = files[p.f];
    const aej_jpeg_adobe *x = kFour ? adobe + p.f : nullptr;
    unsigned long long entry = jd_guess<kFour>(sg, p.j, S);
    if (p.j > 0 && !jd_err<kFour>(sl.state[t - 1])) entry = sl.state[t - 1];
    JdBits br(clean + F.clean_off);
    long long pos = jd_pos<kFour>(entry);
    int k = jd_k<kFour>(entry), z = jd_z(entry);
    const long long seg_end = (sg.start + sg.nbytes) * 8;
    const long long stop = p.j + 1 == sg.n_sub ? seg_end : sg.start * 8 + (p.j + 1) * S;
    const long long seg_blocks = (long long)sg.n_mcu * d.blocks_per_mcu;
    int nstart = 0, dc[kNc] = {};
    int pred[kNc];
    for (int v = 0; v < kNc; v++) pred[v] = sl.dc_pre[t * kNc + v];
    long long next = sl.blk_pre[t];
    if (kFour && F.uniform) k = jd_slot_k(next, z, d.blocks_per_mcu);
    short *c = coef + (F.blk_base + (long long)sg.first_mcu * d.blocks_per_mcu) * 64;
    int rc;
    if (kBox && (F.shift & kJdBox)) {                 // blocks [lo, hi) of the segment lie in the stored MCU rows [win[1], win[3]); c: its block 0, were it stored
        const long long first = (long long)sg.first_mcu * d.blocks_per_mcu, row = (long long)d.mcux * d.blocks_per_mcu;
        const long long lo = max(0LL, F.win[1] * row - first), hi = min(seg_blocks, F.win[3] * row - first);
        c = coef + (F.blk_base + first - F.row0 * row) * 64;
        rc = jd_run<true, true, kFour>(d, br, pos, k, z, stop, seg_end, nstart, dc, c, next, hi, pred, lo, x);
        const long long cur = z == 0 ? next : next - 1;
        if (rc == kJdRunDone || cur >= hi) return;   // nothing the window needs is left in this slot
        if (rc == kJdRunStop) {
            if (p.j + 1 == sg.n_sub) jd_fail(status, p.f, AEJ_JPEGDEC_TRUNCATED);
            return;
        }
        jd_fail(status, p.f, rc == kJdRunOutOfBits ? AEJ_JPEGDEC_TRUNCATED : rc == kJdRunBadCode ? AEJ_JPEGDEC_BAD_CODE
                             : rc == kJdRunPast63 ? AEJ_JPEGDEC_RUN_PAST_63 : AEJ_JPEGDEC_BAD_DC);
        return;
    }
    rc = jd_run<true, false, kFour>(d, br, pos, k, z, stop, seg_end, nstart, dc, c, next, seg_blocks, pred, 0, x);
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

template <bool kBox>
__global__ __launch_bounds__(kJdThreads) void k_jd_write(const JdFile *__restrict__ files, const aej_jpegdec_desc *__restrict__ descs, int n,
                                                         long long n_slots, const JdSeg *__restrict__ segs, const unsigned char *__restrict__ clean,
                                                         JdSlots sl, int S, short *__restrict__ coef, int *__restrict__ status)
{
    jd_write_slot<kBox, false>(files, descs, n, n_slots, segs, clean, sl, S, coef, status, nullptr);
}

__global__ __launch_bounds__(kJdThreads) void k_jd_write4(const JdFile *__restrict__ files, const aej_jpegdec_desc *__restrict__ descs, int n,
                                                          long long n_slots, const JdSeg *__restrict__ segs, const unsigned char *__restrict__ clean,
                                                          JdSlots sl, int S, short *__restrict__ coef, int *__restrict__ status,
                                                          const aej_jpeg_adobe *__restrict__ adobe)
{
    jd_write_slot<true, true>(files, descs, n, n_slots, segs, clean, sl, S, coef, status, adobe);
}

// ---- reconstruction --------------------------------------------------------------------------------------------------------------------
// kAdobe: k_jd_idct4, for the files with kJdAdobe in their shift alone (which k_jd_idct leaves alone, as it does every file with a shift):
// component 3's blocks follow the MCU's others and go to a fourth plane behind the three, pw3 x ph3, under adobe[file]'s table
template <bool kAdobe>
__device__ __forceinline__ void jd_idct_thread(const JdFile *__restrict__ files, const aej_jpegdec_desc *__restrict__ descs, int n,
                                               long long n_blocks, const short *__restrict__ coef, unsigned char *__restrict__ planes,
                                               const aej_jpeg_adobe *__restrict__ adobe)
{
    const long long idx = (long long)blockIdx.x * kJdThreads + threadIdx.x;
    if (idx >= n_blocks) return;
    const int f = jd_find_file<&JdFile::blk_base>(files, n, idx);
    const JdFile &F = files[f];
    if (kAdobe ? !(F.shift & kJdAdobe) : F.shift != 0) return;      // a scaled file: k_jd_scaled reads its coefficients
    const aej_jpegdec_desc &d = descs[f];
    const long long b = idx - F.blk_base, mcu = b / d.blocks_per_mcu;
    const int k = (int)(b % d.blocks_per_mcu), my = (int)(mcu / d.mcux), mx = (int)(mcu % d.mcux);
    const int c = kAdobe ? jd_comp4(d, k) : jd_comp(d, k);
    unsigned char *pl = planes + F.plane_off;
    long long stride, y0, x0;
    const uint16_t *qt = kAdobe ? d.qt[c < 3 ? c : 0] : d.qt[c];
    if (c == 0) {
        const int by = d.ncomp == 1 ? my : my * d.vs + k / d.hs, bx = d.ncomp == 1 ? mx : mx * d.hs + k % d.hs;
        if (by >= (d.height + 7) / 8 || bx >= (d.width + 7) / 8) return;     // dummy block of an edge MCU
        stride = F.pw0; y0 = by * 8; x0 = bx * 8;
    } else if (kAdobe && c == 3) {
        const aej_jpeg_adobe &x = adobe[f];
        const int kk = k - d.hs * d.vs - 2;
        const bool full = x.h3 == d.hs && x.v3 == d.vs;                   // sampled as component 0: its block grid, its dummy blocks
        const int by = full ? my * d.vs + kk / d.hs : my, bx = full ? mx * d.hs + kk % d.hs : mx;
        if (full && (by >= (d.height + 7) / 8 || bx >= (d.width + 7) / 8)) return;
        pl += (long long)F.pw0 * F.ph0 + 2LL * F.pw1 * F.ph1;
        stride = F.pw3; y0 = by * 8; x0 = bx * 8;
        qt = x.qt3;
    } else {
        pl += (long long)F.pw0 * F.ph0 + (long long)(c - 1) * F.pw1 * F.ph1;
        stride = F.pw1; y0 = my * 8; x0 = mx * 8;
    }
    jd_idct_block(coef + idx * 64, qt, pl + y0 * stride + x0, stride);
}

__global__ __launch_bounds__(kJdThreads) void k_jd_idct(const JdFile *__restrict__ files, const aej_jpegdec_desc *__restrict__ descs, int n,
                                                        long long n_blocks, const short *__restrict__ coef, unsigned char *__restrict__ planes)
{
    jd_idct_thread<false>(files, descs, n, n_blocks, coef, planes, nullptr);
}

__global__ __launch_bounds__(kJdThreads) void k_jd_idct4(const JdFile *__restrict__ files, const aej_jpegdec_desc *__restrict__ descs, int n,
                                                         long long n_blocks, const short *__restrict__ coef, unsigned char *__restrict__ planes,
                                                         const aej_jpeg_adobe *__restrict__ adobe)
{
    jd_idct_thread<true>(files, descs, n, n_blocks, coef, planes, adobe);
}

// kJdAdobePx consecutive pixels [r0, r1) of a file with kJdAdobe, kCh output channels: the samples of every plane up-sampled by
// jd_chroma (component 3 sampled as component 0 is read as it is), the colour model's rule, and the bytes stored -- a whole
// group whose first byte is dword-aligned as kCh dwords, anything else byte by byte
template <int kCh>
__device__ __forceinline__ void jd_adobe_group(const JdFile &F, const aej_jpegdec_desc &d, int colour, bool full3, const unsigned char *pl,
                                               unsigned char *img, long long r0, long long r1)
{
    const unsigned char *p1 = pl + (long long)F.pw0 * F.ph0, *p2 = p1 + (long long)F.pw1 * F.ph1, *p3 = p2 + (long long)F.pw1 * F.ph1;
    const int wc = (d.width + d.hs - 1) / d.hs, hc = (d.height + d.vs - 1) / d.vs;
    unsigned w[kCh] = {};
#pragma unroll
    for (int i = 0; i < kJdAdobePx; i++) {
        const long long r = r0 + i;
        if (r >= r1) break;
        const int y = (int)(r / d.width), x = (int)(r % d.width);
        int s[4];
        s[0] = pl[(long long)y * F.pw0 + x];
        s[1] = jd_chroma(p1, F.pw1, d.hs, d.vs, wc, hc, y, x);
        s[2] = jd_chroma(p2, F.pw1, d.hs, d.vs, wc, hc, y, x);
        s[3] = d.ncomp != 4 ? 0 : full3 ? p3[(long long)y * F.pw3 + x] : jd_chroma(p3, F.pw3, d.hs, d.vs, wc, hc, y, x);
        unsigned char o[4];
        jd_adobe_pixel(colour, kCh == 4, s, o);
#pragma unroll
        for (int c = 0; c < kCh; c++) w[(i * kCh + c) >> 2] |= (unsigned)o[c] << (8 * ((i * kCh + c) & 3));
    }
    unsigned char *gp = img + r0 * kCh;
    if (r1 - r0 == kJdAdobePx && ((uintptr_t)gp & 3) == 0) {
#pragma unroll
        for (int c = 0; c < kCh; c++) reinterpret_cast<unsigned *>(gp)[c] = w[c];
    } else {
        const int nb = (int)(r1 - r0) * kCh;
#pragma unroll
        for (int b = 0; b < kJdAdobePx * kCh; b++) if (b < nb) gp[b] = (unsigned char)(w[b >> 2] >> (8 * (b & 3)));
    }
}

// The files with another colour model than YCbCr (JdFile::shift & kJdAdobe; aej_jpeg_adobe::colour RGB, CMYK, YCCK), sample planes ->
// pixels, in the place of k_jd_rgb.  Workgroup `blockIdx.x` is workgroup g - grpa_base of its file, so the file, its colour model and
// its output form are the same for the whole workgroup: no lane diverges on them.  Thread t of the file takes the kJdAdobePx
// consecutive pixels (row-major over the image) from 4 t - lead on, lead in 0..3 chosen so that the group's first output byte is
// dword-aligned whatever the image's offset in the packed output (three channels; with four the groups start at pixel 0 and are
// aligned when the image is).  Bounds: only pixels r in [0, width * height) are read and stored, at img + r * channels; the plane
// reads are jd_chroma's, inside the real samples of each plane.
__global__ __launch_bounds__(kJdThreads) void k_jd_adobe(const JdFile *__restrict__ files, const aej_jpegdec_desc *__restrict__ descs,
                                                         const aej_jpeg_adobe *__restrict__ adobe, int n, const unsigned char *__restrict__ planes,
                                                         unsigned char *__restrict__ out)
{
    const int lo = jd_find_file<&JdFile::grpa_base>(files, n, blockIdx.x);
    const JdFile &F = files[lo];
    const aej_jpegdec_desc &d = descs[lo];
    if (!(F.shift & kJdAdobe) || d.hs > 2 || d.vs > 2) return;      // never: the host gives these workgroups to such files alone
    const int colour = adobe[lo].colour;
    const bool full3 = adobe[lo].h3 == d.hs && adobe[lo].v3 == d.vs, four = (F.shift & kJdCmyk) != 0;
    const long long npx = (long long)d.width * d.height;
    unsigned char *img = out + F.out_off;
    const int lead = four ? 0 : (4 - (int)((uintptr_t)img & 3)) & 3;      // pixel r of an RGB image starts at a + 3 r = a - r (mod 4)
    const long long first = (((long long)blockIdx.x - F.grpa_base) * kJdThreads + threadIdx.x) * kJdAdobePx - lead;
    const long long r0 = max(first, 0LL), r1 = min(first + kJdAdobePx, npx);
    if (r0 >= r1) return;
    const unsigned char *pl = planes + F.plane_off;
    if (four) jd_adobe_group<4>(F, d, colour, full3, pl, img, r0, r1);
    else jd_adobe_group<3>(F, d, colour, full3, pl, img, r0, r1);
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

// Scaled reconstruction, coefficients -> RGB in one kernel.  Workgroup `blockIdx.x` of the launch for scale 1 << kShift is run
// g - grp_base of its file: MCUs [g0, g0 + ng) of MCU row my.  m = 8 >> kShift samples per luma block side.
// LDS: three sample planes of 2m rows x kJdRun * 2m columns (the widest run: two luma blocks per MCU side) and the run's RGB rows.
// Bounds: block indices stay below the file's mcux * mcuy * blocks_per_mcu; LDS columns below ng * hs * m <= kCols for luma and
// (ng + 2) * nc <= kCols for chroma -- jd_up_chroma reads chroma column j of the pixel's own MCU and, for a 4:2:2 file, j - 1 or j + 1
// where the FILE has it: a column of MCUs [c0, c1), since a run's neighbour MCU is in them wherever the image has one; only bytes of
// pixels (y < oh, x < ow) of the file's own image are stored.
template <int kShift>
__global__ __launch_bounds__(kJdThreads) void k_jd_scaled(const JdFile *__restrict__ files, const aej_jpegdec_desc *__restrict__ descs, int n,
                                                          const short *__restrict__ coef, unsigned char *__restrict__ out)
{
    constexpr int m = 8 >> kShift, kRows = 2 * m, kCols = kJdRun * 2 * m, kRgbStride = kCols * 3 + 4;
    __shared__ unsigned char sy[kRows * kCols], scb[kRows * kCols], scr[kRows * kCols];
    __shared__ __align__(4) unsigned char srgb[kRows * kRgbStride];
    const int lo = jd_group_file(files, n, &JdFile::grp_base, kShift - 1);
    const JdFile &F = files[lo];
    const aej_jpegdec_desc &d = descs[lo];
    const int per_row = (d.mcux + kJdRun - 1) / kJdRun, g = (int)(blockIdx.x - F.grp_base[kShift - 1]);
    const int my = g / per_row, g0 = (g % per_row) * kJdRun, ng = min(kJdRun, d.mcux - g0);
    const bool color = d.ncomp == 3;
    const int hs = d.hs, vs = d.vs, nl = color ? hs * vs : 1, nc = jd_chroma_idct_size(hs, vs, m);
    const bool h2v1 = color && hs == 2 && vs == 1;    // the one layout whose chroma is still up-sampled
    const int uh = h2v1 ? 2 : 1, wc = (F.ow + 1) >> 1;      // its real chroma width
    const bool fancy = h2v1 && kShift < 3 && wc > 2;  // jd_up_chroma: no fancy up-sampling beside a 1 x 1 IDCT, nor for <= 2 samples
    const int c0 = fancy && g0 > 0 ? g0 - 1 : g0, c1 = fancy && g0 + ng < d.mcux ? g0 + ng + 1 : g0 + ng;      // MCUs whose chroma is needed
    const int nY = ng * nl, nC = color ? (c1 - c0) * 2 : 0;
    const int bw = (d.width + 7) / 8, bh = (d.height + 7) / 8;
    for (int i = threadIdx.x; i < nY + nC; i += kJdThreads) {
        int mcu, k, c, size;
        unsigned char *dst;
        if (i < nY) {
            mcu = g0 + i / nl; k = i % nl; c = 0; size = m;
            const int ky = k / hs, kx = k % hs;
            if (my * vs + ky >= bh || mcu * hs + kx >= bw) continue;      // dummy block of an edge MCU
            dst = sy + ky * m * kCols + ((mcu - g0) * hs + kx) * m;
        } else {
            const int j = i - nY;
            mcu = c0 + (j >> 1); c = 1 + (j & 1); k = nl + (j & 1); size = nc;
            dst = (c == 1 ? scb : scr) + (mcu - c0) * nc;
        }
        const short *cf = coef + (F.blk_base + ((long long)my * d.mcux + mcu) * d.blocks_per_mcu + k) * 64;
        if (size == m) jd_idct_sized(cf, d.qt[c], m, dst, kCols);
        else jd_idct_sized(cf, d.qt[c], 2 * m, dst, kCols);
    }
    __syncthreads();
    const int y0 = my * vs * m, x0 = g0 * hs * m;
    const int nrows = min(vs * m, F.oh - y0), ncols = min(ng * hs * m, F.ow - x0), nbytes = ncols * 3;
    unsigned char *img = out + F.out_off;
    for (int p = threadIdx.x; p < nrows * ncols; p += kJdThreads) {
        const int r = p / ncols, x = p % ncols;
        const int a = (int)((uintptr_t)(img + ((long long)(y0 + r) * F.ow + x0) * 3) & 3);      // the row sits in LDS as it does in its dwords
        unsigned char *o = srgb + r * kRgbStride + a + 3 * x;
        const int Y = sy[r * kCols + x];
        if (!color) { o[0] = o[1] = o[2] = (unsigned char)Y; continue; }
        // the file's chroma sample of column j is at column j - c0 * nc of the LDS rows, whose row r is the pixel's own (uv = 1)
        jd_rgb(Y, jd_up_chroma(scb, kCols, c0 * nc, uh, 1, fancy, wc, 0, r, x0 + x), jd_up_chroma(scr, kCols, c0 * nc, uh, 1, fancy, wc, 0, r, x0 + x), o);
    }
    __syncthreads();
    jd_store_rows<true>(img + ((long long)y0 * F.ow + x0) * 3, F.ow * 3, srgb, kRgbStride, nrows, nbytes);
}

// Scaled reconstruction of three-component files whose luma is sampled 1 x 2 (4:4:0): k_jd_scaled's plan -- workgroup `blockIdx.x` is run
// g - grp440_base of its file, MCUs [g0, g0 + ng) of MCU row my -- with the MCU m columns by 2m rows of output.  jd_chroma_idct_size gives
// this layout an m x m chroma IDCT at every scale, so the chroma is always up-sampled vertically (jd_up_chroma, uv = 2): h1v2 fancy at
// scales 2 and 4, replication beside the 1 x 1 IDCT of scale 8.  The filter reads the chroma row above the run's first and
// below its last: the vertical halo.  The chroma blocks of MCU rows my - 1 and my + 1, where the image has them, are reconstructed here
// a second time (the horizontal halo of k_jd_scaled does the same with its two neighbour MCUs), whole, into row sets of their own.
// LDS: luma 2m rows x kJdRun * m columns; per chroma plane three sets of m rows (above, own, below; one set of one row at scale 8);
// the run's RGB rows.  Bounds: a neighbour MCU row is only addressed when 0 <= row < mcuy, so block indices stay below the file's
// mcux * mcuy * 4; LDS rows of chroma stay in [m - 1, 2m] of 3m (the neighbour row, jd_up_far, is one off the run's own rows at most, and
// off them only where that MCU row exists); only bytes of pixels (y < oh, x < ow) of the file's own image are stored.
template <int kShift>
__global__ __launch_bounds__(kJdThreads) void k_jd_scaled_h1v2(const JdFile *__restrict__ files, const aej_jpegdec_desc *__restrict__ descs, int n,
                                                               const short *__restrict__ coef, unsigned char *__restrict__ out)
{
    constexpr int m = 8 >> kShift, kCols = kJdRun * m, kRgbStride = kCols * 3 + 4;
    constexpr bool kFancy = kShift < 3;               // no fancy up-sampling beside a 1 x 1 IDCT
    constexpr int kSets = kFancy ? 3 : 1;
    __shared__ unsigned char sy[2 * m * kCols], scb[kSets * m * kCols], scr[kSets * m * kCols];
    __shared__ __align__(4) unsigned char srgb[2 * m * kRgbStride];
    const int lo = jd_group_file(files, n, &JdFile::grp440_base, kShift - 1);
    const JdFile &F = files[lo];
    const aej_jpegdec_desc &d = descs[lo];
    const int per_row = (d.mcux + kJdRun - 1) / kJdRun, g = (int)(blockIdx.x - F.grp440_base[kShift - 1]);
    const int my = g / per_row, g0 = (g % per_row) * kJdRun, ng = min(kJdRun, d.mcux - g0);
    if (my >= d.mcuy || d.hs != 1 || d.vs != 2 || d.ncomp != 3) return;      // never: the host gives these workgroups to such files alone
    const int bh = (d.height + 7) / 8, hc = (F.oh + 1) >> 1;                 // real luma block rows; real chroma rows
    const bool up = kFancy && my > 0, down = kFancy && my + 1 < d.mcuy;
    const int nY = ng * 2, nC = ng * 2 * (1 + (int)up + (int)down);
    for (int i = threadIdx.x; i < nY + nC; i += kJdThreads) {
        int mcu, k, c, row = my;
        unsigned char *dst;
        if (i < nY) {
            mcu = g0 + (i >> 1); k = i & 1; c = 0;
            if (my * 2 + k >= bh) continue;           // the dummy lower block of the last MCU row
            dst = sy + k * m * kCols + (mcu - g0) * m;
        } else {
            const int j = i - nY, set = j / (2 * ng), jj = j - set * 2 * ng;
            const int which = set == 0 ? 1 : (set == 1 && up) ? 0 : 2;       // 0: the MCU row above, 1: the run's own, 2: the one below
            mcu = g0 + (jj >> 1); c = 1 + (jj & 1); k = 2 + (jj & 1);
            row = my + which - 1;
            dst = (c == 1 ? scb : scr) + (kFancy ? which : 0) * m * kCols + (mcu - g0) * m;
        }
        const short *cf = coef + (F.blk_base + ((long long)row * d.mcux + mcu) * 4 + k) * 64;
        jd_idct_sized(cf, d.qt[c], m, dst, kCols);
    }
    __syncthreads();
    const int y0 = my * 2 * m, x0 = g0 * m;
    const int nrows = min(2 * m, F.oh - y0), ncols = min(ng * m, F.ow - x0), nbytes = ncols * 3;
    unsigned char *img = out + F.out_off;
    // the file's chroma row i is row i - (first row of the sets) of the LDS rows: the sets start at the MCU row above the run's, or, the
    // one set of scale 8, at the run's own.  No column is up-sampled, so the rule is given the run's columns as they lie in LDS
    const int coff = (kFancy ? my - 1 : my) * m * kCols;
    for (int p = threadIdx.x; p < nrows * ncols; p += kJdThreads) {
        const int r = p / ncols, x = p % ncols;
        const int a = (int)((uintptr_t)(img + ((long long)(y0 + r) * F.ow + x0) * 3) & 3);      // the row sits in LDS as it does in its dwords
        unsigned char *o = srgb + r * kRgbStride + a + 3 * x;
        jd_rgb(sy[r * kCols + x], jd_up_chroma(scb, kCols, coff, 1, 2, kFancy, 0, hc, y0 + r, x), jd_up_chroma(scr, kCols, coff, 1, 2, kFancy, 0, hc, y0 + r, x), o);
    }
    __syncthreads();
    jd_store_rows<true>(img + ((long long)y0 * F.ow + x0) * 3, F.ow * 3, srgb, kRgbStride, nrows, nbytes);
}

// Luma-only reconstruction, coefficients -> [oh][ow] in one kernel, at every scale 1 << kShift (0: full size) and for every layout: the
// luma blocks of an MCU are the first hs * vs of its blocks_per_mcu whatever the chroma is, and the chroma blocks are never read.
// k_jd_scaled's plan: workgroup `blockIdx.x` is run g - grpl_base of its file, MCUs [g0, g0 + ng) of MCU row my; m = 8 >> kShift.
// LDS: one sample plane of 2m rows x kJdRun * 2m columns (the widest run).  Bounds: block indices stay below the file's
// mcux * mcuy * blocks_per_mcu; LDS columns below ng * hs * m <= kCols, rows below vs * m <= kRows; only bytes of pixels (y < oh,
// x < ow) of the file's own image are stored -- whole dwords inside a row, single bytes at its unaligned ends.
template <int kShift>
__global__ __launch_bounds__(kJdThreads) void k_jd_luma(const JdFile *__restrict__ files, const aej_jpegdec_desc *__restrict__ descs, int n,
                                                        const short *__restrict__ coef, unsigned char *__restrict__ out)
{
    constexpr int m = 8 >> kShift, kRows = 2 * m, kCols = kJdRun * 2 * m;
    __shared__ unsigned char sy[kRows * kCols];
    const int lo = jd_group_file(files, n, &JdFile::grpl_base, kShift);
    const JdFile &F = files[lo];
    const aej_jpegdec_desc &d = descs[lo];
    const int per_row = (d.mcux + kJdRun - 1) / kJdRun, g = (int)(blockIdx.x - F.grpl_base[kShift]);
    const int my = g / per_row, g0 = (g % per_row) * kJdRun, ng = min(kJdRun, d.mcux - g0);
    const int hs = d.ncomp == 3 ? d.hs : 1, vs = d.ncomp == 3 ? d.vs : 1, nl = hs * vs;
    if (my >= d.mcuy || hs > 2 || vs > 2) return;     // never: the host gives a file mcuy * per_row workgroups, the parsers these factors
    const int bw = (d.width + 7) / 8, bh = (d.height + 7) / 8;
    for (int i = threadIdx.x; i < ng * nl; i += kJdThreads) {
        const int mcu = g0 + i / nl, k = i % nl, ky = k / hs, kx = k % hs;
        if (my * vs + ky >= bh || mcu * hs + kx >= bw) continue;      // dummy block of an edge MCU
        const short *cf = coef + (F.blk_base + ((long long)my * d.mcux + mcu) * d.blocks_per_mcu + k) * 64;
        unsigned char *dst = sy + ky * m * kCols + ((mcu - g0) * hs + kx) * m;
        if (kShift == 0) jd_idct_block(cf, d.qt[0], dst, kCols);      // inlined, as in k_jd_idct: 154 VGPRs, against 248 through jd_idct_block_call
        else jd_idct_sized(cf, d.qt[0], m, dst, kCols);
    }
    __syncthreads();
    const int y0 = my * vs * m, x0 = g0 * hs * m;
    const int nrows = min(vs * m, F.oh - y0), nbytes = min(ng * hs * m, F.ow - x0);
    unsigned char *img = out + F.out_off;
    jd_store_rows<false>(img + (long long)y0 * F.ow + x0, F.ow, sy, kCols, nrows, nbytes);
}

// The 8 x 8 block behind a call, for k_jd_sbox<1> alone (the 2m x 2m chroma IDCT of a 4:2:0 file at scale 2): a function of its own, not
// jd_idct_block_call, because sharing that one changes how k_jd_scaled<1> compiles (the trap k_jd_luma<0> met)
__device__ __attribute__((noinline)) void jd_idct_block_sbox(const short *c, const uint16_t *qt, unsigned char *dst)
{
    jd_idct_block(c, qt, dst, kJdBoxW);
}

// one block at IDCT size kN (1, 2, 4 or 8) into an LDS plane of k_jd_sbox<1..3>, kJdBoxW samples a row
template <int kN>
__device__ __forceinline__ void jd_sbox_idct(const short *c, const uint16_t *qt, unsigned char *dst)
{
    if constexpr (kN == 8) jd_idct_block_sbox(c, qt, dst);
    else if constexpr (kN == 4) jd_idct4_block(c, qt, dst, kJdBoxW);
    else if constexpr (kN == 2) jd_idct2_block(c, qt, dst, kJdBoxW);
    else dst[0] = jd_range_limit(jd_descale((long long)((int)c[0] * (int)qt[0]), 3));
}

// Boxed reconstruction at scale 1 << kShift (kShift 0: full size), coefficients -> the pixels of a box of the image at that scale in one
// kernel, for every layout (4:4:4, 4:2:2, 4:2:0, 4:4:0, one component) and both outputs: RGB (a one-component file: R = G = B), or the
// luma plane alone where the file's shift carries kJdLuma.  m = 8 >> kShift samples per luma block side, so an MCU covers hs * m x vs * m
// pixels.  Workgroup `blockIdx.x` is tile g - grps_base[kShift] of its file: tiles of kJdBoxW x kJdBoxH pixels -- TX = 128 / (hs * m) by
// TY = 32 / (vs * m) whole MCUs, for hs, vs in 1, 2 and m in 8, 4, 2, 1 -- in row-major order over the window win = (mx0, my0, mx1, my1)
// of jd_sbox_window, the grid anchored at the window's origin.  The tile's luma blocks go through the m x m IDCT into sy; its chroma
// blocks go at nc (jd_up_plan: 2m for 4:2:0 at a scale, where the chroma comes out at luma resolution; m otherwise) into scb / scr,
// with a ring of one MCU on either side in every direction that is still up-sampled by 2 and not replicated (jd_up_chroma: columns where
// uh = 2, rows where uv = 2, neither beside a 1 x 1 IDCT nor where uh = 2 meets a plane at most two samples wide), the ring clipped to the
// window: by jd_sbox_window every sample a pixel of the box reads lies in the window, so the clip drops nothing that is read.  The
// pixels of the tile that lie in the box then run jd_up_chroma -- indexed so that the FILE's sample (row, column) addresses the LDS
// plane, hence the file's own edge rules -- and jd_rgb, and are stored, byte by byte: a box's rows start at any byte.  Every return in
// front of the barrier depends on the workgroup alone.  At scale 8 a tile is up to 4096 one-coefficient luma blocks, so the IDCT loop
// makes several passes per thread.  The 8 x 8 IDCT of kShift 0 is inlined, as in k_jd_idct and k_jd_luma<0>: 164 VGPRs, occupancy 3;
// through jd_idct_block_call 248, occupancy 2, and k_jd_scaled<1>, which shares that function, no longer compiles as it did.
// LDS: three planes of kJdBoxH rows x kJdBoxW columns, 12 KiB.  Luma: TY * vs * m = 32 rows, TX * hs * m = 128 columns.  Chroma, in
// samples: (TY + 2 ry) * nc rows x (TX + 2 rx) * nc columns with rx, ry in 0, 1 the ring, and nc = hs * m / uh = vs * m / uv, so
// TX * nc = 128 / uh and TY * nc = 32 / uv.  No ring (uh = uv = 1, or replication): at most 32 x 128.  uh = 2: 64 + 2 nc <= 80 columns;
// uv = 2: 16 + 2 nc <= 32 rows (nc <= 8).
// Bounds: MCU rows [cy0, cy1) and [ty0, ty1) lie in [win[1], win[3]), which the stored rows [row0, row0 + n_blocks / (mcux * bpm))
// contain, and MCU columns in [win[0], win[2]) <= mcux, so block indices stay inside the file's stored coefficients; LDS rows and
// columns stay below (cy1 - cy0) * nc and (cx1 - cx0) * nc, the figures above; jd_up_chroma reads samples of MCUs [cy0, cy1) x
// [cx0, cx1) only (the pixel's own MCU and, through the ring, the clamped neighbour's, which the window holds); a store goes to pixel
// (y, x) with t <= y < b and l <= x < r only, at out_off + ((y - t) * (r - l) + (x - l)) * channels, inside the box's image.
template <int kShift>
__global__ __launch_bounds__(kJdThreads) void k_jd_sbox(const JdFile *__restrict__ files, const aej_jpegdec_desc *__restrict__ descs, int n,
                                                        const short *__restrict__ coef, unsigned char *__restrict__ out)
{
    constexpr int m = 8 >> kShift;
    __shared__ unsigned char sy[kJdBoxH * kJdBoxW], scb[kJdBoxH * kJdBoxW], scr[kJdBoxH * kJdBoxW];
    const int lo = jd_group_file(files, n, &JdFile::grps_base, kShift);
    const JdFile &F = files[lo];
    const aej_jpegdec_desc &d = descs[lo];
    if (!(F.shift & kJdBox) || (F.shift & (kJdLuma - 1)) != kShift) return;      // never: the host gives these workgroups to such files alone
    const bool three = d.ncomp == 3, color = three && !(F.shift & kJdLuma);
    const int hs = three ? d.hs : 1, vs = three ? d.vs : 1, nl = hs * vs, bpm = d.blocks_per_mcu;
    if (hs > 2 || vs > 2) return;                     // never: the parsers admit these factors alone
    const int TX = kJdBoxW / (hs * m), TY = kJdBoxH / (vs * m);
    const int ntx = (F.win[2] - F.win[0] + TX - 1) / TX, g = (int)(blockIdx.x - F.grps_base[kShift]);
    const int tx0 = F.win[0] + (g % ntx) * TX, ty0 = F.win[1] + (g / ntx) * TY;
    if (ty0 >= F.win[3]) return;                      // never: the host gives a file ntx * nty workgroups
    const int tx1 = min(tx0 + TX, F.win[2]), ty1 = min(ty0 + TY, F.win[3]);
    const bool wide = kShift > 0 && hs == 2 && vs == 2;      // 4:2:0 at a scale: the chroma IDCT is 2m
    const int nc = wide ? 2 * m : m, uh = wide ? 1 : hs, uv = wide ? 1 : vs;      // jd_up_plan for these factors
    const int sw = (d.width + (1 << kShift) - 1) >> kShift, sh = (d.height + (1 << kShift) - 1) >> kShift;      // the image at this scale
    const int wc = uh == 2 ? (sw + 1) >> 1 : sw, hc = uv == 2 ? (sh + 1) >> 1 : sh;
    constexpr bool fancy = kShift < 3;                // no fancy up-sampling beside a 1 x 1 IDCT
    const bool ring = color && !jd_up_replicates(uh, fancy, wc);
    const int rx = ring && uh == 2, ry = ring && uv == 2;      // the ring, in MCUs
    const int cx0 = max(tx0 - rx, F.win[0]), cx1 = min(tx1 + rx, F.win[2]), cy0 = max(ty0 - ry, F.win[1]), cy1 = min(ty1 + ry, F.win[3]);
    const int ntw = tx1 - tx0, nY = ntw * (ty1 - ty0) * nl, ncx = cx1 - cx0, nC = color ? 2 * ncx * (cy1 - cy0) : 0;
    for (int i = threadIdx.x; i < nY + nC; i += kJdThreads) {
        int mx, my, k, c;
        unsigned char *dst;
        if (i < nY) {
            const int mcu = i / nl, ky = (i % nl) / hs, kx = (i % nl) % hs;
            my = ty0 + mcu / ntw; mx = tx0 + mcu % ntw; k = i % nl; c = 0;
            dst = sy + (((my - ty0) * vs + ky) * m) * kJdBoxW + ((mx - tx0) * hs + kx) * m;
        } else {
            const int j = (i - nY) >> 1;
            c = 1 + ((i - nY) & 1); k = nl + c - 1;
            my = cy0 + j / ncx; mx = cx0 + j % ncx;
            dst = (c == 1 ? scb : scr) + ((my - cy0) * nc) * kJdBoxW + (mx - cx0) * nc;
        }
        const short *cf = coef + (F.blk_base + ((long long)(my - F.row0) * d.mcux + mx) * bpm + k) * 64;
        if constexpr (kShift == 0) jd_idct_block(cf, d.qt[c], dst, kJdBoxW);
        else if (c != 0 && wide) jd_sbox_idct<2 * m>(cf, d.qt[c], dst);
        else jd_sbox_idct<m>(cf, d.qt[c], dst);
    }
    __syncthreads();
    const int l = F.box[0], t = F.box[1], bw = F.box[2] - l;
    const int px0 = max(l, tx0 * hs * m), px1 = min(F.box[2], tx1 * hs * m), py0 = max(t, ty0 * vs * m), py1 = min(F.box[3], ty1 * vs * m);
    const int ncols = px1 - px0, npx = ncols > 0 && py1 > py0 ? ncols * (py1 - py0) : 0;
    unsigned char *img = out + F.out_off;
    // the file's chroma sample (row, column) is at scb[row * kJdBoxW + column - coff]: only formed for rows and columns of [cy0, cy1) x [cx0, cx1)
    const long long coff = (long long)cy0 * nc * kJdBoxW + cx0 * nc;
    for (int p = threadIdx.x; p < npx; p += kJdThreads) {
        const int y = py0 + p / ncols, x = px0 + p % ncols;
        const int Y = sy[(y - ty0 * vs * m) * kJdBoxW + (x - tx0 * hs * m)];
        const long long o = (long long)(y - t) * bw + (x - l);
        if (!color) {
            if (F.shift & kJdLuma) img[o] = (unsigned char)Y;
            else { unsigned char *q = img + o * 3; q[0] = q[1] = q[2] = (unsigned char)Y; }
            continue;
        }
        jd_rgb(Y, jd_up_chroma(scb, kJdBoxW, coff, uh, uv, fancy, wc, hc, y, x), jd_up_chroma(scr, kJdBoxW, coff, uh, uv, fancy, wc, hc, y, x), img + o * 3);
    }
}

// ---- host: descriptor checks, layout and launch sequence -----------------------------------------------------------------------------------
bool jpegdec_descs_ok(const aej_jpegdec_desc *d, int n, const aej_jpeg_adobe *adobe)
{
    if (!d || n < 1) return false;
    for (int i = 0; i < n; i++) {
        const aej_jpegdec_desc &e = d[i];
        if (!jpeg_frame_ok(e, adobe ? adobe + i : nullptr) || e.scan_length < 0 || e.restart_interval < 0) return false;
        const long long mcus = (long long)e.mcux * e.mcuy;
        if (e.n_segments != (e.restart_interval ? (mcus + e.restart_interval - 1) / e.restart_interval : 1)) return false;
    }
    return true;
}

void jpeg_stream_layout(long long len, int n_segments, int S, JdFile &F, JdBufSizes &z)
{
    F.scan_len = len;
    F.clean_off = z.clean;
    z.clean += align_up(len, 4) + 16;
    F.chunk_base = z.chunks;
    F.n_chunks = (len + kJdChunk - 1) / kJdChunk;
    z.chunks += F.n_chunks;
    F.seg_base = z.segs;
    z.segs += n_segments;
    F.slot_base = z.slots;
    F.n_slots = n_segments + (len * 8 + S - 1) / S + 1;
    z.slots += F.n_slots;
}

void jpeg_recon_layout(const aej_jpegdec_desc &d, int shift, JdFile &F, JdBufSizes &z, const int *box, bool window_coef, const aej_jpeg_adobe *x)
{
    // a box: of the full-size image (the callers refuse one at another scale), or -- kJdSbox in shift, set by the _sbox entries for a box
    // that is not the whole scaled image -- of the image at scale 2, 4 or 8
    const bool luma = (shift & kJdLuma) != 0, boxed = (shift & kJdSbox) != 0 || ((shift & (kJdLuma - 1)) == 0 && !jpeg_box_whole(d, box));
    F.blk_base = z.blocks;
    F.n_blocks = (long long)d.mcux * d.mcuy * d.blocks_per_mcu;
    F.row0 = 0;
    for (int s = 0; s < 4; s++) F.grps_base[s] = z.grps[s];
    if (boxed) {
        for (int v = 0; v < 4; v++) F.box[v] = box[v];
        jd_sbox_window(d.width, d.height, d.hs, d.vs, d.ncomp, luma, shift & (kJdLuma - 1), box, F.win);
        if (window_coef) {                            // the window's MCU rows alone, at full width
            F.row0 = F.win[1];
            F.n_blocks = (long long)d.mcux * (F.win[3] - F.win[1]) * d.blocks_per_mcu;
        }
    }
    z.blocks += F.n_blocks;
    F.shift = shift;
    shift &= kJdLuma - 1;
    F.ow = (d.width + (1 << shift) - 1) >> shift; F.oh = (d.height + (1 << shift) - 1) >> shift;
    for (int s = 0; s < 3; s++) { F.grp_base[s] = z.grp[s]; F.grp440_base[s] = z.grp440[s]; }
    for (int s = 0; s < 4; s++) F.grpl_base[s] = z.grpl[s];
    F.plane_off = z.planes;
    F.px_base = z.px;
    F.grpa_base = z.grpa;
    F.pw3 = F.ph3 = 0;
    if (jpeg_adobe_new(x)) {                          // four sample planes (three for an RGB-coded file), no pixels of k_jd_rgb's: workgroups of k_jd_adobe
        F.shift |= kJdAdobe;
        F.pw0 = d.mcux * 8 * d.hs; F.ph0 = d.mcuy * 8 * d.vs;
        F.pw1 = d.mcux * 8; F.ph1 = d.mcuy * 8;
        if (d.ncomp == 4) { F.pw3 = d.mcux * 8 * x->h3; F.ph3 = d.mcuy * 8 * x->v3; }
        z.planes += align_up((long long)F.pw0 * F.ph0 + 2LL * F.pw1 * F.ph1 + (long long)F.pw3 * F.ph3, 256);
        const long long groups = ((long long)d.width * d.height + kJdAdobePx - 1) / kJdAdobePx + 1;      // one more: the lead group
        z.grpa += (groups + kJdThreads - 1) / kJdThreads;
        return;
    }
    if (boxed) {                                      // no sample planes, no pixels of k_jd_rgb's, no workgroups but k_jd_sbox<shift>'s
        const int m = 8 >> shift;                     // samples per luma block side: 8, or with kJdSbox 4, 2, 1
        const int hs = d.ncomp == 3 ? d.hs : 1, vs = d.ncomp == 3 ? d.vs : 1, TX = kJdBoxW / (m * hs), TY = kJdBoxH / (m * vs);
        F.shift |= kJdBox;
        F.ow = box[2] - box[0]; F.oh = box[3] - box[1];
        F.pw0 = F.ph0 = F.pw1 = F.ph1 = 0;
        z.grps[shift] += (long long)((F.win[2] - F.win[0] + TX - 1) / TX) * ((F.win[3] - F.win[1] + TY - 1) / TY);
        return;
    }
    if (luma) {                                       // at every scale: no sample planes, no pixels of k_jd_rgb's, workgroups of k_jd_luma<shift>
        F.pw0 = F.ph0 = F.pw1 = F.ph1 = 0;
        z.grpl[shift] += (long long)d.mcuy * ((d.mcux + kJdRun - 1) / kJdRun);
        return;
    }
    if (shift) {                                      // no sample planes, no pixels of k_jd_rgb's: workgroups of k_jd_scaled<shift>
        F.pw0 = F.ph0 = F.pw1 = F.ph1 = 0;
        const bool h1v2 = d.ncomp == 3 && d.hs == 1 && d.vs == 2;      // 4:4:0: k_jd_scaled_h1v2's grid
        (h1v2 ? z.grp440 : z.grp)[shift - 1] += (long long)d.mcuy * ((d.mcux + kJdRun - 1) / kJdRun);
        return;
    }
    F.pw0 = d.mcux * 8 * d.hs; F.ph0 = d.mcuy * 8 * d.vs;
    F.pw1 = d.ncomp == 3 ? d.mcux * 8 : 0; F.ph1 = d.ncomp == 3 ? d.mcuy * 8 : 0;
    z.planes += align_up((long long)F.pw0 * F.ph0 + 2LL * F.pw1 * F.ph1, 256);
    z.px += (long long)d.width * d.height;
}

void jpegdec_layout(const aej_jpegdec_desc *descs, int n, int S, std::vector<JdFile> &files, JdBufSizes &z, const JdResolved &r)
{
    const aej_jpeg_adobe *adobe = r.adobe;
    files.assign(n, JdFile{});
    z = JdBufSizes{};
    for (int i = 0; i < n; i++) {
        jpeg_stream_layout(descs[i].scan_length, descs[i].n_segments, S, files[i], z);
        jpeg_recon_layout(descs[i], r.shifts.empty() ? 0 : r.shifts[i], files[i], z, r.boxes ? r.boxes + 4 * i : nullptr, true, adobe ? adobe + i : nullptr);
        if (descs[i].ncomp == 3 || (adobe && jpeg_adobe_new(adobe + i))) {      // one DC and one AC table for every component?
            const aej_jpegdec_desc &d = descs[i];
            bool same = !memcmp(&d.dc[1], &d.dc[0], sizeof d.dc[0]) && !memcmp(&d.dc[2], &d.dc[0], sizeof d.dc[0]) &&
                        !memcmp(&d.ac[1], &d.ac[0], sizeof d.ac[0]) && !memcmp(&d.ac[2], &d.ac[0], sizeof d.ac[0]);
            if (d.ncomp == 4) same = same && !memcmp(&adobe[i].dc3, &d.dc[0], sizeof d.dc[0]) && !memcmp(&adobe[i].ac3, &d.ac[0], sizeof d.ac[0]);
            files[i].uniform = same;
            z.uniform += same;
        }
    }
}

// The kFour slot kernels run for a call with a four-component or RGB-coded file, and for one with a file whose components all decode
// under one table pair (JdFile::uniform) -- a three-component one too: a flat page saved with optimised tables is such a file, and the
// plain kernels would need one sync round per subsequence for it, since no bit ever corrects a wrong block slot.
static bool jd_four(const JdBufSizes &z) { return z.grpa > 0 || z.uniform > 0; }

unsigned long long jpegdec_carve(void *base, int n, const JdBufSizes &z, JdBufs &w)
{
    Carver c(base);
    w.files = (JdFile *)c.take<char>(sizeof(JdFile) * n + sizeof(aej_jpegdec_desc) * n + 16);      // one upload: see JdBufs
    w.descs = base ? (aej_jpegdec_desc *)((char *)w.files + sizeof(JdFile) * n) : nullptr;
    w.last_change = base ? (int *)((char *)w.descs + sizeof(aej_jpegdec_desc) * n) : nullptr;
    const bool four = jd_four(z);                     // the kFour slot kernels: the files' aej_jpeg_adobe (a second upload, when the call has any), a fourth DC sum per slot
    w.adobe = four ? c.take<aej_jpeg_adobe>(n) : nullptr;
    w.cnt = c.take<int>(z.chunks * 3);
    w.pre = c.take<long long>(z.chunks * 3);
    w.clean_len = c.take<long long>(n);
    w.segs = c.take<JdSeg>(z.segs);
    w.clean = c.take<unsigned char>(z.clean);
    w.sl.state = c.take<unsigned long long>(z.slots);
    w.sl.used = c.take<unsigned long long>(z.slots);
    w.sl.cnt = c.take<int>(z.slots * (four ? 5 : 4));
    w.sl.first = c.take<unsigned char>(z.slots);
    w.sl.blk_pre = c.take<long long>(z.slots);
    w.sl.dc_pre = c.take<int>(z.slots * (four ? 4 : 3));
    w.coef = c.take<short>(z.blocks * 64);
    w.planes = c.take<unsigned char>(z.planes);
    return c.bytes();
}

static unsigned jd_grid(long long n) { return (unsigned)((n + kJdThreads - 1) / kJdThreads); }

// everything up to the first read-back: upload, un-stuffing, segments, first guesses
hipError_t launch_jpegdec_begin(hipStream_t st, int n, const JdBufSizes &z, const JdBufs &w, const void *blob_host, unsigned long long blob_bytes,
                                const unsigned char *scans, int S, int *status)
{
    hipError_t e = hipMemcpyAsync(w.files, blob_host, blob_bytes, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return e;
    if ((e = launch_jpegdec_unstuff(st, n, z, w, scans, S, status)) != hipSuccess) return e;
    if (jd_four(z)) {
        hipLaunchKernelGGL(k_jd_init4, dim3(jd_grid(z.slots)), dim3(kJdThreads), 0, st, w.files, w.descs, n, z.slots, w.segs, w.clean, w.sl, S,
                           w.last_change, w.adobe);
    } else {
        hipLaunchKernelGGL(jpeg_any_box(z) ? k_jd_init<true> : k_jd_init<false>, dim3(jd_grid(z.slots)), dim3(kJdThreads), 0, st, w.files, w.descs, n,
                           z.slots, w.segs, w.clean, w.sl, S, w.last_change);
    }
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
    for (int r = first_round; r < first_round + rounds; r++) {
        if (jd_four(z))
            hipLaunchKernelGGL(k_jd_sync4, dim3(jd_grid(z.slots)), dim3(kJdThreads), 0, st, w.files, w.descs, n, z.slots, w.segs, w.clean, w.sl, S, r,
                               w.last_change, w.adobe);
        else
            hipLaunchKernelGGL(jpeg_any_box(z) ? k_jd_sync<true> : k_jd_sync<false>, dim3(jd_grid(z.slots)), dim3(kJdThreads), 0, st, w.files, w.descs, n,
                               z.slots, w.segs, w.clean, w.sl, S, r, w.last_change);
    }
    return hipGetLastError();
}

// after the last sync round: the coefficients of every file (natural order, MCU order, dummy blocks included) and the decode's status words
hipError_t launch_jpegdec_write(hipStream_t st, int n, const JdBufSizes &z, const JdBufs &w, int S, int *status)
{
    hipError_t e = hipMemsetAsync(w.coef, 0, (size_t)z.blocks * 128, st);
    if (e != hipSuccess) return e;
    if (jd_four(z)) {
        hipLaunchKernelGGL(k_jd_scan_slots4, dim3(n), dim3(kJdScanThreads), 0, st, w.files, w.sl);
        if (z.uniform > 0) {                          // files whose bits do not tell the block slot: DC sums again under the slots the block counts give
            hipLaunchKernelGGL(k_jd_fix4, dim3(jd_grid(z.slots)), dim3(kJdThreads), 0, st, w.files, w.descs, n, z.slots, w.segs, w.clean, w.sl, S, w.adobe);
            hipLaunchKernelGGL(k_jd_scan_slots4, dim3(n), dim3(kJdScanThreads), 0, st, w.files, w.sl);
        }
        hipLaunchKernelGGL(k_jd_write4, dim3(jd_grid(z.slots)), dim3(kJdThreads), 0, st, w.files, w.descs, n, z.slots, w.segs, w.clean, w.sl, S, w.coef,
                           status, w.adobe);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(k_jd_scan_slots, dim3(n), dim3(kJdScanThreads), 0, st, w.files, w.sl);
    hipLaunchKernelGGL(jpeg_any_box(z) ? k_jd_write<true> : k_jd_write<false>, dim3(jd_grid(z.slots)), dim3(kJdThreads), 0, st, w.files, w.descs, n, z.slots,
                       w.segs, w.clean, w.sl, S, w.coef, status);
    return hipGetLastError();
}

hipError_t launch_jpegdec_finish(hipStream_t st, int n, const JdBufSizes &z, const JdBufs &w, int S, unsigned char *out, int *status)
{
    const hipError_t e = launch_jpegdec_write(st, n, z, w, S, status);
    if (e != hipSuccess) return e;
    return launch_jpegdec_recon(st, n, z, w, out);
}

// the files of a call that decode at scale 2, 4, 8, the luma-only ones at every scale and the boxed ones: one launch per kernel and scale present
// (JdFile::shift and ::grp_base / ::grp440_base / ::grpl_base pick a file's kernel and workgroups; the layout inside the kernel follows
// the file's sampling factors)
static hipError_t launch_jpegdec_recon_scaled(hipStream_t st, int n, const JdBufSizes &z, const JdBufs &w, unsigned char *out)
{
    if (z.grp[0] > 0) hipLaunchKernelGGL(k_jd_scaled<1>, dim3((unsigned)z.grp[0]), dim3(kJdThreads), 0, st, w.files, w.descs, n, w.coef, out);
    if (z.grp[1] > 0) hipLaunchKernelGGL(k_jd_scaled<2>, dim3((unsigned)z.grp[1]), dim3(kJdThreads), 0, st, w.files, w.descs, n, w.coef, out);
    if (z.grp[2] > 0) hipLaunchKernelGGL(k_jd_scaled<3>, dim3((unsigned)z.grp[2]), dim3(kJdThreads), 0, st, w.files, w.descs, n, w.coef, out);
    if (z.grp440[0] > 0) hipLaunchKernelGGL(k_jd_scaled_h1v2<1>, dim3((unsigned)z.grp440[0]), dim3(kJdThreads), 0, st, w.files, w.descs, n, w.coef, out);
    if (z.grp440[1] > 0) hipLaunchKernelGGL(k_jd_scaled_h1v2<2>, dim3((unsigned)z.grp440[1]), dim3(kJdThreads), 0, st, w.files, w.descs, n, w.coef, out);
    if (z.grp440[2] > 0) hipLaunchKernelGGL(k_jd_scaled_h1v2<3>, dim3((unsigned)z.grp440[2]), dim3(kJdThreads), 0, st, w.files, w.descs, n, w.coef, out);
    if (z.grpl[0] > 0) hipLaunchKernelGGL(k_jd_luma<0>, dim3((unsigned)z.grpl[0]), dim3(kJdThreads), 0, st, w.files, w.descs, n, w.coef, out);
    if (z.grpl[1] > 0) hipLaunchKernelGGL(k_jd_luma<1>, dim3((unsigned)z.grpl[1]), dim3(kJdThreads), 0, st, w.files, w.descs, n, w.coef, out);
    if (z.grpl[2] > 0) hipLaunchKernelGGL(k_jd_luma<2>, dim3((unsigned)z.grpl[2]), dim3(kJdThreads), 0, st, w.files, w.descs, n, w.coef, out);
    if (z.grpl[3] > 0) hipLaunchKernelGGL(k_jd_luma<3>, dim3((unsigned)z.grpl[3]), dim3(kJdThreads), 0, st, w.files, w.descs, n, w.coef, out);
    if (z.grps[0] > 0) hipLaunchKernelGGL(k_jd_sbox<0>, dim3((unsigned)z.grps[0]), dim3(kJdThreads), 0, st, w.files, w.descs, n, w.coef, out);
    if (z.grps[1] > 0) hipLaunchKernelGGL(k_jd_sbox<1>, dim3((unsigned)z.grps[1]), dim3(kJdThreads), 0, st, w.files, w.descs, n, w.coef, out);
    if (z.grps[2] > 0) hipLaunchKernelGGL(k_jd_sbox<2>, dim3((unsigned)z.grps[2]), dim3(kJdThreads), 0, st, w.files, w.descs, n, w.coef, out);
    if (z.grps[3] > 0) hipLaunchKernelGGL(k_jd_sbox<3>, dim3((unsigned)z.grps[3]), dim3(kJdThreads), 0, st, w.files, w.descs, n, w.coef, out);
    if (z.grpa > 0) {                                 // the four-component and RGB-coded files: four sample planes, then their pixels
        hipLaunchKernelGGL(k_jd_idct4, dim3(jd_grid(z.blocks)), dim3(kJdThreads), 0, st, w.files, w.descs, n, z.blocks, w.coef, w.planes, w.adobe);
        hipLaunchKernelGGL(k_jd_adobe, dim3((unsigned)z.grpa), dim3(kJdThreads), 0, st, w.files, w.descs, w.adobe, n, w.planes, out);
    }
    return hipGetLastError();
}

// coefficients (natural order, MCU order) -> RGB or luma, for n files: the full-size RGB ones (z.px counts their pixels), then the rest
hipError_t launch_jpegdec_recon(hipStream_t st, int n, const JdBufSizes &z, const JdBufs &w, unsigned char *out)
{
    if (z.px > 0) {
        hipLaunchKernelGGL(k_jd_idct, dim3(jd_grid(z.blocks)), dim3(kJdThreads), 0, st, w.files, w.descs, n, z.blocks, w.coef, w.planes);
        hipLaunchKernelGGL(k_jd_rgb, dim3(jd_grid(z.px)), dim3(kJdThreads), 0, st, w.files, w.descs, n, z.px, w.planes, out);
    }
    return launch_jpegdec_recon_scaled(st, n, z, w, out);
}

// ---- host: the entropy decode stepped through on the CPU (aej_test_jpegdec_coefs_host) ------------------------------------------------------
// One or three components.  Un-stuffs as k_jd_count / k_jd_scatter do (jd_byte_class, RSTn numbers checked), then one jd_run<true> per
// restart segment from its first bit to its last: what the sync rounds' fixed point and k_jd_write give, without subsequences.
int jpegdec_coefs_host(const aej_jpegdec_desc &d, const unsigned char *file, unsigned long long nbytes, short *coef, unsigned long long coef_blocks)
{
    if ((d.ncomp != 1 && d.ncomp != 3) || d.blocks_per_mcu < 1 || d.blocks_per_mcu > 6 || d.mcux < 1 || d.mcuy < 1 || d.n_segments < 1) return AEJ_ERR_ARG;
    if (d.scan_offset < 0 || d.scan_length < 0 || (unsigned long long)d.scan_offset + (unsigned long long)d.scan_length > nbytes) return AEJ_ERR_ARG;
    const long long total = (long long)d.mcux * d.mcuy, blocks = total * d.blocks_per_mcu;
    if ((unsigned long long)blocks > coef_blocks) return AEJ_ERR_CAPACITY;
    memset(coef, 0, (size_t)blocks * 128);
    const unsigned char *s = file + d.scan_offset;
    std::vector<unsigned> words((size_t)(d.scan_length / 4 + 8), 0u);
    unsigned char *clean = reinterpret_cast<unsigned char *>(words.data());
    std::vector<JdSeg> segs(1, JdSeg{});
    long long o = 0;
    for (long long p = 0; p < d.scan_length; p++) {
        const int c = jd_byte_class(s, d.scan_length, p);
        if (c == kJdByteEnd) break;
        if (c == kJdByteData) clean[o++] = s[p];
        else if (c == kJdByteRst) {
            if ((s[p] & 7) != (int)((segs.size() - 1) & 7)) return AEJ_JPEGDEC_BAD_RESTART;
            JdSeg g{};
            g.start = o;
            segs.push_back(g);
        }
    }
    if ((long long)segs.size() != d.n_segments) return AEJ_JPEGDEC_BAD_RESTART;
    const long long ri = d.restart_interval ? d.restart_interval : total;
    for (size_t g = 0; g < segs.size(); g++) {
        JdSeg &sg = segs[g];
        sg.nbytes = (g + 1 < segs.size() ? segs[g + 1].start : o) - sg.start;
        sg.first_mcu = (int)std::min((long long)g * ri, total);
        sg.n_mcu = (int)std::min(ri, total - sg.first_mcu);
        JdBits br(clean);
        long long pos = sg.start * 8, next = 0;
        const long long seg_end = (sg.start + sg.nbytes) * 8, seg_blocks = (long long)sg.n_mcu * d.blocks_per_mcu;
        int k = 0, z = 0, nstart = 0, dc[3] = {}, pred[3] = {};
        const int rc = jd_run<true>(d, br, pos, k, z, seg_end, seg_end, nstart, dc, coef + (long long)sg.first_mcu * d.blocks_per_mcu * 64, next,
                                    seg_blocks, pred);
        if (rc == kJdRunDone) continue;
        if (rc == kJdRunStop) {
            if ((z == 0 ? next : next - 1) < seg_blocks) return AEJ_JPEGDEC_TRUNCATED;
            continue;
        }
        return rc == kJdRunOutOfBits ? AEJ_JPEGDEC_TRUNCATED : rc == kJdRunBadCode ? AEJ_JPEGDEC_BAD_CODE
             : rc == kJdRunPast63 ? AEJ_JPEGDEC_RUN_PAST_63 : AEJ_JPEGDEC_BAD_DC;
    }
    return 0;
}

}  // namespace aej
