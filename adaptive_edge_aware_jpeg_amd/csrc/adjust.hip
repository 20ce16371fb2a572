// adjust.hip -- Pillow's ImageEnhance (Brightness, Contrast, Color, Sharpness), ImageOps.autocontrast / equalize / posterize / solarize /
// invert / grayscale, Image.point and Image.histogram on the device (aej_adjust_*, aej_histogram_batch), bit for bit, over many packed
// 8-bit images of 1 to 4 channels, of different sizes and chains, in one call.  include/aej.h has the arithmetic.
//
//   k_adjust_hist<C>          the histogram of one pass: a workgroup takes a chunk of kAdChunk pixels of one image, evaluates the steps
//                             before the statistics op in registers, counts into one LDS histogram PER WAVE (a constant image sends
//                             every lane of a wave to one bin; the waves at least do not meet), merges the waves and adds the
//                             non-zero bins to the image's counters with no-return integer atomics: order-free, so deterministic
//   k_adjust_luts             one workgroup per image and statistics op, one lane per band: the 256-step walks of ImageOps.py in int64
//                             and float64; also the widening of aej_histogram_batch
//   k_adjust_apply<C, GRAY>   reads each source byte once, applies the whole segment per pixel in registers (tables staged in LDS),
//                             writes each output byte once
// A lane takes 16 / 8 / 4 / 4 adjacent pixels of 1 / 2 / 3 / 4 channels: 16 bytes (12 for RGB) by one vector access at whatever address
// the packed image has -- the hardware splits a misaligned one --, and the last pixels of an image byte by byte.  A launch is one grid
// over every image that needs it (a per-image entry, a prefix sum of chunks, a binary search by chunk, as warp.hip's); the grid is
// capped at kAdMaxGrid and the workgroups stride.  Bounds: a lane touches pixel q only if q < npix; a table index is masked to 8 bits.
#include <math.h>
#include <string.h>

#include <vector>

#include "aej_ctx.h"

#pragma clang fp contract(off)

namespace aej {

template <int kC> struct AdLane { static constexpr int pix = kC == 1 ? 16 : kC == 2 ? 8 : 4; };

__device__ __forceinline__ int ad_luma(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

// kP pixels from pixel q on (q < npix): one vector access when all kP exist, else byte by byte (the missing ones are 0)
template <int kC, int kP>
__device__ __forceinline__ void ad_load(const unsigned char *__restrict__ p, long long q, long long npix, int (&px)[kP][kC])
{
    if (q + kP <= npix) {
        unsigned w[kP * kC / 4];
        __builtin_memcpy(w, p + q * kC, kP * kC);
#pragma unroll
        for (int i = 0; i < kP; i++)
#pragma unroll
            for (int b = 0; b < kC; b++) {
                const int at = i * kC + b;
                px[i][b] = (int)((w[at >> 2] >> (8 * (at & 3))) & 255u);
            }
    } else {
#pragma unroll
        for (int i = 0; i < kP; i++)
#pragma unroll
            for (int b = 0; b < kC; b++) px[i][b] = q + i < npix ? (int)p[(q + i) * kC + b] : 0;
    }
}

// the tables of the entry's steps into LDS, a dword per lane (a table is 1024 bytes and 256-byte aligned)
__device__ __forceinline__ void ad_stage(const AdEntry &e, unsigned char *tab)
{
    for (int k = 0; k < e.n_steps; k++) {
        const int kind = e.step[k].kind, slot = e.step[k].slot;
        if (kind != AEJ_ADJUST_CONTRAST && kind != AEJ_ADJUST_AUTOCONTRAST && kind != AEJ_ADJUST_EQUALIZE && kind != AEJ_ADJUST_LUT) continue;
        const unsigned *s = (const unsigned *)(e.tables + slot * AEJ_ADJUST_TABLE_BYTES);
        unsigned *d = (unsigned *)(tab + slot * AEJ_ADJUST_TABLE_BYTES);
        for (int i = threadIdx.x; i < AEJ_ADJUST_TABLE_BYTES / 4; i += kAdThreads) d[i] = s[i];
    }
}

// the steps of one entry on kP pixels: -> the channels left (kC, or 1 after a GRAYSCALE)
template <int kC, int kP>
__device__ __forceinline__ int ad_run(const AdEntry &e, const unsigned char *tab, int (&px)[kP][kC], const int (&dg)[kP][kC])
{
    int c = kC;
    for (int k = 0; k < e.n_steps; k++) {
        const AdStep st = e.step[k];
        const float a = st.factor;
        const bool inside = a >= 0.f && a <= 1.f;
        const unsigned char *t = tab + (st.slot & (AEJ_ADJUST_MAX_OPS - 1)) * AEJ_ADJUST_TABLE_BYTES;
        const int nc = c - ((c == 2 || c == 4) ? 1 : 0);      // colour bands: alpha passes through
        if (st.kind == AEJ_ADJUST_BRIGHTNESS || st.kind == AEJ_ADJUST_CONTRAST) {
            const int d = st.kind == AEJ_ADJUST_CONTRAST ? (int)t[0] : 0;
#pragma unroll
            for (int i = 0; i < kP; i++)
#pragma unroll
                for (int b = 0; b < kC; b++)
                    if (b < nc) px[i][b] = ad_blend(d, px[i][b], a, inside);
        } else if (st.kind == AEJ_ADJUST_COLOR) {
            if constexpr (kC >= 3) {
                if (c >= 3) {
#pragma unroll
                    for (int i = 0; i < kP; i++) {
                        const int L = ad_luma(px[i][0], px[i][1], px[i][2]);
#pragma unroll
                        for (int b = 0; b < 3; b++) px[i][b] = ad_blend(L, px[i][b], a, inside);
                    }
                }
            }
        } else if (st.kind == AEJ_ADJUST_SHARPNESS) {
#pragma unroll
            for (int i = 0; i < kP; i++)
#pragma unroll
                for (int b = 0; b < kC; b++)
                    if (b < nc) px[i][b] = ad_blend(dg[i][b], px[i][b], a, inside);
        } else if (st.kind == AEJ_ADJUST_GRAYSCALE) {
            if constexpr (kC >= 3) {
                if (c >= 3) {
#pragma unroll
                    for (int i = 0; i < kP; i++) px[i][0] = ad_luma(px[i][0], px[i][1], px[i][2]);
                }
            }
            c = 1;
        } else {                                              // AUTOCONTRAST, EQUALIZE, LUT: a table per band
#pragma unroll
            for (int i = 0; i < kP; i++)
#pragma unroll
                for (int b = 0; b < kC; b++)
                    if (b < c) px[i][b] = (int)t[b * 256 + (px[i][b] & 255)];
        }
    }
    return c;
}

template <int kC>
__global__ __launch_bounds__(kAdThreads) void k_adjust_hist(const AdEntry *__restrict__ entries, int n, long long chunks)
{
    constexpr int kP = AdLane<kC>::pix, kWaves = kAdThreads / 64;
    __shared__ unsigned wh[kWaves][kC * 256];
    __shared__ __align__(16) unsigned char tab[AEJ_ADJUST_MAX_OPS * AEJ_ADJUST_TABLE_BYTES];
    unsigned *mine = wh[threadIdx.x >> 6];
    for (long long chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const AdEntry &e = chunk_entry(entries, n, chunk);
        ad_stage(e, tab);
        for (int i = threadIdx.x; i < kWaves * kC * 256; i += kAdThreads) (&wh[0][0])[i] = 0u;
        __syncthreads();
        const long long p0 = (chunk - e.chunk_base) * kAdChunk;
        const bool sharp = e.n_steps > 0 && e.step[0].kind == AEJ_ADJUST_SHARPNESS;
        for (int j = 0; j < kAdChunk / (kAdThreads * kP); j++) {
            const long long q = p0 + ((long long)j * kAdThreads + threadIdx.x) * kP;
            if (q >= e.npix) continue;
            int px[kP][kC], dg[kP][kC] = {};
            ad_load<kC, kP>(e.in, q, e.npix, px);
            if (sharp) ad_load<kC, kP>(e.deg, q, e.npix, dg);
            const int c = ad_run<kC, kP>(e, tab, px, dg);
#pragma unroll
            for (int i = 0; i < kP; i++) {
                if (q + i >= e.npix) continue;
                if (e.luma) {
                    int L = px[i][0];
                    if constexpr (kC >= 3) {
                        if (c >= 3) L = ad_luma(px[i][0], px[i][1], px[i][2]);
                    }
                    atomicAdd(&mine[L & 255], 1u);
                } else {
#pragma unroll
                    for (int b = 0; b < kC; b++)
                        if (b < c) atomicAdd(&mine[b * 256 + (px[i][b] & 255)], 1u);
                }
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < e.bins && i < kC * 256; i += kAdThreads) {
            unsigned s = 0;
#pragma unroll
            for (int w = 0; w < kWaves; w++) s += wh[w][i];
            if (s) atomicAdd(&e.hist[i], s);
        }
        __syncthreads();
    }
}

template <int kC, bool kGray>
__global__ __launch_bounds__(kAdThreads) void k_adjust_apply(const AdEntry *__restrict__ entries, int n, long long chunks)
{
    constexpr int kP = AdLane<kC>::pix, kOut = kGray ? 1 : kC;
    __shared__ __align__(16) unsigned char tab[AEJ_ADJUST_MAX_OPS * AEJ_ADJUST_TABLE_BYTES];
    for (long long chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const AdEntry &e = chunk_entry(entries, n, chunk);
        ad_stage(e, tab);
        __syncthreads();
        const long long p0 = (chunk - e.chunk_base) * kAdChunk;
        const bool sharp = e.n_steps > 0 && e.step[0].kind == AEJ_ADJUST_SHARPNESS;
        for (int j = 0; j < kAdChunk / (kAdThreads * kP); j++) {
            const long long q = p0 + ((long long)j * kAdThreads + threadIdx.x) * kP;
            if (q >= e.npix) continue;
            int px[kP][kC], dg[kP][kC] = {};
            ad_load<kC, kP>(e.in, q, e.npix, px);
            if (sharp) ad_load<kC, kP>(e.deg, q, e.npix, dg);
            ad_run<kC, kP>(e, tab, px, dg);
            unsigned char *o = e.out + q * kOut;
            if (q + kP <= e.npix) {
                unsigned w[kP * kOut / 4] = {};
#pragma unroll
                for (int i = 0; i < kP; i++)
#pragma unroll
                    for (int b = 0; b < kOut; b++) {
                        const int at = i * kOut + b;
                        w[at >> 2] |= (unsigned)(px[i][b] & 255) << (8 * (at & 3));
                    }
                __builtin_memcpy(o, w, kP * kOut);
            } else {
#pragma unroll
                for (int i = 0; i < kP; i++)
#pragma unroll
                    for (int b = 0; b < kOut; b++)
                        if (q + i < e.npix) o[i * kOut + b] = (unsigned char)px[i][b];
            }
        }
        __syncthreads();                                      // the next chunk's tables replace these
    }
}

// Python's float floor division for vx >= 0, wx > 0 (floatobject.c)
__device__ __forceinline__ double ad_floordiv(double vx, double wx)
{
    const double mod = fmod(vx, wx), div = (vx - mod) / wx;
    if (div == 0.0) return 0.0;
    double fl = floor(div);
    if (div - fl > 0.5) fl += 1.0;
    return fl;
}

__global__ __launch_bounds__(64) void k_adjust_luts(const AdLutEntry *__restrict__ entries)
{
    __shared__ long long hh[3][256];
    const AdLutEntry &e = entries[blockIdx.x];
    if (e.kind == kAdWiden) {
        for (int i = threadIdx.x; i < e.bands * 256; i += 64) e.wide[i] = (long long)e.hist[i];
        return;
    }
    const int band = threadIdx.x;
    if (band >= e.bands || band >= 3) return;
    const unsigned *h = e.hist + band * 256;
    if (e.kind == AEJ_ADJUST_CONTRAST) {
        long long sum = 0;
        for (int i = 0; i < 256; i++) sum += (long long)i * (long long)h[i];
        const double mean = (double)sum / (double)e.npix;
        e.table[0] = (unsigned char)(int)(mean + 0.5);
        return;
    }
    long long *g = hh[band];
    int mode = 0;                                             // 0 the identity, 1 autocontrast's line, 2 equalize's running sum
    double scale = 0.0, offset = 0.0;
    long long step = 0;
    if (e.kind == AEJ_ADJUST_AUTOCONTRAST) {
        long long n = 0;
        for (int i = 0; i < 256; i++) {
            g[i] = ((e.ignore[i >> 5] >> (i & 31)) & 1u) ? 0 : (long long)h[i];
            n += g[i];
        }
        long long cut = (long long)ad_floordiv((double)n * e.cutoff[0], 100.0);
        for (int lo = 0; lo < 256; lo++) {
            if (cut > g[lo]) { cut -= g[lo]; g[lo] = 0; } else { g[lo] -= cut; cut = 0; }
            if (cut <= 0) break;
        }
        cut = (long long)ad_floordiv((double)n * e.cutoff[1], 100.0);
        for (int hi = 255; hi >= 0; hi--) {
            if (cut > g[hi]) { cut -= g[hi]; g[hi] = 0; } else { g[hi] -= cut; cut = 0; }
            if (cut <= 0) break;
        }
        int lo = 255, hi = 0;
        for (int i = 0; i < 256; i++) if (g[i]) { lo = i; break; }
        for (int i = 255; i >= 0; i--) if (g[i]) { hi = i; break; }
        if (hi > lo) {
            mode = 1;
            scale = 255.0 / (double)(hi - lo);
            offset = (double)(-lo) * scale;
        }
    } else {                                                  // AEJ_ADJUST_EQUALIZE
        long long sum = 0, last = 0;
        int nonzero = 0;
        for (int i = 0; i < 256; i++)
            if (h[i]) { nonzero++; sum += h[i]; last = h[i]; }
        step = nonzero > 1 ? (sum - last) / 255 : 0;
        if (step) mode = 2;
    }
    long long acc = step / 2;
    for (int i = 0; i < 256; i++) {
        long long v = i;
        if (mode == 1) v = (long long)((double)i * scale + offset);
        if (mode == 2) { v = acc / step; acc += h[i]; }
        v = v < 0 ? 0 : v > 255 ? 255 : v;
        for (int k = 0; k < e.copies; k++) e.table[(band + k) * 256 + i] = (unsigned char)v;
    }
}

// ---- host: what one chain becomes, and the plan of a call ---------------------------------------------------------------------------
static bool ad_statistics(int kind) { return kind == AEJ_ADJUST_CONTRAST || kind == AEJ_ADJUST_AUTOCONTRAST || kind == AEJ_ADJUST_EQUALIZE; }

struct AdSeg { int first, count, cin, cout, sharp; };
struct AdChain { int n_seg; AdSeg seg[AEJ_ADJUST_MAX_OPS]; int ch_at[AEJ_ADJUST_MAX_OPS]; };      // ch_at: the channels op k sees

static int ad_chain(const aej_adjust_desc &d, int n_tables, bool histogram, aej_adjust_plan &p, AdChain &ch, const char **why)
{
    memset(&p, 0, sizeof p);
    memset(&ch, 0, sizeof ch);
    if (d.width < 1 || d.height < 1 || d.width > kAdMaxSide || d.height > kAdMaxSide) { *why = "sizes from 1 to 32767 a side"; return AEJ_ERR_ARG; }
    if (d.channels < 1 || d.channels > 4) { *why = "1 to 4 channels"; return AEJ_ERR_ARG; }
    if (d.src_offset < 0 || d.dst_offset < 0) { *why = "negative offset"; return AEJ_ERR_ARG; }
    p.out_channels = d.channels;
    if (histogram) {
        if (d.n_ops != 0) { *why = "a histogram takes no ops"; return AEJ_ERR_ARG; }
        p.n_passes = 1;
        p.n_launches = 2;
        return 0;
    }
    if (d.n_ops < 1 || d.n_ops > AEJ_ADJUST_MAX_OPS) { *why = "a chain of 1 to 8 ops"; return AEJ_ERR_ARG; }
    int c = d.channels;
    AdSeg *s = &ch.seg[0];
    *s = { 0, 0, c, c, 0 };
    ch.n_seg = 1;
    for (int k = 0; k < d.n_ops; k++) {
        const aej_adjust_op &op = d.ops[k];
        ch.ch_at[k] = c;
        switch (op.kind) {
        case AEJ_ADJUST_BRIGHTNESS: case AEJ_ADJUST_CONTRAST: case AEJ_ADJUST_COLOR: case AEJ_ADJUST_SHARPNESS:
            if (!isfinite(op.factor)) { *why = "a factor that is not finite"; return AEJ_ERR_ARG; }
            break;
        case AEJ_ADJUST_AUTOCONTRAST:
            if (!isfinite(op.cutoff[0]) || !isfinite(op.cutoff[1]) || op.cutoff[0] < 0 || op.cutoff[1] < 0) { *why = "a cutoff that is negative or not finite"; return AEJ_ERR_ARG; }
            [[fallthrough]];
        case AEJ_ADJUST_EQUALIZE:
            if (c != 1 && c != 3) { *why = "a histogram table op on an image of 2 or 4 channels"; return AEJ_ERR_ARG; }
            break;
        case AEJ_ADJUST_LUT:
            if (n_tables >= 0 && (op.table < 0 || op.table >= n_tables)) { *why = "a table number outside the tables"; return AEJ_ERR_ARG; }
            break;
        case AEJ_ADJUST_GRAYSCALE:
            break;
        default:
            *why = "unknown op";
            return AEJ_ERR_ARG;
        }
        if (op.kind == AEJ_ADJUST_SHARPNESS) {
            p.n_smooths++;
            if (k > 0) {
                p.segment_first[ch.n_seg] = k;
                s = &ch.seg[ch.n_seg++];
                *s = { k, 0, c, c, 0 };
            }
            s->sharp = 1;
        }
        if (ad_statistics(op.kind)) p.n_passes++;
        if (op.kind == AEJ_ADJUST_GRAYSCALE) c = 1;
        s->count++;
        s->cout = c;
    }
    p.out_channels = c;
    p.n_segments = ch.n_seg;
    p.n_launches = 2 * p.n_passes + p.n_smooths + p.n_segments;
    return 0;
}

int adjust_resolve(const aej_adjust_desc &d, int n_tables, aej_adjust_plan &p, const char **why)
{
    AdChain ch;
    return ad_chain(d, n_tables, false, p, ch, why);
}

template <typename T> static T *ad_at(T *p, long long n) { return p ? p + n : nullptr; }

// -> 0, or the error code with *bad the image and *why the reason.  workspace NULL: everything but the device pointers, and plan.bytes.
int adjust_plan(const aej_adjust_desc *descs, int n, const unsigned char *tables_host, int n_tables, bool histogram, void *workspace,
                const unsigned char *src, unsigned char *dst, AdPlan &plan, int *bad, const char **why)
{
    plan = AdPlan();
    std::vector<AdChain> chain(n);
    std::vector<aej_adjust_plan> ap(n);
    int max_seg = 0;
    long long n_hists = 0;
    for (int i = 0; i < n; i++) {
        *bad = i;
        const int code = ad_chain(descs[i], n_tables, histogram, ap[i], chain[i], why);
        if (code) return code;
        const long long npix = (long long)descs[i].width * descs[i].height;
        plan.spans.reads.push_back({ i, descs[i].src_offset, npix * descs[i].channels });
        plan.spans.writes.push_back({ i, descs[i].dst_offset, histogram ? (long long)descs[i].channels * 256 : npix * ap[i].out_channels });
        max_seg = std::max(max_seg, chain[i].n_seg);
        n_hists += ap[i].n_passes;
    }
    *bad = -1;
    // ---- the counts: entries and table entries, launch by launch (first walk), so that the workspace can be carved before the pointers are set
    Carver cv(workspace);
    std::vector<unsigned char *> plane0(n, nullptr), plane1(n, nullptr), smooth(n, nullptr);
    long long n_entries = 0, n_luts = 0;
    for (int i = 0; i < n; i++) {
        n_entries += ap[i].n_passes + ap[i].n_segments;
        n_luts += ap[i].n_passes;
    }
    plan.entries_dev = cv.take<unsigned char>(n_entries * (long long)sizeof(AdEntry));
    plan.luts_dev = cv.take<unsigned char>(n_luts * (long long)sizeof(AdLutEntry));
    plan.tables_dev = cv.take<unsigned char>(histogram ? 0 : (long long)n * AEJ_ADJUST_MAX_OPS * AEJ_ADJUST_TABLE_BYTES);
    plan.hists_dev = cv.take<unsigned>(n_hists * kAdHistWords);
    plan.n_hists = n_hists;
    for (int i = 0; i < n && !histogram; i++) {
        if (chain[i].n_seg >= 2) plane0[i] = cv.take<unsigned char>(plan.spans.reads[i].bytes);
        if (chain[i].n_seg >= 3) plane1[i] = cv.take<unsigned char>(plan.spans.reads[i].bytes);
        if (ap[i].n_smooths) smooth[i] = cv.take<unsigned char>(plan.spans.reads[i].bytes);
    }
    if (!histogram) {
        plan.tables.assign((size_t)n * AEJ_ADJUST_MAX_OPS * AEJ_ADJUST_TABLE_BYTES, 0);
        for (int i = 0; i < n && tables_host; i++)
            for (int k = 0; k < descs[i].n_ops; k++)
                if (descs[i].ops[k].kind == AEJ_ADJUST_LUT)
                    memcpy(&plan.tables[((size_t)i * AEJ_ADJUST_MAX_OPS + k) * AEJ_ADJUST_TABLE_BYTES],
                           tables_host + (size_t)descs[i].ops[k].table * AEJ_ADJUST_TABLE_BYTES, AEJ_ADJUST_TABLE_BYTES);
    }
    // ---- the launches
    long long hist_at = 0;
    auto entry_of = [&](int i, const AdSeg &sg, int s, int n_steps) {
        const aej_adjust_desc &d = descs[i];
        AdEntry e;
        memset(&e, 0, sizeof e);
        e.in = s == 0 ? (src ? src + d.src_offset : nullptr) : ((s - 1) & 1) ? plane1[i] : plane0[i];
        e.deg = sg.sharp ? smooth[i] : nullptr;
        e.tables = ad_at(plan.tables_dev, (long long)i * AEJ_ADJUST_MAX_OPS * AEJ_ADJUST_TABLE_BYTES);
        e.npix = (long long)d.width * d.height;
        e.n_steps = n_steps;
        for (int k = 0; k < n_steps; k++) e.step[k] = { d.ops[sg.first + k].kind, sg.first + k, d.ops[sg.first + k].factor, 0 };
        return e;
    };
    auto push_launch = [&](AdLaunch l) -> int {
        l.count = (int)(l.kernel == 1 ? plan.luts.size() : plan.entries.size()) - l.first;
        if (!l.count && l.kernel != 3) return 0;
        plan.launches.push_back(l);
        return 0;
    };
    if (histogram) {
        for (int cin = 1; cin <= 4; cin++) {
            AdLaunch l = { 0, cin, 0, (int)plan.entries.size(), 0, 0, 0 };
            for (int i = 0; i < n; i++) {
                if (descs[i].channels != cin) continue;
                AdSeg sg = { 0, 0, cin, cin, 0 };
                AdEntry e = entry_of(i, sg, 0, 0);
                e.tables = nullptr;
                e.hist = ad_at(plan.hists_dev, (long long)i * kAdHistWords);
                e.bins = cin * 256;
                e.chunk_base = l.chunks;
                l.chunks += (e.npix + kAdChunk - 1) / kAdChunk;
                plan.entries.push_back(e);
            }
            push_launch(l);
        }
        AdLaunch l = { 1, 0, 0, 0, 0, 0, 0 };
        for (int i = 0; i < n; i++) {
            AdLutEntry u;
            memset(&u, 0, sizeof u);
            u.hist = ad_at(plan.hists_dev, (long long)i * kAdHistWords);
            u.wide = dst ? (long long *)dst + descs[i].dst_offset : nullptr;
            u.kind = kAdWiden;
            u.bands = descs[i].channels;
            plan.luts.push_back(u);
        }
        push_launch(l);
        plan.bytes = cv.bytes();
        return 0;
    }
    for (int s = 0; s < max_seg; s++) {
        // SMOOTH of the segment's input, for the images whose segment s opens with a SHARPNESS
        std::vector<aej_window_desc> wd;
        std::vector<int> wi;
        int max_pass = 0;
        for (int i = 0; i < n; i++) {
            if (s >= chain[i].n_seg) continue;
            const AdSeg &sg = chain[i].seg[s];
            int np = 0;
            for (int k = 0; k < sg.count; k++) np += ad_statistics(descs[i].ops[sg.first + k].kind);
            max_pass = std::max(max_pass, np);
            if (!sg.sharp) continue;
            aej_window_desc w;
            memset(&w, 0, sizeof w);
            w.width = descs[i].width; w.height = descs[i].height; w.channels = sg.cin;
            w.kind = AEJ_WINDOW_KERNEL; w.size = 3; w.scale = 13.f; w.offset = 0.f;
            for (int k = 0; k < 9; k++) w.kernel[k] = k == 4 ? 5.f : 1.f;
            wd.push_back(w);
            wi.push_back(i);
        }
        if (!wd.empty()) {
            plan.smooths.emplace_back();
            AdSmooth &sm = plan.smooths.back();
            int wbad = -1;
            const int code = window_plan(wd.data(), (int)wd.size(), sm.plan, &wbad, why);
            if (code) { *bad = wbad >= 0 ? wi[wbad] : -1; return code; }
            sm.blob = sm.plan.entries;
            for (size_t k = 0; k < sm.blob.size(); k++) {
                const int i = wi[sm.plan.image[k]];
                AdSeg sg = chain[i].seg[s];
                sm.blob[k].in = entry_of(i, sg, s, 0).in;
                sm.blob[k].out = smooth[i];
            }
            sm.blob_dev = cv.take<unsigned char>((long long)(sm.blob.size() * sizeof(WnEntry)));
            AdLaunch l = { 3, 0, 0, 0, 0, (int)plan.smooths.size() - 1, 0 };
            plan.launches.push_back(l);
        }
        // the histogram passes of segment s
        for (int pass = 0; pass < max_pass; pass++) {
            std::vector<AdLutEntry> lut_round;
            for (int cin = 1; cin <= 4; cin++) {
                AdLaunch l = { 0, cin, 0, (int)plan.entries.size(), 0, 0, 0 };
                for (int i = 0; i < n; i++) {
                    if (s >= chain[i].n_seg || chain[i].seg[s].cin != cin) continue;
                    const AdSeg &sg = chain[i].seg[s];
                    int at = -1, seen = 0;
                    for (int k = 0; k < sg.count && at < 0; k++)
                        if (ad_statistics(descs[i].ops[sg.first + k].kind) && seen++ == pass) at = k;
                    if (at < 0) continue;
                    const aej_adjust_op &op = descs[i].ops[sg.first + at];
                    const int c = chain[i].ch_at[sg.first + at];
                    AdEntry e = entry_of(i, sg, s, at);
                    e.luma = op.kind == AEJ_ADJUST_CONTRAST || (op.kind == AEJ_ADJUST_AUTOCONTRAST && op.preserve_tone);
                    e.bins = e.luma ? 256 : c * 256;
                    e.hist = ad_at(plan.hists_dev, hist_at * kAdHistWords);
                    e.chunk_base = l.chunks;
                    l.chunks += (e.npix + kAdChunk - 1) / kAdChunk;
                    plan.entries.push_back(e);
                    AdLutEntry u;
                    memset(&u, 0, sizeof u);
                    u.hist = e.hist;
                    u.table = ad_at(plan.tables_dev, ((long long)i * AEJ_ADJUST_MAX_OPS + sg.first + at) * AEJ_ADJUST_TABLE_BYTES);
                    u.npix = e.npix;
                    u.kind = op.kind;
                    u.bands = e.luma ? 1 : c;
                    u.copies = e.luma && op.kind == AEJ_ADJUST_AUTOCONTRAST ? c : 1;
                    u.cutoff[0] = op.cutoff[0]; u.cutoff[1] = op.cutoff[1];
                    memcpy(u.ignore, op.ignore, sizeof u.ignore);
                    lut_round.push_back(u);
                    hist_at++;
                }
                push_launch(l);
            }
            AdLaunch l = { 1, 0, 0, (int)plan.luts.size(), 0, 0, 0 };
            plan.luts.insert(plan.luts.end(), lut_round.begin(), lut_round.end());
            push_launch(l);
        }
        // the apply launch of segment s
        for (int cin = 1; cin <= 4; cin++)
            for (int gray = 0; gray < 2; gray++) {
                AdLaunch l = { 2, cin, gray, (int)plan.entries.size(), 0, 0, 0 };
                for (int i = 0; i < n; i++) {
                    if (s >= chain[i].n_seg || chain[i].seg[s].cin != cin || (chain[i].seg[s].cout != cin) != (gray != 0)) continue;
                    const AdSeg &sg = chain[i].seg[s];
                    AdEntry e = entry_of(i, sg, s, sg.count);
                    e.out = s == chain[i].n_seg - 1 ? (dst ? dst + descs[i].dst_offset : nullptr) : (s & 1) ? plane1[i] : plane0[i];
                    e.chunk_base = l.chunks;
                    l.chunks += (e.npix + kAdChunk - 1) / kAdChunk;
                    plan.entries.push_back(e);
                }
                push_launch(l);
            }
    }
    plan.bytes = cv.bytes();
    return 0;
}

template <int kC>
static void ad_launch(hipStream_t st, const AdLaunch &l, const AdEntry *entries)
{
    const dim3 grid((unsigned)std::min<long long>(l.chunks, kAdMaxGrid)), block(kAdThreads);
    if (l.kernel == 0) hipLaunchKernelGGL(k_adjust_hist<kC>, grid, block, 0, st, entries, l.count, l.chunks);
    if (l.kernel == 2 && !l.gray) hipLaunchKernelGGL((k_adjust_apply<kC, false>), grid, block, 0, st, entries, l.count, l.chunks);
    if constexpr (kC > 1)
        if (l.kernel == 2 && l.gray) hipLaunchKernelGGL((k_adjust_apply<kC, true>), grid, block, 0, st, entries, l.count, l.chunks);
}

// everything of a call on one stream: the uploads, the zeroed histograms, the launches in order.  The caller waits.
hipError_t launch_adjust(hipStream_t st, const AdPlan &plan)
{
    hipError_t e = hipMemcpyAsync(plan.entries_dev, plan.entries.data(), plan.entries.size() * sizeof(AdEntry), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return e;
    if (!plan.luts.empty()) {
        e = hipMemcpyAsync(plan.luts_dev, plan.luts.data(), plan.luts.size() * sizeof(AdLutEntry), hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return e;
    }
    if (!plan.tables.empty()) {
        e = hipMemcpyAsync(plan.tables_dev, plan.tables.data(), plan.tables.size(), hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return e;
    }
    if (plan.n_hists) {
        e = hipMemsetAsync(plan.hists_dev, 0, (size_t)plan.n_hists * kAdHistWords * sizeof(unsigned), st);
        if (e != hipSuccess) return e;
    }
    for (const AdLaunch &l : plan.launches) {
        if (l.kernel == 3) {
            const AdSmooth &sm = plan.smooths[l.round];
            e = launch_window(st, sm.plan, sm.blob_dev, sm.blob.data());
            if (e != hipSuccess) return e;
            continue;
        }
        if (l.kernel == 1) {
            hipLaunchKernelGGL(k_adjust_luts, dim3((unsigned)l.count), dim3(64), 0, st, (const AdLutEntry *)plan.luts_dev + l.first);
            continue;
        }
        const AdEntry *entries = (const AdEntry *)plan.entries_dev + l.first;
        if (l.cin == 1) ad_launch<1>(st, l, entries);
        if (l.cin == 2) ad_launch<2>(st, l, entries);
        if (l.cin == 3) ad_launch<3>(st, l, entries);
        if (l.cin == 4) ad_launch<4>(st, l, entries);
    }
    return hipGetLastError();
}

}  // namespace aej
