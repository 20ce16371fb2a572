// lut3d.hip -- Pillow's Color3DLUT on the device (aej_lut3d_*), bit for bit, over many packed 8-bit images of 3 and 4 channels, of
// different sizes and tables, in one call.  include/aej.h has the arithmetic: the three colour bytes of a pixel pick a cell of the
// table and a 15-bit position in it, and the cell's eight corners are interpolated in integers, axis 1 first.
//
// A pixel's result depends on that pixel alone, so an image is a run of w * h pixels and a workgroup takes a tile of that run; a lane
// takes kLtRun = 4 adjacent pixels at a time: 3 or 4 dwords in, 3 or 4 dwords out, at whatever alignment the image has in its packed
// allocation (lt_load / lt_store, as window.hip's), and the last lane of an image its 1 to 3 pixels byte by byte.  On the device every
// table entry is four INT16 (lut3d_blob pads a 3-channel entry), so the two corners of an axis-1 pair are 16 adjacent bytes on an
// 8-byte boundary, whichever the table's channels.
// k_lut3d<ci, tc, co> reads the table where the upload put it, through L1 / L2 (the largest, 65^3, is 2.2 MB).  (A second path that
// staged tables of up to 8192 entries in LDS was measured and not kept: EXPERIMENTS.md, "Pillow's Color3DLUT".)
// A launch is one grid over every image of one (ci, tc, co) (a per-image entry, a prefix sum of workgroups, a binary search
// by blockIdx.x, as window.hip's).  Bounds: 255 divides no s_d - 1 in 1 .. 64, so 255 * scale_d < (s_d - 1) << 18, every cell_d is at
// most s_d - 2 and the furthest corner, entry cell + s12 + s1 + 1, is at most s1 s2 s3 - 1: no table read leaves the table, whatever
// the bytes.  A lane reads and writes only pixels below npix, so no image access leaves the image.
#include <math.h>
#include <string.h>

#include <vector>

#include "aej_ctx.h"

#pragma clang fp contract(off)

namespace aej {

// The images and the tables lie in device memory: said in the pointers' types, so that they are read and written with global
// instructions, which do not wait on the LDS counter as flat ones do
#define LT_GLOBAL __attribute__((address_space(1)))
typedef const LT_GLOBAL unsigned char *LtIn;
typedef LT_GLOBAL unsigned char *LtOut;
typedef unsigned long long LtWord;                // one table entry: four INT16, channel 0 lowest
typedef const LT_GLOBAL LtWord *LtTable;

// 4 * kW bytes at any address, or the first nb of them (the rest zero), as dwords
template <int kW>
__device__ __forceinline__ void lt_load(LtIn p, int nb, unsigned (&v)[kW])
{
    if (nb == 4 * kW) {
        __builtin_memcpy(v, p, 4 * kW);
    } else {
#pragma unroll
        for (int b = 0; b < 4 * kW; b++) {            // (unrolled: v stays in registers)
            if ((b & 3) == 0) v[b >> 2] = 0;
            if (b < nb) v[b >> 2] |= (unsigned)p[b] << (8 * (b & 3));
        }
    }
}

template <int kW>
__device__ __forceinline__ void lt_store(LtOut p, int nb, const unsigned (&v)[kW])
{
    if (nb == 4 * kW) {
        __builtin_memcpy(p, v, 4 * kW);
    } else {
#pragma unroll
        for (int b = 0; b < 4 * kW; b++)
            if (b < nb) p[b] = (unsigned char)(v[b >> 2] >> (8 * (b & 3)));
    }
}

// channel c of an entry, sign-extended
template <int c>
__device__ __forceinline__ int lt_chan(LtWord q) { return (int)(short)(unsigned short)(q >> (16 * c)); }

__device__ __forceinline__ int lt_lerp(int a, int b, int s) { return (a * (32768 - s) + b * s) >> 15; }

template <int c>
__device__ __forceinline__ unsigned lt_channel(const LtWord (&q)[8], int f1, int f2, int f3)
{
    const int l0 = lt_lerp(lt_chan<c>(q[0]), lt_chan<c>(q[1]), f1), l1 = lt_lerp(lt_chan<c>(q[2]), lt_chan<c>(q[3]), f1);
    const int l2 = lt_lerp(lt_chan<c>(q[4]), lt_chan<c>(q[5]), f1), l3 = lt_lerp(lt_chan<c>(q[6]), lt_chan<c>(q[7]), f1);
    const int v = lt_lerp(lt_lerp(l0, l1, f2), lt_lerp(l2, l3, f2), f3);
    return (unsigned)min(max((v + 32) >> 6, 0), 255);
}

// a workgroup takes the kLtTile pixels of its image from pixel (blockIdx.x - tile_base) * kLtTile on
template <int kCI, int kTC, int kCO>
__global__ __launch_bounds__(kLtThreads) void k_lut3d(const LtEntry *__restrict__ entries, int n)
{
    const LtEntry &e = tile_entry(entries, n);
    const LtTable tab = (LtTable)e.table;
    const unsigned sc1 = e.scale[0], sc2 = e.scale[1], sc3 = e.scale[2];
    const int s1 = e.s1, s12 = e.s12;
    const LtIn src = (LtIn)e.in;
    const LtOut dst = (LtOut)e.out;
    const long long p0 = ((long long)blockIdx.x - e.tile_base) * kLtTile, p1 = min(p0 + kLtTile, e.npix);
    for (long long p = p0 + (long long)threadIdx.x * kLtRun; p < p1; p += kLtThreads * kLtRun) {
        const int np = (int)min((long long)kLtRun, p1 - p);
        unsigned in[kCI], out[kCO];
        lt_load<kCI>(src + p * kCI, np * kCI, in);
#pragma unroll
        for (int k = 0; k < kCO; k++) out[k] = 0;
#pragma unroll
        for (int j = 0; j < kLtRun; j++) {
            auto byte_in = [&](int at) { return (in[at >> 2] >> (8 * (at & 3))) & 255u; };
            const unsigned i1 = byte_in(j * kCI) * sc1, i2 = byte_in(j * kCI + 1) * sc2, i3 = byte_in(j * kCI + 2) * sc3;
            const int f1 = (int)((i1 & 0x3FFFFu) >> 3), f2 = (int)((i2 & 0x3FFFFu) >> 3), f3 = (int)((i3 & 0x3FFFFu) >> 3);
            const int cell = (int)(i1 >> 18) + (int)(i2 >> 18) * s1 + (int)(i3 >> 18) * s12;
            const LtWord q[8] = { tab[cell], tab[cell + 1], tab[cell + s1], tab[cell + s1 + 1],
                                 tab[cell + s12], tab[cell + s12 + 1], tab[cell + s12 + s1], tab[cell + s12 + s1 + 1] };
            unsigned px[4];
            px[0] = lt_channel<0>(q, f1, f2, f3);
            px[1] = lt_channel<1>(q, f1, f2, f3);
            px[2] = lt_channel<2>(q, f1, f2, f3);
            if (kCO == 4) px[3] = kTC == 4 ? lt_channel<3>(q, f1, f2, f3) : byte_in(j * kCI + 3);      // (kCO 4 over kTC 3 has kCI 4)
#pragma unroll
            for (int c = 0; c < kCO; c++) {
                const int at = j * kCO + c;
                out[at >> 2] |= px[c] << (8 * (at & 3));
            }
        }
        lt_store<kCO>(dst + p * kCO, np * kCO, out);
    }
}

// ---- host: the float -> INT16 rule --------------------------------------------------------------------------------------------------
int lut3d_prepare(const float *table, long long n, short *out)
{
    const double hi = (32767 - 0.5) / 16320, lo = (-32768 + 0.5) / 16320;
    for (long long i = 0; i < n; i++)
        if (table[i] != table[i]) return AEJ_ERR_ARG;
    for (long long i = 0; i < n; i++) {
        const float v = table[i];
        if ((double)v >= hi) { out[i] = 32767; continue; }
        if ((double)v <= lo) { out[i] = -32768; continue; }
        const float p = v * 16320.0f;                 // rounded to float32: with a double product one sample in a few thousand differs
        out[i] = v < 0 ? (short)((double)p - 0.5) : (short)((double)p + 0.5);
    }
    return 0;
}

// ---- host: the plan of a call ---------------------------------------------------------------------------------------------------------
static const int kLtCombos[5][3] = { { 3, 3, 3 }, { 4, 3, 3 }, { 4, 3, 4 }, { 3, 4, 4 }, { 4, 4, 4 } };      // (ci, tc, co)

// -> 0, or the error code with *bad the image and *why the reason.  table_offsets NULL (the size query): the tables' lengths are not
// checked and their number is what the descriptors name.
int lut3d_plan(const aej_lut3d_desc *descs, int n, const long long *table_offsets, int n_tables, LtPlan &plan, int *bad, const char **why)
{
    plan = LtPlan();
    *bad = -1;
    if (!table_offsets) {
        n_tables = 0;
        for (int i = 0; i < n; i++)
            if (descs[i].table >= 0 && descs[i].table < n) n_tables = std::max(n_tables, descs[i].table + 1);
    }
    std::vector<LtEntry> image(n);
    std::vector<int> table_entries(n_tables, 0);
    plan.table_tc.assign(n_tables, 0);
    for (int i = 0; i < n; i++) {
        const aej_lut3d_desc &d = descs[i];
        LtEntry &e = image[i];
        memset(&e, 0, sizeof e);
        *bad = i;
        if (d.width < 1 || d.height < 1 || d.width > 65535 || d.height > 65535) { *why = "sizes from 1 to 65535 a side"; return AEJ_ERR_ARG; }
        if (d.src_offset < 0 || d.dst_offset < 0) { *why = "negative offset"; return AEJ_ERR_ARG; }
        bool known = false;
        for (const auto &c : kLtCombos) known = known || (d.channels_in == c[0] && d.table_channels == c[1] && d.channels_out == c[2]);
        if (!known) { *why = "(channels_in, table_channels, channels_out) other than (3, 3, 3), (4, 3, 3), (4, 3, 4), (3, 4, 4), (4, 4, 4)"; return AEJ_ERR_ARG; }
        for (int a = 0; a < 3; a++) {
            if (d.size[a] < 2 || d.size[a] > 65) { *why = "a table size outside [2, 65]"; return AEJ_ERR_ARG; }
            e.scale[a] = (unsigned)((d.size[a] - 1) / 255.0 * (1 << 18));
        }
        if (d.table < 0 || d.table >= n_tables || d.table >= n) { *why = "table index outside the call's tables (or not below the number of images)"; return AEJ_ERR_ARG; }
        e.s1 = d.size[0];
        e.s12 = d.size[0] * d.size[1];
        e.entries = e.s12 * d.size[2];
        e.npix = (long long)d.width * d.height;
        if (table_offsets && table_offsets[d.table + 1] - table_offsets[d.table] != (long long)e.entries * d.table_channels) {
            *why = "a table whose length is not s1 * s2 * s3 * table_channels";
            return AEJ_ERR_ARG;
        }
        if (plan.table_tc[d.table] && (plan.table_tc[d.table] != d.table_channels || table_entries[d.table] != e.entries)) {
            *why = "a table used with two sizes or channel counts";
            return AEJ_ERR_ARG;
        }
        plan.table_tc[d.table] = d.table_channels;
        table_entries[d.table] = e.entries;
        plan.spans.reads.push_back({ i, d.src_offset, e.npix * d.channels_in });
        plan.spans.writes.push_back({ i, d.dst_offset, e.npix * d.channels_out });
    }
    *bad = -1;
    // the padded upload: every table on a 256-byte boundary
    plan.table_at.assign(n_tables + 1, 0);
    for (int t = 0; t < n_tables; t++) plan.table_at[t + 1] = plan.table_at[t] + align_up(table_entries[t], 32);
    for (const auto &c : kLtCombos) {
        LtLaunch l = { c[0], c[1], c[2], (int)plan.entries.size(), 0, 0 };
        for (int i = 0; i < n; i++) {
            const aej_lut3d_desc &d = descs[i];
            if (d.channels_in != c[0] || d.table_channels != c[1] || d.channels_out != c[2]) continue;
            LtEntry e = image[i];
            e.tile_base = l.tiles;
            l.tiles += (e.npix + kLtTile - 1) / kLtTile;
            plan.entries.push_back(e);
            plan.image.push_back(i);
        }
        l.count = (int)plan.entries.size() - l.first;
        if (l.tiles > 0x7fffffffLL) { *why = "more than 2^31 workgroups in one launch"; return AEJ_ERR_UNSUPPORTED; }
        if (l.count) plan.launches.push_back(l);
    }
    return 0;
}

// the upload of a call: the entries of every launch with their device pointers, and the tables with every entry padded to four INT16
void lut3d_blob(const LtPlan &plan, const aej_lut3d_desc *descs, const short *tables_host, const long long *table_offsets, const unsigned char *src,
                unsigned char *dst, const uint2 *tables_dev, std::vector<LtEntry> &blob, std::vector<short> &padded)
{
    blob = plan.entries;
    for (size_t k = 0; k < blob.size(); k++) {
        const int i = plan.image[k];
        blob[k].in = src + plan.spans.reads[i].offset;
        blob[k].out = dst + plan.spans.writes[i].offset;
        blob[k].table = tables_dev + plan.table_at[descs[i].table];
    }
    padded.assign((size_t)plan.table_at.back() * 4, 0);
    for (size_t t = 0; t + 1 < plan.table_at.size(); t++) {
        const int tc = plan.table_tc[t];
        if (!tc) continue;
        const short *from = tables_host + table_offsets[t];
        short *to = padded.data() + plan.table_at[t] * 4;
        const long long entries = (table_offsets[t + 1] - table_offsets[t]) / tc;
        for (long long k = 0; k < entries; k++)
            for (int c = 0; c < tc; c++) to[4 * k + c] = from[tc * k + c];
    }
}

template <int kCI, int kTC, int kCO>
static void lt_launch(hipStream_t st, const LtLaunch &l, const LtEntry *entries)
{
    const dim3 grid((unsigned)l.tiles), block(kLtThreads);
    hipLaunchKernelGGL((k_lut3d<kCI, kTC, kCO>), grid, block, 0, st, entries, l.count);
}

hipError_t launch_lut3d(hipStream_t st, const LtPlan &plan, unsigned char *blob_dev, const LtEntry *blob_host, uint2 *tables_dev, const short *padded)
{
    hipError_t e = hipMemcpyAsync(blob_dev, blob_host, plan.entries.size() * sizeof(LtEntry), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return e;
    e = hipMemcpyAsync(tables_dev, padded, (size_t)plan.table_at.back() * 8, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return e;
    for (const LtLaunch &l : plan.launches) {
        const LtEntry *entries = (const LtEntry *)blob_dev + l.first;
        if (l.ci == 3 && l.tc == 3) lt_launch<3, 3, 3>(st, l, entries);
        if (l.ci == 4 && l.tc == 3 && l.co == 3) lt_launch<4, 3, 3>(st, l, entries);
        if (l.ci == 4 && l.tc == 3 && l.co == 4) lt_launch<4, 3, 4>(st, l, entries);
        if (l.ci == 3 && l.tc == 4) lt_launch<3, 4, 4>(st, l, entries);
        if (l.ci == 4 && l.tc == 4) lt_launch<4, 4, 4>(st, l, entries);
    }
    return hipGetLastError();
}

}  // namespace aej
