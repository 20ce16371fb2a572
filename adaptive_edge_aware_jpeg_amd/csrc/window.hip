// window.hip -- Pillow's Kernel (the ten built-ins among them), rank and mode filters on the device (aej_window_*), bit for bit, over
// many packed 8-bit images of 1 to 4 channels, of different sizes and filters, in one call.  include/aej.h has the arithmetic.  Three
// families with three border rules: a Kernel copies the samples within r of an edge, a rank window is clamped to the image, a mode
// window is clipped to it.
//
// One workgroup = one 64 x 32 output tile.  wn_stage puts the tile and its halo of r pixels into LDS as bytes, once, with positions
// outside the image replaced by the nearest image sample (the rank rule; the other two kernels never use such a position), so that
// the window loops have no bounds to test.  Then a lane produces 4 adjacent bytes of a tile row at a time:
//   k_window_conv<C, K>   the K x K float32 convolution in exactly Pillow's order; every LDS offset is a compile-time constant
//   k_window_rank<C>      the rank-th smallest of the window by 8-step radix selection: from the top bit down, keep the bit when the
//                         number of window samples below the candidate is <= rank.  One path for every size and rank.
//   k_window_mode<C>      for every in-image window sample its count of equals; the highest count wins, the smaller value on a tie
// A launch is one grid over every image that needs it (a per-image entry, a prefix sum of workgroups, a binary search by blockIdx.x,
// as filter.hip's).  Bounds: only the part of the region that the tile's in-image outputs need is staged and only lanes with an
// in-image output compute, so no global read leaves the image and no LDS read leaves the buffer.
#include <math.h>
#include <string.h>

#include <vector>

#include "aej_ctx.h"

#pragma clang fp contract(off)

namespace aej {

// nb (1 .. 4) bytes at any address, as the low bytes of a word; the address of a row of a packed image has no alignment
__device__ __forceinline__ unsigned wn_load4(const unsigned char *p, int nb)
{
    unsigned v = 0;
    if (nb == 4) {
        __builtin_memcpy(&v, p, 4);
    } else {
        for (int b = 0; b < nb; b++) v |= (unsigned)p[b] << (8 * b);
    }
    return v;
}

__device__ __forceinline__ void wn_store4(unsigned char *p, int nb, unsigned v)
{
    if (nb == 4) {
        __builtin_memcpy(p, &v, 4);
    } else {
        for (int b = 0; b < nb; b++) p[b] = (unsigned char)(v >> (8 * b));
    }
}

// LDS: (th + 2 r) rows of `pitch` bytes; a row is `pad` bytes, which put the tile's first byte on a dword, then the (tw + 2 r) pixels
// of the region.  Region position (ly, lx) holds the image at (clamp(Y0 - r + ly), clamp(X0 - r + lx)).
__host__ __device__ inline int wn_pad(int r, int ch) { return (4 - (r * ch) % 4) % 4; }
__host__ __device__ inline int wn_pitch(int r, int ch) { return (wn_pad(r, ch) + (kWnTileW + 2 * r) * ch + 3) & ~3; }
static unsigned wn_lds(int r, int ch) { return (unsigned)((kWnTileH + 2 * r) * wn_pitch(r, ch)); }

struct WnTile { int X0, Y0, tw, th; };

__device__ __forceinline__ WnTile wn_tile(const WnEntry &e)
{
    const int tiles_x = (e.w + kWnTileW - 1) / kWnTileW, local = (int)((long long)blockIdx.x - e.tile_base);
    WnTile t;
    t.X0 = (local % tiles_x) * kWnTileW;
    t.Y0 = (local / tiles_x) * kWnTileH;
    t.tw = min(kWnTileW, e.w - t.X0);
    t.th = min(kWnTileH, e.h - t.Y0);
    return t;
}

template <int kC>
__device__ __forceinline__ void wn_stage(const WnEntry &e, const WnTile &t, int r, unsigned char *lds, int pad, int pitch)
{
    const int rows = t.th + 2 * r;
    const int gx_lo = max(t.X0 - r, 0), gx_hi = min(t.X0 + t.tw + r - 1, e.w - 1);      // the region's columns inside the image
    {   // a lane loads 4 bytes of a row
        const int nb_row = (gx_hi - gx_lo + 1) * kC, ndw = (nb_row + 3) >> 2;
        for (int it = threadIdx.x; it < rows * ndw; it += kWnThreads) {
            const int row = it / ndw, d = it - row * ndw, nb = min(4, nb_row - 4 * d);
            const int gy = min(max(t.Y0 - r + row, 0), e.h - 1);
            const unsigned v = wn_load4(e.in + ((long long)gy * e.w + gx_lo) * kC + 4 * d, nb);
            unsigned char *s = lds + row * pitch + pad + (gx_lo - (t.X0 - r)) * kC + 4 * d;
            for (int b = 0; b < nb; b++) s[b] = (unsigned char)(v >> (8 * b));
        }
    }
    const int nl = max(0, r - t.X0), nr = max(0, t.X0 + t.tw + r - e.w);      // region columns left and right of the image: each <= r
    for (int it = threadIdx.x; it < rows * (nl + nr) * kC; it += kWnThreads) {
        const int c = it % kC, q = it / kC, col = q % (nl + nr), row = q / (nl + nr);
        const int gy = min(max(t.Y0 - r + row, 0), e.h - 1);
        const int lx = col < nl ? col : t.tw + 2 * r - nr + (col - nl), gx = col < nl ? 0 : e.w - 1;
        lds[row * pitch + pad + lx * kC + c] = e.in[((long long)gy * e.w + gx) * kC + c];
    }
    __syncthreads();
}

// ---- Kernel ------------------------------------------------------------------------------------------------------------------------
// A lane's 4 output bytes are one dword of the tile row; their windows lie in the 2 M + 1 dwords around it on each of K region rows
// (M = dwords that cover r pixels).  Bytes of those dwords beyond the staged region only reach output bytes that are not stored.
template <int kC, int kK>
__global__ __launch_bounds__(kWnThreads) void k_window_conv(const WnEntry *__restrict__ entries, int n)
{
    extern __shared__ __align__(16) unsigned char wn_lds_buf[];
    const WnEntry &e = tile_entry(entries, n);
    constexpr int r = kK / 2, M = (r * kC + 3) / 4, ND = 2 * M + 1;
    constexpr int pad = (4 - (r * kC) % 4) % 4, pitch = (pad + (kWnTileW + 2 * r) * kC + 3) & ~3, tile_off = pad + r * kC;
    const WnTile t = wn_tile(e);
    wn_stage<kC>(e, t, r, wn_lds_buf, pad, pitch);
    float qk[kK * kK];
#pragma unroll
    for (int i = 0; i < kK * kK; i++) qk[i] = e.q[i];
    const float ss0 = e.ss0;
    const int nb_row = t.tw * kC, ndw = (nb_row + 3) >> 2;
    for (int it = threadIdx.x; it < t.th * ndw; it += kWnThreads) {
        const int row = it / ndw, d = it - row * ndw;
        const unsigned char *base = wn_lds_buf + (r + row) * pitch + tile_off + 4 * d;
        float ss[4] = { ss0, ss0, ss0, ss0 };
        unsigned centre = 0;
#pragma unroll
        for (int j = 0; j < kK; j++) {                // kernel row j meets image row y + r - j
            unsigned wv[ND];
#pragma unroll
            for (int m = 0; m < ND; m++) wv[m] = *(const unsigned *)(base + (r - j) * pitch + 4 * (m - M));
            if (j == r) centre = wv[M];
#pragma unroll
            for (int b = 0; b < 4; b++) {
                float rs = 0.f;
#pragma unroll
                for (int i = 0; i < kK; i++) {
                    constexpr int zero = 4 * M;
                    const int at = zero + b + (i - r) * kC;
                    const float p = (float)((wv[at >> 2] >> (8 * (at & 3))) & 255u);
                    const float term = qk[j * kK + i] * p;
                    rs = i == 0 ? term : rs + term;
                }
                ss[b] = ss[b] + rs;
            }
        }
        const int y = t.Y0 + row;
        const bool edge_y = y < r || y >= e.h - r;
        unsigned v = 0;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int x = t.X0 + (4 * d + b) / kC;
            const unsigned keep = (centre >> (8 * b)) & 255u;
            const float s = ss[b];
            const unsigned conv = s <= 0.f ? 0u : s >= 255.f ? 255u : (unsigned)s;
            v |= ((edge_y || x < r || x >= e.w - r) ? keep : conv) << (8 * b);
        }
        wn_store4(e.out + ((long long)y * e.w + t.X0) * kC + 4 * d, min(4, nb_row - 4 * d), v);
    }
}

// ---- rank ----------------------------------------------------------------------------------------------------------------------------
template <int kC>
__global__ __launch_bounds__(kWnThreads) void k_window_rank(const WnEntry *__restrict__ entries, int n)
{
    extern __shared__ __align__(16) unsigned char wn_lds_buf[];
    const WnEntry &e = tile_entry(entries, n);
    const int r = e.r, rank = e.rank, pad = wn_pad(r, kC), pitch = wn_pitch(r, kC);
    const WnTile t = wn_tile(e);
    wn_stage<kC>(e, t, r, wn_lds_buf, pad, pitch);
    const int nb_row = t.tw * kC, ndw = (nb_row + 3) >> 2;
    for (int it = threadIdx.x; it < t.th * ndw; it += kWnThreads) {
        const int row = it / ndw, d = it - row * ndw, nb = min(4, nb_row - 4 * d);
        const unsigned char *corner = wn_lds_buf + row * pitch + pad + 4 * d;      // the window's first sample of byte 0
        unsigned v = 0;
        for (int b = 0; b < nb; b++) {
            unsigned res = 0;
            for (int bit = 7; bit >= 0; bit--) {
                const unsigned cand = res | (1u << bit);
                int below = 0;
                for (int dy = 0; dy <= 2 * r; dy++) {
                    const unsigned char *line = corner + dy * pitch + b;
                    for (int dx = 0; dx <= 2 * r; dx++) below += line[dx * kC] < cand;
                }
                if (below <= rank) res = cand;
            }
            v |= res << (8 * b);
        }
        wn_store4(e.out + ((long long)(t.Y0 + row) * e.w + t.X0) * kC + 4 * d, nb, v);
    }
}

// ---- mode ----------------------------------------------------------------------------------------------------------------------------
template <int kC>
__global__ __launch_bounds__(kWnThreads) void k_window_mode(const WnEntry *__restrict__ entries, int n)
{
    extern __shared__ __align__(16) unsigned char wn_lds_buf[];
    const WnEntry &e = tile_entry(entries, n);
    const int r = e.r, pad = wn_pad(r, kC), pitch = wn_pitch(r, kC);
    const WnTile t = wn_tile(e);
    wn_stage<kC>(e, t, r, wn_lds_buf, pad, pitch);
    const int nb_row = t.tw * kC, ndw = (nb_row + 3) >> 2;
    for (int it = threadIdx.x; it < t.th * ndw; it += kWnThreads) {
        const int row = it / ndw, d = it - row * ndw, nb = min(4, nb_row - 4 * d);
        const int y = t.Y0 + row, dy0 = max(-r, -y), dy1 = min(r, e.h - 1 - y);      // the window's rows inside the image
        unsigned v = 0;
        for (int b = 0; b < nb; b++) {
            const int x = t.X0 + (4 * d + b) / kC, dx0 = max(-r, -x), dx1 = min(r, e.w - 1 - x);
            const unsigned char *at = wn_lds_buf + (r + row) * pitch + pad + r * kC + 4 * d + b;
            unsigned best = *at;
            int most = 0;
            for (int iy = dy0; iy <= dy1; iy++)
                for (int ix = dx0; ix <= dx1; ix++) {
                    const unsigned s = at[iy * pitch + ix * kC];
                    int count = 0;
                    for (int jy = dy0; jy <= dy1; jy++) {
                        const unsigned char *line = at + jy * pitch;
                        for (int jx = dx0; jx <= dx1; jx++) count += line[jx * kC] == s;
                    }
                    if (count > most || (count == most && s < best)) { most = count; best = s; }
                }
            v |= (most > 2 ? best : (unsigned)*at) << (8 * b);
        }
        wn_store4(e.out + ((long long)y * e.w + t.X0) * kC + 4 * d, nb, v);
    }
}

// ---- host: the plan of a call -------------------------------------------------------------------------------------------------------------------
// -> 0, or the error code with *bad the image and *why the reason.  The quotients kernel[i] / scale and offset + 0.5f are taken here, once.
int window_plan(const aej_window_desc *descs, int n, WnPlan &plan, int *bad, const char **why)
{
    const float cap = ldexpf(1.f, 100);
    std::vector<WnEntry> image(n);
    plan = WnPlan();
    for (int i = 0; i < n; i++) {
        const aej_window_desc &d = descs[i];
        WnEntry &e = image[i];
        memset(&e, 0, sizeof e);
        *bad = i;
        if (d.width < 1 || d.height < 1 || d.width > 65535 || d.height > 65535) { *why = "sizes from 1 to 65535 a side"; return AEJ_ERR_ARG; }
        if (d.channels < 1 || d.channels > 4) { *why = "1 to 4 channels"; return AEJ_ERR_ARG; }
        if (d.src_offset < 0 || d.dst_offset < 0) { *why = "negative offset"; return AEJ_ERR_ARG; }
        e.w = d.width; e.h = d.height;
        if (d.kind == AEJ_WINDOW_KERNEL) {
            if (d.size != 3 && d.size != 5) { *why = "a kernel of 3 x 3 or 5 x 5"; return AEJ_ERR_ARG; }
            if (!isfinite(d.scale) || !isfinite(d.offset)) { *why = "scale or offset not finite"; return AEJ_ERR_ARG; }
            if (d.scale == 0) { *why = "a scale of 0"; return AEJ_ERR_ARG; }
            bool large = fabsf(d.offset) > cap;
            for (int k = 0; k < d.size * d.size; k++) {
                const float q = d.kernel[k] / d.scale;
                if (!isfinite(d.kernel[k]) || !isfinite(q)) { *why = "a kernel value or its quotient by the scale not finite"; return AEJ_ERR_ARG; }
                large = large || fabsf(q) > cap;
                e.q[k] = q;
            }
            if (large) { *why = "|kernel / scale| or |offset| above 2^100"; return AEJ_ERR_UNSUPPORTED; }
            e.ss0 = d.offset + 0.5f;
            e.r = d.size / 2;
        } else if (d.kind == AEJ_WINDOW_RANK) {
            if (d.size < 1 || d.size % 2 == 0) { *why = "an odd rank size from 1 on"; return AEJ_ERR_ARG; }
            if (d.size > 2 * kWnRankHalo + 1) { *why = "rank size above 15"; return AEJ_ERR_UNSUPPORTED; }
            if (d.rank < 0 || d.rank >= d.size * d.size) { *why = "rank outside [0, size * size)"; return AEJ_ERR_ARG; }
            e.r = d.size / 2;
            e.rank = d.rank;
        } else if (d.kind == AEJ_WINDOW_MODE) {
            if (d.size < 1) { *why = "a mode size from 1 on"; return AEJ_ERR_ARG; }
            if (d.size > 2 * kWnModeHalo + 1) { *why = "mode size above 7"; return AEJ_ERR_UNSUPPORTED; }
            e.r = d.size / 2;
        } else {
            *why = "unknown filter kind";
            return AEJ_ERR_ARG;
        }
        const long long bytes = (long long)d.width * d.height * d.channels;
        plan.spans.reads.push_back({ i, d.src_offset, bytes });
        plan.spans.writes.push_back({ i, d.dst_offset, bytes });
    }
    *bad = -1;
    static const int kinds[4][2] = { { AEJ_WINDOW_KERNEL, 3 }, { AEJ_WINDOW_KERNEL, 5 }, { AEJ_WINDOW_RANK, 0 }, { AEJ_WINDOW_MODE, 0 } };
    for (const auto &k : kinds)
        for (int ch = 1; ch <= 4; ch++) {
            WnLaunch l = { k[0], ch, k[1], (int)plan.entries.size(), 0, 0, 0 };
            for (int i = 0; i < n; i++) {
                if (descs[i].kind != k[0] || descs[i].channels != ch || (k[1] && descs[i].size != k[1])) continue;
                WnEntry e = image[i];
                e.tile_base = l.tiles;
                l.tiles += (long long)((e.w + kWnTileW - 1) / kWnTileW) * ((e.h + kWnTileH - 1) / kWnTileH);
                l.lds = std::max(l.lds, wn_lds(e.r, ch));
                plan.entries.push_back(e);
                plan.image.push_back(i);
            }
            l.count = (int)plan.entries.size() - l.first;
            if (l.tiles > 0x7fffffffLL) { *why = "more than 2^31 workgroups in one launch"; return AEJ_ERR_UNSUPPORTED; }
            if (l.count) plan.launches.push_back(l);
        }
    return 0;
}

// the upload of a call: the entries of every launch with their device pointers
void window_blob(const WnPlan &plan, const unsigned char *src, unsigned char *dst, std::vector<WnEntry> &blob)
{
    blob = plan.entries;
    for (size_t k = 0; k < blob.size(); k++) {
        blob[k].in = src + plan.spans.reads[plan.image[k]].offset;
        blob[k].out = dst + plan.spans.writes[plan.image[k]].offset;
    }
}

template <int kC>
static void wn_launch(hipStream_t st, const WnLaunch &l, const WnEntry *entries)
{
    const dim3 grid((unsigned)l.tiles), block(kWnThreads);
    if (l.kind == AEJ_WINDOW_KERNEL && l.size == 3) hipLaunchKernelGGL((k_window_conv<kC, 3>), grid, block, l.lds, st, entries, l.count);
    if (l.kind == AEJ_WINDOW_KERNEL && l.size == 5) hipLaunchKernelGGL((k_window_conv<kC, 5>), grid, block, l.lds, st, entries, l.count);
    if (l.kind == AEJ_WINDOW_RANK) hipLaunchKernelGGL(k_window_rank<kC>, grid, block, l.lds, st, entries, l.count);
    if (l.kind == AEJ_WINDOW_MODE) hipLaunchKernelGGL(k_window_mode<kC>, grid, block, l.lds, st, entries, l.count);
}

hipError_t launch_window(hipStream_t st, const WnPlan &plan, unsigned char *blob_dev, const WnEntry *blob_host)
{
    hipError_t e = hipMemcpyAsync(blob_dev, blob_host, plan.entries.size() * sizeof(WnEntry), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return e;
    for (const WnLaunch &l : plan.launches) {
        const WnEntry *entries = (const WnEntry *)blob_dev + l.first;
        if (l.ch == 1) wn_launch<1>(st, l, entries);
        if (l.ch == 2) wn_launch<2>(st, l, entries);
        if (l.ch == 3) wn_launch<3>(st, l, entries);
        if (l.ch == 4) wn_launch<4>(st, l, entries);
    }
    return hipGetLastError();
}

}  // namespace aej
