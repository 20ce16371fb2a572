// png.hip -- the PNG half of png_decode_many after the inflate: the scanline un-filter (PNG specification, section 9) and the expansion of
// grey, palette and alpha layouts to the image the caller asked for; and, further down, the scanline filter of png_encode_many.
//
// One workgroup per work item -- a non-interlaced file, or one non-empty Adam7 pass of an interlaced one, which is an un-filter problem of
// its own (h_p rows of row_bytes_p bytes at its own place in the file's inflated span): all passes of all files of a launch run at once,
// seven workgroups a file -- and in it one wave64 that un-filters.  Un-filtering is a recurrence -- Sub, Average and Paeth need the byte
// `bpp` to the left, Up, Average and Paeth the row above, Paeth the byte above-left as well -- so the rows of a file are not independent,
// but its anti-diagonals are.  The wave walks bands of 64 rows: lane k owns row r0 + k and runs one unit (bpp bytes: a pixel of 1 .. 8 bytes, or one byte
// of a packed depth) behind lane k - 1.  At step g lane k un-filters unit x = g - k; "up" is what lane k - 1 produced one step earlier and
// arrives by one cross-lane move of a packed dword (two for the units of 6 and 8 bytes: 16-bit RGB and RGBA), "up-left" is the "up" of the lane's own previous step and "left" its previous
// result: both stay in registers.  Lane 0's "up" is the last row of the band before, which that band left in the file's carry row in the
// workspace.  The other waves of the workgroup (kWaves in all) only move data: they share the rows of the stage-in before the walk of a
// tile and of the stage-out after it (profiles/png_decode_kernel_times.txt: 214 -> 97 ms for 64 files of 4K against the walking wave
// doing it all).
//
// Global memory is never touched one unit per lane.  A band is cut into tiles of kTile bytes per row, skewed like the walk (row k's tile
// starts k units to the left of row 0's), so that every lane has a unit in every step of a tile.  A tile is staged into LDS with
// whole-wave loads (rows are 1 + row_bytes apart, so by aligned dwords and a funnel shift), un-filtered in place, and leaves through the
// expansion -- sub-byte unpack and scale, palette lookup from an LDS copy of PLTE, alpha kept or dropped -- in whole-wave dword stores.
//
// Nothing in a file can fault or hang the kernel: every loop is bounded by the descriptor's height and row bytes, every load address is
// clamped into the item's span of the inflated buffer, which lies inside its file's (whose size the caller's inflate has vouched for: a
// file with another status or size is not read at all), every store lies inside the item's image, and a filter byte above 4 ends the
// item with a status.
//
// A pass's image goes to the workspace as a small packed image (w_p x h_p x oc, after the expansion) and its status to a word of its
// own there, so the seven walks of an interlaced file run in different workgroups at once and none of them scatters pixels.
// png_adam7_interleave_kernel (behind the un-filter kernel) then writes every row of the image in whole dwords: a wave stages the
// stretch of each pass row that the output row draws from into LDS with whole-wave dword loads and picks every pixel's pass from
// (x & 7, y & 7); an odd row is the seventh pass alone.  It also folds the passes' status words into the file's (the largest wins) and
// leaves the image alone unless all are ok.
#include "aej_launch.h"

namespace aej {

namespace {

constexpr int kRows = 64;                    // rows per band: one per lane of the walking wave
constexpr int kWaves = 8;                    // waves per workgroup: wave 0 walks, all of them stage
constexpr int kTile = 256;                   // bytes per tile row (252 for bpp 3 and 6: a whole number of units and of dwords)
constexpr int kPitch = kTile / 4 + 1;        // dwords between tile rows in LDS: odd, so the lanes' rows fall on different banks
constexpr int kUpRow = kRows;                // the tile row that holds lane 0's "up"

enum { kOk = 0, kInflateFailed = 1, kSizeMismatch = 2, kBadFilter = 3 };      // include/aej.h AEJ_PNG_*

// bytes of a file's carry row: its scanline as the band's last lane holds it in the tiles (kRows - 1 units to the right), in whole tiles,
// and the dwords the next band's lane 0 reads past them
__host__ __device__ constexpr int tile_bytes_of(int bpp) { return bpp == 3 || bpp == 6 ? 252 : kTile; }

__host__ __device__ inline long long carry_bytes_of(int rb, int bpp)
{
    const int tb = tile_bytes_of(bpp), p = tb / bpp;
    const long long ntile = (rb / bpp + kRows - 1 + p - 1) / p;
    return (ntile * tb + (kRows - 1) * bpp + 8 + 255) & ~255LL;
}

struct PngLds {
    unsigned tile[(kRows + 1) * kPitch];
    unsigned pal[192];                       // PLTE: 256 x RGB, zero past its end
};

// the dword at byte `at` of `base` (4-byte aligned), read as two aligned dwords; bytes outside [lo, hi) -- both multiples of 4 with
// hi - lo >= 4 -- read as whatever the clamped address holds: the caller uses none of them
__device__ inline unsigned load_dword_at(const unsigned char *base, long long at, long long lo, long long hi)
{
    const long long a = at & ~3LL;
    const int sh = (int)(at & 3) * 8;
    const long long a0 = min(max(a, lo), hi - 4), a1 = min(max(a + 4, lo), hi - 4);
    const unsigned v0 = *reinterpret_cast<const unsigned *>(base + a0);
    const unsigned v1 = *reinterpret_cast<const unsigned *>(base + a1);
    return sh ? (v0 >> sh) | (v1 << (32 - sh)) : v0;
}

// a unit in registers: one dword up to 4 bytes, two above
template <int BPP> struct Unit { using type = unsigned; };
template <> struct Unit<6> { using type = unsigned long long; };
template <> struct Unit<8> { using type = unsigned long long; };

template <int BPP> __device__ inline typename Unit<BPP>::type read_unit(const unsigned char *p)
{
    if (BPP == 8) return *reinterpret_cast<const unsigned *>(p) | (unsigned long long)*reinterpret_cast<const unsigned *>(p + 4) << 32;
    if (BPP == 6) {                                  // (a unit of 6 bytes starts at an even byte of its tile row)
        const unsigned short *q = reinterpret_cast<const unsigned short *>(p);
        return q[0] | (unsigned)q[1] << 16 | (unsigned long long)q[2] << 32;
    }
    if (BPP == 4) return *reinterpret_cast<const unsigned *>(p);
    if (BPP == 2) return *reinterpret_cast<const unsigned short *>(p);
    unsigned v = p[0];
    if (BPP == 3) v |= (unsigned)p[1] << 8 | (unsigned)p[2] << 16;
    return v;
}

template <int BPP> __device__ inline void write_unit(unsigned char *p, typename Unit<BPP>::type v)
{
    if (BPP == 8) {
        reinterpret_cast<unsigned *>(p)[0] = (unsigned)v;
        reinterpret_cast<unsigned *>(p)[1] = (unsigned)((unsigned long long)v >> 32);
        return;
    }
    if (BPP == 6) {
        unsigned short *q = reinterpret_cast<unsigned short *>(p);
        q[0] = (unsigned short)v;
        q[1] = (unsigned short)(v >> 16);
        q[2] = (unsigned short)((unsigned long long)v >> 32);
        return;
    }
    if (BPP == 4) { *reinterpret_cast<unsigned *>(p) = v; return; }
    if (BPP == 2) { *reinterpret_cast<unsigned short *>(p) = (unsigned short)v; return; }
    p[0] = (unsigned char)v;
    if (BPP == 3) { p[1] = (unsigned char)(v >> 8); p[2] = (unsigned char)(v >> 16); }
}

// one byte of the specification's reconstruction: filter type ft, filtered byte x, a = left, b = up, c = up-left
__device__ inline unsigned recon_byte(int ft, unsigned x, int a, int b, int c)
{
    const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
    const int paeth = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);      // ties in the order a, b, c
    const int pred = ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) >> 1 : ft == 4 ? paeth : 0;
    return (x + (unsigned)pred) & 255u;
}

// one image byte: channel ch of pixel px of the tile row `row` (LDS bytes), whose byte 0 is byte `first` of the scanline
template <bool DEEP>
__device__ inline unsigned sample(const PngFile &f, const unsigned char *row, const unsigned char *pal, int first, int px, int ch)
{
    unsigned raw;
    if (DEEP) {
        // big-endian samples.  Pillow keeps the high byte of every sample but a grey file's: that one is mode "I;16", whose pixels are the
        // whole samples (oc == 2: in host order) and whose convert("RGB") CLIPS them to 255; grey + alpha opens as RGBA
        const int sc = f.ct == 2 || f.ct == 6 ? ch : f.ct == 4 && ch == 3 ? 1 : 0;
        const unsigned char *s = row + (px * f.bpp + 2 * sc - first);
        const unsigned hi = s[0], lo = s[1];
        if (f.ct == 0) return f.oc == 2 ? (ch ? hi : lo) : (hi ? 255u : lo);
        return hi;
    }
    if (f.depth == 8) {
        const bool own = f.ct == 2 || f.ct == 6 || (f.ct == 4 && f.oc == 2);      // the channel's own sample; else sample 0 (grey, index)
        raw = row[px * f.bpp + (own ? ch : 0) - first];
    } else {
        const int bit = px * f.depth;
        raw = (row[(bit >> 3) - first] >> (8 - f.depth - (bit & 7))) & ((1u << f.depth) - 1u);
        if (f.ct == 0) raw *= f.depth == 1 ? 255u : f.depth == 2 ? 85u : 17u;
    }
    return f.ct == 3 ? pal[raw * 3 + ch] : raw;
}

template <int BPP, bool DEEP>
__device__ int unfilter_file(PngLds &L, const PngFile &f, const unsigned char *inflated, unsigned char *out, unsigned char *carry)
{
    constexpr int TB = tile_bytes_of(BPP);           // bytes per tile row
    using unit_t = typename Unit<BPP>::type;
    constexpr int P = TB / BPP;                      // units per tile row = steps per tile
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long stride = 1 + (long long)f.rb;
    const long long lo = f.in_off & ~3LL, hi = (f.in_off + (long long)f.H * stride + 3) & ~3LL;      // whole dwords, inside the file's
    const int U = f.rb / BPP;                        // units per row
    const int ntile = (U + kRows - 1 + P - 1) / P;   // the last lane's last unit is step U + 62
    const long long carry_bytes = carry_bytes_of(f.rb, BPP);
    unsigned char *tile8 = reinterpret_cast<unsigned char *>(L.tile);
    const unsigned char *pal8 = reinterpret_cast<const unsigned char *>(L.pal);
    unsigned char *mine = tile8 + lane * (kPitch * 4);
    const unsigned char *up0 = tile8 + kUpRow * (kPitch * 4);
    unsigned char *cr = carry + f.carry_off;

    for (int r0 = 0; r0 < f.H; r0 += kRows) {
        const int row = r0 + lane;
        const bool rowv = row < f.H;
        const int nrows = min(kRows, f.H - r0);
        const int ft = rowv ? inflated[f.in_off + row * stride] : 0;
        if (__ballot(ft > 4) != 0ull) return kBadFilter;       // every wave looks at the same 64 bytes: the whole workgroup leaves
        unit_t left = 0, upleft = 0, res = 0;
        for (int t = 0; t < ntile; t++) {
            // ---- stage in: TB bytes of every row of the band, row k from its unit t P - k on (eight rows in flight per wave), and lane 0's
            // "up" from the carry row
            if (lane < TB / 4) {
                for (int k0 = 8 * wave; k0 < nrows; k0 += 8 * kWaves) {
                    unsigned v[8];
#pragma unroll
                    for (int j = 0; j < 8; j++) {
                        const int k = min(k0 + j, nrows - 1);
                        const long long b0 = (long long)(t * P - k) * BPP + 4 * lane;      // the dword's first byte in the scanline
                        v[j] = load_dword_at(inflated, f.in_off + (r0 + k) * stride + 1 + b0, lo, hi);
                    }
#pragma unroll
                    for (int j = 0; j < 8; j++)
                        if (k0 + j < nrows) L.tile[(k0 + j) * kPitch + lane] = v[j];
                }
                if (wave == kWaves - 1)
                    L.tile[kUpRow * kPitch + lane] =
                        r0 > 0 ? load_dword_at(cr, (long long)t * TB + (kRows - 1) * BPP + 4 * lane, 0, carry_bytes) : 0u;
            }
            __syncthreads();
            // ---- the walk: step s of the tile is unit x = t P + s - lane of the lane's row
            const int steps = min(P, U + kRows - 1 - t * P);
            for (int s = 0; wave == 0 && s < steps; s++) {
                const int x = t * P + s - lane;
                unit_t up = __shfl_up(res, 1);
                if (lane == 0) up = read_unit<BPP>(up0 + s * BPP);
                if (rowv && x >= 0 && x < U) {
                    const unit_t raw = read_unit<BPP>(mine + s * BPP);
                    const unit_t a = x ? left : 0u, c = x ? upleft : 0u;
                    unit_t r = 0;
#pragma unroll
                    for (int i = 0; i < BPP; i++)
                        r |= (unit_t)recon_byte(ft, (unsigned)(raw >> (8 * i)) & 255u, (int)((a >> (8 * i)) & 255), (int)((up >> (8 * i)) & 255),
                                                (int)((c >> (8 * i)) & 255)) << (8 * i);
                    write_unit<BPP>(mine + s * BPP, r);
                    left = res = r;
                }
                upleft = up;
            }
            __syncthreads();
            // ---- stage out: the band's last row to the carry row (skewed as it lies in the tile), every row's units to the image
            if (r0 + kRows < f.H && wave == kWaves - 1 && lane < TB / 4)
                reinterpret_cast<unsigned *>(cr)[(long long)t * (TB / 4) + lane] = L.tile[(kRows - 1) * kPitch + lane];
            for (int k = wave; k < nrows; k += kWaves) {
                const int u0 = max(t * P - k, 0), u1 = min((t + 1) * P - k, U);
                if (u0 >= u1) continue;
                const int ppu = DEEP || f.depth == 8 ? 1 : 8 / f.depth;          // pixels per unit
                const int p0 = u0 * ppu, p1 = min(u1 * ppu, f.W);
                const long long rowo = f.out_off + (long long)(r0 + k) * f.W * f.oc;
                const long long o0 = rowo + (long long)p0 * f.oc, o1 = rowo + (long long)p1 * f.oc;
                const long long d0 = o0 - (long long)(reinterpret_cast<uintptr_t>(out + o0) & 3);      // whole dwords of `out`
                const unsigned char *src = tile8 + k * (kPitch * 4);
                const int first = (t * P - k) * BPP;
                for (long long d = d0 + 4 * lane; d < o1; d += 4 * 64) {
                    const int rel = (int)(max(d, o0) - rowo);
                    int px = rel / f.oc, ch = rel - px * f.oc;
                    unsigned word = 0;
                    const bool whole = d >= o0 && d + 4 <= o1;
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        if (d + e < o0 || d + e >= o1) continue;
                        const unsigned v = sample<DEEP>(f, src, pal8, first, px, ch);
                        if (++ch == f.oc) { ch = 0; px++; }
                        if (whole) word |= v << (8 * e);
                        else out[d + e] = (unsigned char)v;
                    }
                    if (whole) *reinterpret_cast<unsigned *>(out + d) = word;
                }
            }
            __syncthreads();
        }
    }
    return kOk;
}

// DEEP: the files of bit depth 16 (units of 2, 4, 6 and 8 bytes) have a kernel of their own, so that the kernel every other file runs
// holds the four instantiations it always held.  blockIdx.x is the file of the group; of an interlaced file blockIdx.y is the pass,
// whose place in the file's inflated span, in its pass images and among its carry rows follows from the passes before it.
template <bool DEEP>
__global__ __launch_bounds__(kWaves * 64) void png_unfilter_kernel(PngGroup grp, int first, int count, const unsigned char *__restrict__ inflated,
                                                          const long long *__restrict__ inflate_out_bytes, const int *__restrict__ inflate_status,
                                                          const unsigned char *__restrict__ palettes, unsigned char *out, unsigned char *workspace,
                                                          int *__restrict__ status)
{
    __shared__ PngLds L;
    if ((int)blockIdx.x >= count) return;
    PngFile f = grp.f[blockIdx.x];
    if ((f.depth == 16) != DEEP) return;
    const int index = first + blockIdx.x;
    int item = -1;
    if (f.item >= 0) {
        const int pass = (int)blockIdx.y, W = f.W, H = f.H, bits = f.depth >= 8 ? 8 * f.bpp : f.depth;
        for (int q = 0;; q++) {
            const Adam7Pass a = adam7_pass(W, H, q);
            const int rb = (int)(((long long)a.w * bits + 7) >> 3);
            if (q == pass) {
                if (a.w == 0) return;                    // an empty pass has no bytes in the file, no image and no status
                f.W = a.w;
                f.H = a.h;
                f.rb = rb;
                break;
            }
            if (a.w > 0) {
                f.in_off += (long long)a.h * (1 + (long long)rb);
                f.carry_off += carry_bytes_of(rb, f.bpp);
            }
            f.out_off += ((long long)a.w * a.h * f.oc + 3) & ~3LL;
        }
        item = f.item + pass;
    } else if (blockIdx.y != 0) return;
    int st = kOk;
    // a file the inflate did not vouch for is not read at all
    if (inflate_status && inflate_status[index] != 0) st = kInflateFailed;
    else if (inflate_out_bytes && inflate_out_bytes[index] != f.raw_bytes) st = kSizeMismatch;
    if (st == kOk) {
        for (int i = threadIdx.x; i < 192; i += kWaves * 64)
            L.pal[i] = f.ct == 3 ? reinterpret_cast<const unsigned *>(palettes + 768LL * index)[i] : 0u;
        __syncthreads();
        unsigned char *dst = item >= 0 ? workspace : out;        // a pass's image lies in the workspace
        if (DEEP)
            st = f.bpp == 2 ? unfilter_file<2, true>(L, f, inflated, dst, workspace) : f.bpp == 4 ? unfilter_file<4, true>(L, f, inflated, dst, workspace)
               : f.bpp == 6 ? unfilter_file<6, true>(L, f, inflated, dst, workspace) : unfilter_file<8, true>(L, f, inflated, dst, workspace);
        else
            st = f.bpp == 1 ? unfilter_file<1, false>(L, f, inflated, dst, workspace) : f.bpp == 2 ? unfilter_file<2, false>(L, f, inflated, dst, workspace)
               : f.bpp == 3 ? unfilter_file<3, false>(L, f, inflated, dst, workspace) : unfilter_file<4, false>(L, f, inflated, dst, workspace);
    }
    // one status word per work item: the seven passes of a file report apart and the interleave folds them
    if (threadIdx.x == 0) {
        if (item >= 0) reinterpret_cast<int *>(workspace)[item] = st;
        else status[index] = st;
    }
}

// ---- the Adam7 interleave ---------------------------------------------------------------------------------------------------------------
constexpr int kIlWaves = 4;                  // waves per workgroup, a row each at a time
constexpr int kIlRows = 16;                  // rows per workgroup
constexpr int kIlChunk = 128;                // output pixels per step of a wave: a multiple of 8, so every pass's stretch starts on its lattice
constexpr int kIlSlot = kIlChunk + 2;        // dwords of LDS per pass and wave: kIlChunk pixels of 4 bytes (the seventh pass's stretch)

__global__ __launch_bounds__(kIlWaves * 64) void png_adam7_interleave_kernel(PngAdam7Group grp, int count, const unsigned char *__restrict__ workspace,
                                                                             unsigned char *out, int *__restrict__ status)
{
    __shared__ unsigned slots[kIlWaves][7][kIlSlot];
    if ((int)blockIdx.y >= count) return;
    const PngAdam7File f = grp.f[blockIdx.y];
    if ((int)blockIdx.x * kIlRows >= f.H) return;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int oc = f.oc;
    // the file's status: the largest of its non-empty passes'; an image is assembled only from seven good passes
    int st = kOk;
    for (int p = 0; p < 7; p++)
        if (adam7_pass(f.W, f.H, p).w > 0) st = max(st, reinterpret_cast<const int *>(workspace)[f.item + p]);
    if (blockIdx.x == 0 && threadIdx.x == 0) status[f.file] = st;
    if (st != kOk) return;
    unsigned (*slot)[kIlSlot] = slots[wave];
    const int y_end = min(f.H, ((int)blockIdx.x + 1) * kIlRows);
    for (int y = (int)blockIdx.x * kIlRows + wave; y < y_end; y += kIlWaves) {
        const long long rowo = f.out_off + (long long)y * f.W * oc;
        for (int X0 = 0; X0 < f.W; X0 += kIlChunk) {
            const int X1 = min(X0 + kIlChunk, f.W);
            // ---- stage in: of every pass with pixels on row y, the stretch that falls into [X0, X1)
            long long img = f.img_off;
            for (int p = 0; p < 7; p++) {
                const Adam7Pass a = adam7_pass(f.W, f.H, p);
                const long long size = ((long long)a.w * a.h * oc + 3) & ~3LL;
                const int j0 = X0 >> a.sx;                                   // (X0 is a multiple of dx and x0 < dx)
                const int nj = min(a.w - j0, kIlChunk >> a.sx);
                if (a.w > 0 && y >= a.y0 && ((y - a.y0) & ((1 << a.sy) - 1)) == 0 && nj > 0) {
                    const long long src = img + ((long long)((y - a.y0) >> a.sy) * a.w + j0) * oc;
                    for (int i = lane; 4 * i < nj * oc; i += 64) slot[p][i] = load_dword_at(workspace, src + 4 * i, img, img + size);
                }
                img += size;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // ---- the row's bytes of pixels X0 .. X1, by whole dwords of `out`
            const long long o0 = rowo + (long long)X0 * oc, o1 = rowo + (long long)X1 * oc;
            const long long d0 = o0 - (long long)(reinterpret_cast<uintptr_t>(out + o0) & 3);
            for (long long d = d0 + 4 * lane; d < o1; d += 4 * 64) {
                const int rel = (int)(max(d, o0) - o0);
                int px = rel / oc, ch = rel - px * oc;                        // the pixel counted from X0
                unsigned word = 0;
                const bool whole = d >= o0 && d + 4 <= o1;
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    if (d + e < o0 || d + e >= o1) continue;
                    const int p = adam7_pass_of(px, y);                      // (X0 is a multiple of 8)
                    const Adam7Pass a = adam7_pass(f.W, f.H, p);
                    const unsigned v = reinterpret_cast<const unsigned char *>(slot[p])[((px - a.x0) >> a.sx) * oc + ch];
                    if (++ch == oc) { ch = 0; px++; }
                    if (whole) word |= v << (8 * e);
                    else out[d + e] = (unsigned char)v;
                }
                if (whole) *reinterpret_cast<unsigned *>(out + d) = word;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    }
}

// ---- the scanline filter of png_encode_many (aej_png_filter_batch) -------------------------------------------------------------------
// Encoding has no recurrence: a row is filtered against the RAW row above, so rows are independent.  One wave64 per row, kEncWaves rows
// per workgroup, all rows of up to kPngGroup images in one launch: a wave finds its image by a search over the group's first-row table.
// The wave makes two passes over its row, 256 bytes a step, a dword per lane.  Pass 1 forms the cost sum (v < 128 ? v : 256 - v) of the
// five filters' bytes in registers, reduces them across the wave and applies Pillow's rule (None; if its cost is not 0: Up, Sub, Average
// only with optimize, Paeth, each only if strictly cheaper).  Pass 2 recomputes the chosen filter and stores it behind the filter byte.
// "left" and "up-left" never come from memory: they are the lane's own dword and its neighbour's (the last lane's of the step before
// for lane 0, zero at the row's start -- the a = c = 0 columns), shifted by bpp bytes.
// SOURCE: H rows of rb bytes each, contiguous, any alignment (the caller makes a strided tensor contiguous first).  The lanes' dwords
// are aligned in the DESTINATION (rows are 1 + rb apart, so no alignment holds for both); the source is read as aligned dwords and a
// funnel shift, and only dwords that overlap the image are loaded.  A dword of the destination that is not wholly the row's is stored
// by bytes.  rb <= 2^24 keeps a cost sum inside an int; the entry refuses more.
constexpr int kEncWaves = 4;

// the four bytes at address p; aligned dwords that do not overlap [lo, hi) are not loaded and read as 0
__device__ inline unsigned load4_within(uintptr_t p, uintptr_t lo, uintptr_t hi)
{
    const uintptr_t a = p & ~(uintptr_t)3;
    const int sh = (int)(p & 3) * 8;
    unsigned v0 = 0u, v1 = 0u;
    if (a + 4 > lo && a < hi) v0 = *reinterpret_cast<const unsigned *>(a);
    if (sh && a + 8 > lo && a + 4 < hi) v1 = *reinterpret_cast<const unsigned *>(a + 4);
    return sh ? (v0 >> sh) | (v1 << (32 - sh)) : v0;
}

// filter type ft of byte x with a = left, b = up, c = up-left (PNG specification 9.2)
__device__ inline unsigned filter_byte(int ft, int x, int a, int b, int c)
{
    const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
    const int paeth = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
    const int pred = ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) >> 1 : ft == 4 ? paeth : 0;
    return (unsigned)(x - pred) & 255u;
}

__global__ __launch_bounds__(kEncWaves * 64) void png_filter_kernel(PngEncGroup grp, int count, int rows, int optimize, unsigned char *out)
{
    const int lane = threadIdx.x & 63;
    const int r = (int)blockIdx.x * kEncWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (r >= rows) return;
    int lo = 0, hi = count - 1;                                  // the last image whose first row is not beyond r
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (grp.f[mid].row0 <= r) lo = mid; else hi = mid - 1;
    }
    const PngEncImage f = grp.f[lo];
    const int y = r - f.row0, rb = f.rb, bpp = f.bpp;
    if (y < 0 || y >= f.H) return;
    const uintptr_t img_lo = reinterpret_cast<uintptr_t>(f.src), img_hi = img_lo + (size_t)f.H * (size_t)rb;
    const uintptr_t row = img_lo + (size_t)y * (size_t)rb;
    unsigned char *dst = out + f.dst_off + (long long)y * (rb + 1);         // the filter byte, then byte q of the row at dst[1 + q]
    const int q_first = -1 - (int)(reinterpret_cast<uintptr_t>(dst) & 3);   // row position of the first byte of dst's first dword (-1: the filter byte)

    // bytes q0 .. q0 + 3 of the row and of the row above; zero outside [0, rb) and above the first row
    auto load = [&](int q0, unsigned &x, unsigned &b) {
        x = 0u; b = 0u;
        if (q0 + 4 > 0 && q0 < rb) {
            unsigned mask = 0xffffffffu;
            if (q0 < 0) mask &= 0xffffffffu << (8 * -q0);
            if (q0 + 4 > rb) mask &= 0xffffffffu >> (8 * (q0 + 4 - rb));
            x = load4_within(row + (intptr_t)q0, img_lo, img_hi) & mask;
            if (y > 0) b = load4_within(row - (size_t)rb + (intptr_t)q0, img_lo, img_hi) & mask;
        }
    };
    // the dword bpp bytes to the left of `own`, whose left neighbour dword is `prev`
    auto left_of = [&](unsigned own, unsigned prev) {
        return bpp == 4 ? prev : (unsigned)(((unsigned long long)own << 32 | prev) >> (32 - 8 * bpp));
    };

    int cost[5] = { 0, 0, 0, 0, 0 };
    unsigned cx = 0u, cb = 0u;                                              // the last lane's dwords of the step before
    for (int base = q_first; base < rb; base += 256) {
        const int q0 = base + 4 * lane;
        unsigned x, b;
        load(q0, x, b);
        unsigned xp = __shfl_up(x, 1), bp = __shfl_up(b, 1);
        if (lane == 0) { xp = cx; bp = cb; }
        cx = (unsigned)__builtin_amdgcn_readlane((int)x, 63);
        cb = (unsigned)__builtin_amdgcn_readlane((int)b, 63);
        const unsigned a = left_of(x, xp), c = left_of(b, bp);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (q0 + j < 0 || q0 + j >= rb) continue;
            const int X = (x >> (8 * j)) & 255, A = (a >> (8 * j)) & 255, B = (b >> (8 * j)) & 255, C = (c >> (8 * j)) & 255;
#pragma unroll
            for (int ft = 0; ft < 5; ft++) {
                const int v = (int)filter_byte(ft, X, A, B, C);
                cost[ft] += v < 128 ? v : 256 - v;
            }
        }
    }
#pragma unroll
    for (int ft = 0; ft < 5; ft++)
        for (int o = 32; o > 0; o >>= 1) cost[ft] += __shfl_xor(cost[ft], o);
    int ft = 0, best = cost[0];
    if (best != 0) {
        if (cost[2] < best) { best = cost[2]; ft = 2; }
        if (cost[1] < best) { best = cost[1]; ft = 1; }
        if (optimize && cost[3] < best) { best = cost[3]; ft = 3; }
        if (cost[4] < best) { best = cost[4]; ft = 4; }
    }
    ft = __builtin_amdgcn_readfirstlane(ft);

    cx = 0u; cb = 0u;
    for (int base = q_first; base < rb; base += 256) {
        const int q0 = base + 4 * lane;
        unsigned x, b;
        load(q0, x, b);
        unsigned xp = __shfl_up(x, 1), bp = __shfl_up(b, 1);
        if (lane == 0) { xp = cx; bp = cb; }
        cx = (unsigned)__builtin_amdgcn_readlane((int)x, 63);
        cb = (unsigned)__builtin_amdgcn_readlane((int)b, 63);
        const unsigned a = left_of(x, xp), c = left_of(b, bp);
        unsigned word = 0u;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const unsigned v = q0 + j == -1 ? (unsigned)ft
                                            : filter_byte(ft, (x >> (8 * j)) & 255, (a >> (8 * j)) & 255, (b >> (8 * j)) & 255, (c >> (8 * j)) & 255);
            word |= v << (8 * j);
        }
        if (q0 >= -1 && q0 + 4 <= rb) *reinterpret_cast<unsigned *>(dst + 1 + q0) = word;
        else {
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (q0 + j >= -1 && q0 + j < rb) dst[1 + q0 + j] = (unsigned char)(word >> (8 * j));
        }
    }
}

}  // namespace

long long png_carry_bytes(int rb, int bpp) { return carry_bytes_of(rb, bpp); }

void launch_png_unfilter(hipStream_t st, const PngGroup &grp, int first, int count, const unsigned char *inflated, const long long *inflate_out_bytes,
                         const int *inflate_status, const unsigned char *palettes, unsigned char *out, unsigned char *workspace, int *status)
{
    // one launch for the files of up to 8 bits a sample, as ever, and one for the 16-bit files, where the group has any; seven
    // workgroups a file where a file of that kind is interlaced
    int passes[2] = { 0, 0 };
    for (int i = 0; i < count; i++) {
        int &p = passes[grp.f[i].depth == 16];
        p = std::max(p, grp.f[i].item >= 0 ? 7 : 1);
    }
    if (passes[0])
        hipLaunchKernelGGL(png_unfilter_kernel<false>, dim3(count, passes[0]), dim3(kWaves * 64), 0, st, grp, first, count, inflated, inflate_out_bytes,
                           inflate_status, palettes, out, workspace, status);
    if (passes[1])
        hipLaunchKernelGGL(png_unfilter_kernel<true>, dim3(count, passes[1]), dim3(kWaves * 64), 0, st, grp, first, count, inflated, inflate_out_bytes,
                           inflate_status, palettes, out, workspace, status);
}

void launch_png_adam7_interleave(hipStream_t st, const PngAdam7Group &grp, int count, int max_height, const unsigned char *workspace,
                                 unsigned char *out, int *status)
{
    if (count > 0 && max_height > 0)
        hipLaunchKernelGGL(png_adam7_interleave_kernel, dim3((max_height + kIlRows - 1) / kIlRows, count), dim3(kIlWaves * 64), 0, st, grp, count,
                           workspace, out, status);
}

void launch_png_filter(hipStream_t st, const PngEncGroup &grp, int count, int rows, int optimize, unsigned char *out)
{
    if (count > 0 && rows > 0)
        hipLaunchKernelGGL(png_filter_kernel, dim3((rows + kEncWaves - 1) / kEncWaves), dim3(kEncWaves * 64), 0, st, grp, count, rows, optimize, out);
}

}  // namespace aej
