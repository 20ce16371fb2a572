// requant.hip -- the quantised coefficients of an encoded batch under other quantisation tables, from the pre-quantisation DCT
// values the encode left in dct_f32 (aej_requantise_batch, include/aej.h).  The quantisation of jpeg.py:499-502 is the only step of
// the encode that depends on the quality range (jpeg.py:356-404, 485-506, 688-705), so a rate-distortion sweep runs colour, Canny,
// quadtree and DCT once per block range and this kernel once per group of quality ranges.
//
// Semantics: set j, coefficient i of a leaf of size s at layer offset off
//     out[j][off + i] = quantise(Y[off + zz_s[i]], Q_j[l][s][zz_s[i]])
// with zz_s the context's zigzag order (raster index at zigzag position i) and quantise() the DCT epilogues' own (aej_quant.h): the
// result is bit for bit what aej_encode_batch writes under set j.
//
// Shape: a streaming kernel (4 B of Y read once, 4 B per set written, per coefficient).  Every thread produces four consecutive zigzag
// positions of one leaf (s^2 is a multiple of four), so a set's writes are one 16-byte store per lane, contiguous across the lanes that
// work on one leaf -- and, since the encode lays the leaves of a layer end to end, across consecutive leaves too; Y is gathered inside
// the leaf.  Leaves of size <= 8 (at most 16 groups of four) are packed 64 per wave through a prefix sum; sizes 16 and 32 take one
// wave per leaf; 64 and above one workgroup per leaf.  The zigzag orders of sizes <= 32 and, while they fit, the quantisers of sizes
// <= 16 of every set (stored in zigzag order, so lanes read consecutive words) are staged in LDS; larger tables are read through L2.
#include "aej_common.h"
#include "aej_launch.h"
#include "aej_quant.h"

namespace aej {

constexpr int kRqThreads = 256;
constexpr int kRqSmallMax = 8;         // leaves up to this size are packed several per wave
constexpr int kRqWaveMax = 32;         // ... up to this size one wave per leaf; above it one workgroup per leaf

__global__ __launch_bounds__(kRqThreads) void k_requant_check(Geom g, QtGeom q, const int *__restrict__ leaves, const long long *__restrict__ counts,
                                                              const int *__restrict__ qmats, long long qmat_words, int *__restrict__ bad)
{
    const int l = blockIdx.y, b = blockIdx.z, plane = b * 3 + l;
    long long n = counts[(long long)plane * 4 + 1];
    if (n < 0 || n > q.leaf_cap[l]) {
        if (blockIdx.x == 0 && threadIdx.x == 0) *bad = 1;
        n = 0;
    }
    const int4 *tab = reinterpret_cast<const int4 *>(leaves) + (long long)b * q.leaf_stride + q.leaf_off[l];
    for (long long i = (long long)blockIdx.x * kRqThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kRqThreads) {
        const int4 lf = tab[i];
        const bool size_ok = lf.z >= q.bmin && lf.z <= q.bmax && (lf.z & (lf.z - 1)) == 0;
        // the same bounds as aej_decode_batch's tables: origin inside the layer, coefficients inside the layer's span
        if (!size_ok || lf.x < 0 || lf.y < 0 || lf.x >= g.w[l] || lf.y >= g.h[l] || lf.w < 0 ||
            (long long)lf.w + (long long)lf.z * lf.z > q.coeff_cap[l])
            *bad = 1;
    }
    if (l == 0 && b == 0)      // the quantisers of every set (the codec's tables are >= 1: jpeg.py:724 clips at 1)
        for (long long i = (long long)blockIdx.x * kRqThreads + threadIdx.x; i < qmat_words; i += (long long)gridDim.x * kRqThreads)
            if (qmats[i] < 1) *bad = 2;
}

struct RqArgs {
    const float *dct;          // [B][coeff_stride] raster order per leaf
    const int *leaves;         // [B][leaf_stride][4]
    const long long *counts;   // [B][3][4]
    const int *qmats;          // [n_sets][3][sizes][s*s] raster order
    int *out;                  // set j at out + j * set_stride
    long long set_stride;
    int n_sets;
    long long set_words, layer_words;      // per set, per layer of a set
    long long qoff[kMaxSizes];             // offset of size k inside a layer
    const int *zz[kMaxSizes];              // zigzag order (raster index at zigzag position), the context's
    int lds_zz_off[kMaxSizes];             // LDS word offset of zz[k] (-1: read from global)
    int lds_q_off[kMaxSizes];              // LDS word offset of set 0's zigzag-ordered quantisers of size k (-1: global); set j at + j * lds_q_set
    int lds_q_set;
    int lds_words;
    const int *bad;
};

// the four zigzag positions i .. i + 3 of the leaf at layer offset `off` (size index k) for every set
__device__ __forceinline__ void rq_group(const RqArgs &a, const int *lds, int l, int k, long long base, int off, int i)
{
    int r[4];
    if (a.lds_zz_off[k] >= 0) {
        const int4 z = *reinterpret_cast<const int4 *>(lds + a.lds_zz_off[k] + i);
        r[0] = z.x; r[1] = z.y; r[2] = z.z; r[3] = z.w;
    } else {
        const int4 z = *reinterpret_cast<const int4 *>(a.zz[k] + i);
        r[0] = z.x; r[1] = z.y; r[2] = z.z; r[3] = z.w;
    }
    const float *Y = a.dct + base + off;
    float y[4];
#pragma unroll
    for (int c = 0; c < 4; c++) y[c] = __builtin_nontemporal_load(Y + r[c]);
    const bool aligned = ((base + off + i) & 3) == 0 && (a.set_stride & 3) == 0;
    int *o = a.out + base + off + i;
    for (int j = 0; j < a.n_sets; j++, o += a.set_stride) {
        int qv[4];
        if (a.lds_q_off[k] >= 0) {
            const int4 v = *reinterpret_cast<const int4 *>(lds + a.lds_q_off[k] + j * a.lds_q_set + i);
            qv[0] = v.x; qv[1] = v.y; qv[2] = v.z; qv[3] = v.w;
        } else {
            const int *Q = a.qmats + j * a.set_words + l * a.layer_words + a.qoff[k];
#pragma unroll
            for (int c = 0; c < 4; c++) qv[c] = Q[r[c]];
        }
        int v[4];
#pragma unroll
        for (int c = 0; c < 4; c++) v[c] = quantise(y[c], qv[c]);
        if (aligned) *reinterpret_cast<int4 *>(o) = make_int4(v[0], v[1], v[2], v[3]);
        else { o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = v[3]; }
    }
}

__global__ __launch_bounds__(kRqThreads) void k_requant(Geom g, QtGeom q, RqArgs a)
{
    extern __shared__ int lds[];       // [a.lds_words] staged tables, then [4 waves][64] group prefix + [4][64] leaf offsets + [4][64] size index
    if (*a.bad) return;                // the leaf tables or the quantisers failed k_requant_check: nothing is written
    const int l = blockIdx.y, b = blockIdx.z, plane = b * 3 + l;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long n = a.counts[(long long)plane * 4 + 1];
    const int4 *tab = reinterpret_cast<const int4 *>(a.leaves) + (long long)b * q.leaf_stride + q.leaf_off[l];
    const long long base = (long long)b * q.coeff_stride + q.coeff_off[l];
    const int bmin_log2 = 31 - __clz(q.bmin);

    // stage the small tables: zigzag orders, and this layer's quantisers of every set in zigzag order
    for (int k = 0; k < q.nsizes; k++) {
        const int s = q.bmin << k, ss = s * s;
        if (a.lds_zz_off[k] >= 0)
            for (int i = tid; i < ss; i += kRqThreads) lds[a.lds_zz_off[k] + i] = a.zz[k][i];
        if (a.lds_q_off[k] >= 0)
            for (int e = tid; e < a.n_sets * ss; e += kRqThreads) {
                const int j = e / ss, i = e - j * ss;
                lds[a.lds_q_off[k] + j * a.lds_q_set + i] = a.qmats[j * a.set_words + l * a.layer_words + a.qoff[k] + a.zz[k][i]];
            }
    }
    __syncthreads();

    // 1. leaves of size <= kRqSmallMax: 64 leaves per wave, their groups of four dealt out to the lanes through a prefix sum
    int *pre = lds + a.lds_words + wave * 192, *offs = pre + 64, *ks = pre + 128;
    for (long long c0 = ((long long)blockIdx.x * 4 + wave) * 64; c0 < n; c0 += (long long)gridDim.x * 4 * 64) {
        const long long i = c0 + lane;
        int ng = 0, k = 0, off = 0;
        if (i < n) {
            const int4 lf = tab[i];
            if (lf.z <= kRqSmallMax) { ng = lf.z * lf.z / 4; k = (31 - __clz(lf.z)) - bmin_log2; off = lf.w; }
        }
        const int incl = wave_scan_incl(ng);
        const int total = __builtin_amdgcn_readlane(incl, 63);
        pre[lane] = incl - ng; offs[lane] = off; ks[lane] = k;
        __builtin_amdgcn_wave_barrier();
        for (int e = lane; e < total; e += 64) {
            int lo = 0, hi = 63;                 // the last leaf whose first group is <= e (it has groups: see the prefix)
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (pre[mid] <= e) lo = mid; else hi = mid - 1;
            }
            rq_group(a, lds, l, ks[lo], base, offs[lo], 4 * (e - pre[lo]));
        }
        __builtin_amdgcn_wave_barrier();
    }
    // 2. sizes 16 and 32: one wave per leaf
    for (long long i = (long long)blockIdx.x * 4 + wave; i < n; i += (long long)gridDim.x * 4) {
        const int4 lf = tab[i];
        if (lf.z <= kRqSmallMax || lf.z > kRqWaveMax) continue;
        const int k = (31 - __clz(lf.z)) - bmin_log2, ng = lf.z * lf.z / 4;
        for (int e = lane; e < ng; e += 64) rq_group(a, lds, l, k, base, lf.w, 4 * e);
    }
    // 3. sizes >= 64: one workgroup per leaf
    for (long long i = blockIdx.x; i < n; i += gridDim.x) {
        const int4 lf = tab[i];
        if (lf.z <= kRqWaveMax) continue;
        const int k = (31 - __clz(lf.z)) - bmin_log2, ng = lf.z * lf.z / 4;
        for (int e = tid; e < ng; e += kRqThreads) rq_group(a, lds, l, k, base, lf.w, 4 * e);
    }
}

// host side ---------------------------------------------------------------------------------------------------------------
int launch_requant(hipStream_t st, const Geom &g, const QtGeom &q, const float *dct, const int *leaves, const long long *counts, int n_sets,
                   const int *qmats, const int *const *zz, int *out, long long set_stride, int *bad, int blocks_per_plane)
{
    RqArgs a = {};
    a.dct = dct; a.leaves = leaves; a.counts = counts; a.qmats = qmats; a.out = out; a.set_stride = set_stride; a.n_sets = n_sets; a.bad = bad;
    long long lw = 0;
    for (int k = 0; k < q.nsizes; k++) { const int s = q.bmin << k; a.qoff[k] = lw; lw += (long long)s * s; a.zz[k] = zz[k]; }
    a.layer_words = lw; a.set_words = 3 * lw;
    // LDS: zigzag orders of the sizes <= 32, then the quantisers of the sizes <= 16 for every set while they fit in 32 KiB
    int words = 0, qwords = 0;
    for (int k = 0; k < kMaxSizes; k++) { a.lds_zz_off[k] = -1; a.lds_q_off[k] = -1; }
    for (int k = 0; k < q.nsizes; k++) {
        const int s = q.bmin << k;
        if (s <= kRqWaveMax) { a.lds_zz_off[k] = words; words += s * s; }
        if (s <= 16) qwords += s * s;
    }
    if (qwords > 0 && (long long)words + (long long)qwords * n_sets <= 8192) {
        a.lds_q_set = qwords;
        int o = words;
        for (int k = 0; k < q.nsizes; k++) { const int s = q.bmin << k; if (s <= 16) { a.lds_q_off[k] = o; o += s * s; } }
        words += qwords * n_sets;
    }
    a.lds_words = words;
    const size_t lds = ((size_t)words + 4 * 192) * sizeof(int);
    hipLaunchKernelGGL(k_requant, dim3(blocks_per_plane, 3, g.B), dim3(kRqThreads), lds, st, g, q, a);
    return 0;
}

void launch_requant_check(hipStream_t st, const Geom &g, const QtGeom &q, const int *leaves, const long long *counts, const int *qmats,
                          long long qmat_words, int *bad)
{
    long long maxcap = 0;
    for (int l = 0; l < 3; l++) maxcap = q.leaf_cap[l] > maxcap ? q.leaf_cap[l] : maxcap;
    long long bx = (maxcap + kRqThreads - 1) / kRqThreads;
    const long long bq = (qmat_words + kRqThreads - 1) / kRqThreads;
    if (bq > bx) bx = bq;
    if (bx > 1024) bx = 1024;
    if (bx < 1) bx = 1;
    hipLaunchKernelGGL(k_requant_check, dim3((unsigned)bx, 3, g.B), dim3(kRqThreads), 0, st, g, q, leaves, counts, qmats, qmat_words, bad);
}

}  // namespace aej
