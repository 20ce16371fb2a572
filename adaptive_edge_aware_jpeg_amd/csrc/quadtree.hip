// quadtree.hip -- QuadTree._build_tree + get_leaves_and_states (src/jpeg/quadtree.py:93-165) without a
// tree walk.  gfx950 only.
//
// The reference splits top-down with an explicit stack; a node (x, y, s) splits iff
//     s > max_size  or  (s > min_size and any(edge[y:y+s, x:x+s])).
// Order-free restatement used here (equivalence is checked against the reference-generated golden cases):
//   * "any(edge)" over aligned squares is an OR-pyramid over min-size cells;
//   * the pre-order DFS sequence of (internal '01' / leaf '00' / out-of-bounds child '10') symbols is the
//     sequence of all existing nodes sorted by (Morton code of origin, descending size), so a cell in Morton
//     order emits the nodes that *originate* at it, largest first;
//   * leaves in DFS order are therefore in ascending Morton order of their origin cell.
// Three passes over 256-cell (16x16, Morton-aligned) chunks: OR-pyramid, per-chunk counts, prefix sums, emit.
#include "aej_common.h"
#include "aej_launch.h"
#include <algorithm>
#include <string.h>

namespace aej {

__device__ __forceinline__ unsigned compact1by1(unsigned v)
{
    v &= 0x55555555u;
    v = (v | (v >> 1)) & 0x33333333u;
    v = (v | (v >> 2)) & 0x0F0F0F0Fu;
    v = (v | (v >> 4)) & 0x00FF00FFu;
    v = (v | (v >> 8)) & 0x0000FFFFu;
    return v;
}
// Morton code with x in the even bits, y in the odd bits (children order TL, TR, BL, BR: quadtree.py:123-131)
__device__ __forceinline__ void morton_decode(unsigned m, int &x, int &y) { x = (int)compact1by1(m); y = (int)compact1by1(m >> 1); }

__device__ __forceinline__ long long lvl_off(int ncell, int lv)
{
    long long o = 0;
    for (int j = 0; j < lv; j++) { long long s = ncell >> j; o += s * s; }
    return o;
}

// ------------------------------------------------------------------------------------------------
// OR-pyramid and node evaluation, one WAVE per chunk.
// A chunk is a Morton-aligned square of 16x16 min-size cells (256 cells); lane t owns the four sibling cells
// 4t..4t+3 (= one level-1 node), so levels 0..1 of the pyramid are lane-local and levels 2..4 are nibble / 16-bit /
// whole-word tests on one wave ballot.  Levels >= 5 (only needed when bmax/bmin >= 32) are a tiny global array
// filled by k_qt_upper with idempotent stores of 1.  No LDS, no workgroup barriers.
// ------------------------------------------------------------------------------------------------
struct ChunkEdges {
    unsigned e0;             // bit i = OR over cell 4*lane + i
    bool e1, e2, e3, e4;     // OR over the lane's level-1 / 2 / 3 / 4 ancestors
};

__device__ __forceinline__ ChunkEdges chunk_edges(const Geom &g, const QtGeom &q, int l, int b, const unsigned long long *__restrict__ edge_bits,
                                                  unsigned chunk, int lane)
{
    const int ncell = q.ncell[l], cell = q.cell;
    const int w = g.w[l], h = g.h[l], wpr = g.wpr[l];
    int ccx, ccy, lx, ly;
    morton_decode(chunk, ccx, ccy);
    morton_decode((unsigned)lane, lx, ly);
    const unsigned long long *src = edge_bits + (long long)b * g.bpstride + g.bpoff[l];
    ChunkEdges E;
    E.e0 = 0;
    if (cell == 4 && ncell >= 16) {
        // fast path (min block 4): the chunk is one 64x64 bit-plane tile = 64 contiguous words; this lane's four cells are the
        // 8x8-pixel square at rows 8*ly.., bits 8*lx..: eight word loads issued together, then nibble tests
        const int X0 = ccx * 64, Y0 = ccy * 64;
        if (X0 < w && Y0 < h) {
            const unsigned long long *tile = src + bp_index(Y0, X0 >> 6, wpr);
            unsigned rows[8];
#pragma unroll
            for (int r = 0; r < 8; r++) {
                const int y = Y0 + 8 * ly + r;
                rows[r] = y < h ? (unsigned)((tile[8 * ly + r] >> (8 * lx)) & 0xFFull) : 0u;
            }
            const unsigned top = rows[0] | rows[1] | rows[2] | rows[3], bot = rows[4] | rows[5] | rows[6] | rows[7];
            E.e0 = ((top & 0x0Fu) ? 1u : 0u) | ((top & 0xF0u) ? 2u : 0u) | ((bot & 0x0Fu) ? 4u : 0u) | ((bot & 0xF0u) ? 8u : 0u);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int cx = ccx * 16 + lx * 2 + (i & 1), cy = ccy * 16 + ly * 2 + (i >> 1);
            if (cx < ncell && cy < ncell && cx * cell < w && cy * cell < h) {
                int x0 = cx * cell, y0 = cy * cell;
                int x1 = min(x0 + cell, w), y1 = min(y0 + cell, h);
                bool e = false;
                for (int y = y0; y < y1; y++)
                    for (int xw = x0 >> 6; xw <= (x1 - 1) >> 6; xw++) {
                        int lo = max(x0, xw * 64) - xw * 64, hi = min(x1, xw * 64 + 64) - xw * 64;
                        unsigned long long mask = (hi - lo == 64) ? ~0ull : (((1ull << (hi - lo)) - 1ull) << lo);
                        e |= (src[bp_index(y, xw, wpr)] & mask) != 0;
                    }
                E.e0 |= (e ? 1u : 0u) << i;
            }
        }
    }
    E.e1 = E.e0 != 0;
    const unsigned long long m = __ballot(E.e1);
    E.e2 = ((m >> (lane & ~3)) & 0xFull) != 0;
    E.e3 = ((m >> (lane & ~15)) & 0xFFFFull) != 0;
    E.e4 = m != 0;
    return E;
}

// The chunk kernels run on a grid of (sum over layers of ceil(nchunk / 4), batch): the layers have different chunk counts (a 4:2:0
// chroma plane has a quarter of the luma's), and a grid sized for the largest layer launched twice as many waves as it needed.
__device__ __forceinline__ bool locate_chunk_block(const QtGeom &q, int nl, int bx, int &l, unsigned &chunk0)
{
    for (l = 0; l < nl; l++) {
        const int nb = (q.nchunk[l] + 3) >> 2;
        if (bx < nb) { chunk0 = (unsigned)bx * 4u; return true; }
        bx -= nb;
    }
    return false;
}

__global__ __launch_bounds__(256) void k_qt_upper(Geom g, QtGeom q, const unsigned long long *__restrict__ edge_bits, unsigned char *__restrict__ pyr_all)
{
    const int b = blockIdx.y;
    int l;
    unsigned chunk;
    if (!locate_chunk_block(q, g.nl, (int)blockIdx.x, l, chunk)) return;
    const int lane = threadIdx.x & 63;
    chunk += threadIdx.x >> 6;
    const int ncell = q.ncell[l], ltot = q.ltot[l], cell = q.cell;
    if ((long long)chunk >= q.nchunk[l] || ltot <= 4) return;
    int ccx, ccy;
    morton_decode(chunk, ccx, ccy);
    if (ccx * 16 * cell >= g.w[l] || ccy * 16 * cell >= g.h[l]) return;
    ChunkEdges E = chunk_edges(g, q, l, b, edge_bits, chunk, lane);
    if (lane == 0 && E.e4) {
        unsigned char *pyr = pyr_all + (long long)b * q.pyr_stride + q.pyr_off[l];
        for (int k = 5; k <= ltot && (cell << k) <= q.bmax; k++) {
            int side = ncell >> k;
            pyr[lvl_off(ncell, k) + (long long)((ccy * 16) >> k) * side + ((ccx * 16) >> k)] = 1;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// per-cell node evaluation shared by the count and emit passes
// ------------------------------------------------------------------------------------------------
struct CellNodes {
    int nsym;        // number of symbols originating at this cell
    unsigned syms;   // 2 bits per symbol, first emitted in the low bits
    int leaf_lvl;    // level of the leaf originating here, or -1
};

// edge(level lvn ancestor of cell gidx = 256*chunk + 4*lane + i)
__device__ __forceinline__ bool node_edge(const QtGeom &q, int l, const ChunkEdges &E, const unsigned char *__restrict__ pyr, int i, int cx, int cy, int lvn)
{
    switch (lvn) {
    case 0: return (E.e0 >> i) & 1u;
    case 1: return E.e1;
    case 2: return E.e2;
    case 3: return E.e3;
    case 4: return E.e4;
    default: {
        const int ncell = q.ncell[l], side = ncell >> lvn;
        return pyr[lvl_off(ncell, lvn) + (long long)(cy >> lvn) * side + (cx >> lvn)] != 0;
    }
    }
}

__device__ __forceinline__ CellNodes eval_cell(const QtGeom &q, int l, int w, int h, const ChunkEdges &E, const unsigned char *__restrict__ pyr, unsigned gidx,
                                               int cx, int cy)
{
    CellNodes r;
    r.nsym = 0; r.syms = 0; r.leaf_lvl = -1;
    const int ltot = q.ltot[l], cell = q.cell, i = (int)(gidx & 3u);
    int a = gidx == 0 ? ltot : min((int)(__ffs((int)gidx) - 1) >> 1, ltot);
    if (a < ltot) {
        // the level-a node exists only if its parent is in bounds and splits
        int mask = ~((2 << a) - 1);
        int pcx = cx & mask, pcy = cy & mask;
        if (pcx * cell >= w || pcy * cell >= h) return r;
        int psize = cell << (a + 1);
        bool psplit = psize > q.bmax;
        if (!psplit && psize > q.bmin) psplit = node_edge(q, l, E, pyr, i, cx, cy, a + 1);
        if (!psplit) return r;
    }
    if (cx * cell >= w || cy * cell >= h) {   // quadtree.py:109-110, 153-155: absent child
        r.nsym = 1; r.syms = 2u;
        return r;
    }
    for (int lvn = a; lvn >= 0; lvn--) {
        int size = cell << lvn;
        bool split = size > q.bmax;
        if (!split && size > q.bmin) split = node_edge(q, l, E, pyr, i, cx, cy, lvn);
        if (split) {
            r.syms |= 1u << (2 * r.nsym);
            r.nsym++;
        } else {
            r.nsym++;          // '00'
            r.leaf_lvl = lvn;
            break;
        }
    }
    return r;
}

// The four sibling cells of a lane.  Cell 0 may be the origin of nodes of any level (general walk); cells 1..3 can only
// originate their own level-0 node, which exists iff the lane's level-1 node is in bounds and splits -- the same test
// eval_cell makes, evaluated once for the three of them.
__device__ __forceinline__ void eval_lane(const QtGeom &q, int l, int w, int h, const ChunkEdges &E, const unsigned char *__restrict__ pyr, unsigned chunk,
                                          int lane, long long ncell2, CellNodes (&c)[4], int &cx0, int &cy0)
{
    int ccx, ccy, lx, ly;
    morton_decode(chunk, ccx, ccy);
    morton_decode((unsigned)lane, lx, ly);
    cx0 = ccx * 16 + lx * 2; cy0 = ccy * 16 + ly * 2;
    const unsigned g0 = chunk * 256u + (unsigned)lane * 4u;
#pragma unroll
    for (int i = 0; i < 4; i++) { c[i].nsym = 0; c[i].syms = 0; c[i].leaf_lvl = -1; }
    if ((long long)g0 >= ncell2) return;
    c[0] = eval_cell(q, l, w, h, E, pyr, g0, cx0, cy0);
    const int cell = q.cell;
    bool split1 = 2 * cell > q.bmax;
    if (!split1 && 2 * cell > q.bmin) split1 = E.e1;
    if (!(split1 && cx0 * cell < w && cy0 * cell < h)) return;
#pragma unroll
    for (int i = 1; i < 4; i++) {
        if ((long long)(g0 + i) >= ncell2) continue;
        const int cx = cx0 + (i & 1), cy = cy0 + (i >> 1);
        c[i].nsym = 1;
        if (cx * cell >= w || cy * cell >= h) c[i].syms = 2u;                                           // absent child '10'
        else if (cell > q.bmax || (cell > q.bmin && ((E.e0 >> i) & 1u))) c[i].syms = 1u;                // '01'
        else c[i].leaf_lvl = 0;                                                                         // '00'
    }
}

// The count pass leaves what it found for the emit pass in 12 bits per lane, so the emit pass neither re-reads the edge
// bit-plane nor walks the levels again.  Cell 0 originates k >= 0 split symbols '01' followed by a leaf '00' (type 1), nothing
// (type 2), or it is a single absent child '10' (type 3); cells 1..3 originate at most one symbol (0 none, 1 '00', 2 '01', 3 '10').
__device__ __forceinline__ unsigned pack_lane(const CellNodes (&c)[4])
{
    unsigned code = 0;
    if (c[0].nsym > 0) {
        if (c[0].nsym == 1 && c[0].syms == 2u) code = 3u;
        else {
            const int k = c[0].nsym - (c[0].leaf_lvl >= 0 ? 1 : 0);
            code = (c[0].leaf_lvl >= 0 ? 1u : 2u) | ((unsigned)k << 2);
        }
    }
#pragma unroll
    for (int i = 1; i < 4; i++) {
        const unsigned ci = c[i].nsym == 0 ? 0u : (c[i].syms == 2u ? 3u : c[i].syms == 1u ? 2u : 1u);
        code |= ci << (4 + 2 * i);
    }
    return code;
}

__device__ __forceinline__ void unpack_lane(unsigned code, unsigned g0, int ltot, CellNodes (&c)[4])
{
#pragma unroll
    for (int i = 0; i < 4; i++) { c[i].nsym = 0; c[i].syms = 0; c[i].leaf_lvl = -1; }
    const unsigned t = code & 3u;
    const int k = (int)((code >> 2) & 15u);
    if (t == 3u) { c[0].nsym = 1; c[0].syms = 2u; }
    else if (t != 0u) {
        const int a = g0 == 0 ? ltot : min((int)(__ffs((int)g0) - 1) >> 1, ltot);      // level of the largest node originating here
        c[0].syms = 0x55555555u & ((1u << (2 * k)) - 1u);
        c[0].nsym = k + (t == 1u ? 1 : 0);
        if (t == 1u) c[0].leaf_lvl = a - k;
    }
#pragma unroll
    for (int i = 1; i < 4; i++) {
        const unsigned ci = (code >> (4 + 2 * i)) & 3u;
        if (ci) { c[i].nsym = 1; c[i].syms = ci == 3u ? 2u : ci == 2u ? 1u : 0u; c[i].leaf_lvl = ci == 1u ? 0 : -1; }
    }
}

__device__ __forceinline__ int wave_incl_scan(int v, int /*lane*/) { return wave_scan_incl(v); }      // aej_common.h: DPP, all lanes active
__device__ __forceinline__ int wave_sum(int v) { return wave_total(v); }

// pass 2: per-chunk totals (symbols, leaves, coefficients, leaves per block size); one wave per chunk
__global__ __launch_bounds__(256) void k_qt_count(Geom g, QtGeom q, const unsigned long long *__restrict__ edge_bits,
                                                  const unsigned char *__restrict__ pyr_all, int *__restrict__ chunk_cnt,
                                                  unsigned short *__restrict__ lane_code)
{
    const int b = blockIdx.y;
    int l;
    unsigned chunk;
    if (!locate_chunk_block(q, g.nl, (int)blockIdx.x, l, chunk)) return;
    const int lane = threadIdx.x & 63;
    chunk += threadIdx.x >> 6;
    if ((long long)chunk >= q.nchunk[l]) return;
    const long long ncell2 = (long long)q.ncell[l] * q.ncell[l];
    const unsigned char *pyr = pyr_all + (long long)b * q.pyr_stride + q.pyr_off[l];
    {
        // A chunk that lies wholly outside the plane (about half of the root square) can originate one thing only: the
        // absent-child symbol '10' of a node whose origin is the chunk's first cell.  Only lane 0 has anything to evaluate.
        int ccx, ccy;
        morton_decode(chunk, ccx, ccy);
        if (ccx * 16 * q.cell >= g.w[l] || ccy * 16 * q.cell >= g.h[l]) {
            ChunkEdges Z;
            Z.e0 = 0; Z.e1 = Z.e2 = Z.e3 = Z.e4 = false;
            int ns = 0;
            if (lane == 0 && (long long)chunk * 256 < ncell2) ns = eval_cell(q, l, g.w[l], g.h[l], Z, pyr, chunk * 256u, ccx * 16, ccy * 16).nsym;
            lane_code[((long long)b * q.chunk_stride + q.chunk_off[l] + chunk) * 64 + lane] = (unsigned short)(ns ? 3u : 0u);
            if (lane == 0) {
                int *o = chunk_cnt + ((long long)b * q.chunk_stride + q.chunk_off[l] + chunk) * kChunkInts;
                o[0] = ns; o[1] = 0; o[2] = 0; o[3] = 0;
#pragma unroll
                for (int k = 0; k < kMaxSizes; k++) o[4 + k] = 0;
            }
            return;
        }
    }
    const ChunkEdges E = chunk_edges(g, q, l, b, edge_bits, chunk, lane);
    if (!E.e4 && (q.cell << 4) <= q.bmax) {
        // A chunk without a single edge pixel whose own size does not exceed the maximum block: no node inside it splits, so
        // the only cell that can originate anything is the chunk's first one (the chunk itself as a leaf, or as the origin of a
        // larger node: the general walk, on lane 0 alone).  No sibling tests, no wave reductions -- this is every chunk of a
        // flat region (41 % of the bench planes' area).
        CellNodes z[4];
#pragma unroll
        for (int i = 0; i < 4; i++) { z[i].nsym = 0; z[i].syms = 0; z[i].leaf_lvl = -1; }
        if (lane == 0 && (long long)chunk * 256 < ncell2) {
            int ccx, ccy;
            morton_decode(chunk, ccx, ccy);
            z[0] = eval_cell(q, l, g.w[l], g.h[l], E, pyr, chunk * 256u, ccx * 16, ccy * 16);
        }
        lane_code[((long long)b * q.chunk_stride + q.chunk_off[l] + chunk) * 64 + lane] = (unsigned short)pack_lane(z);
        if (lane == 0) {
            int *o = chunk_cnt + ((long long)b * q.chunk_stride + q.chunk_off[l] + chunk) * kChunkInts;
            const int lv = z[0].leaf_lvl, sz = lv >= 0 ? q.cell << lv : 0;
            o[0] = z[0].nsym; o[1] = lv >= 0 ? 1 : 0; o[2] = sz * sz; o[3] = 0;
#pragma unroll
            for (int k = 0; k < kMaxSizes; k++) o[4 + k] = (k == lv) ? 1 : 0;
        }
        return;
    }
    int nsym = 0, nleaf = 0, ncoef = 0;
    int nsz[kMaxSizes];
#pragma unroll
    for (int k = 0; k < kMaxSizes; k++) nsz[k] = 0;
    CellNodes cn[4];
    int cx0, cy0;
    eval_lane(q, l, g.w[l], g.h[l], E, pyr, chunk, lane, ncell2, cn, cx0, cy0);
    lane_code[((long long)b * q.chunk_stride + q.chunk_off[l] + chunk) * 64 + lane] = (unsigned short)pack_lane(cn);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const CellNodes &c = cn[i];
        nsym += c.nsym;
        if (c.leaf_lvl >= 0) {
            nleaf++;
            int s = q.cell << c.leaf_lvl;
            ncoef += s * s;
#pragma unroll
            for (int k = 0; k < kMaxSizes; k++) nsz[k] += (c.leaf_lvl == k) ? 1 : 0;
        }
    }
    // wave totals: the symbol count (< 1024 per chunk) and the per-size leaf counts (<= 256) travel three to a word through the
    // butterfly; leaves and coefficients follow from the per-size counts
    static_assert(kMaxSizes <= 8, "three packed words hold the symbol count and 8 sizes");
    unsigned pk[3] = { (unsigned)nsym, 0u, 0u };
#pragma unroll
    for (int k = 0; k < kMaxSizes; k++) pk[(k + 1) / 3] |= (unsigned)nsz[k] << (10 * ((k + 1) % 3));
#pragma unroll
    for (int i = 0; i < 3; i++) pk[i] = (unsigned)wave_sum((int)pk[i]);
    nsym = (int)(pk[0] & 1023u);
    nleaf = 0; ncoef = 0;
#pragma unroll
    for (int k = 0; k < kMaxSizes; k++) {
        nsz[k] = k < q.nsizes ? (int)((pk[(k + 1) / 3] >> (10 * ((k + 1) % 3))) & 1023u) : 0;
        const int sz = q.cell << k;
        nleaf += nsz[k];
        ncoef += nsz[k] * sz * sz;
    }
    if (lane == 0) {
        int *o = chunk_cnt + ((long long)b * q.chunk_stride + q.chunk_off[l] + chunk) * kChunkInts;
        o[0] = nsym; o[1] = nleaf; o[2] = ncoef; o[3] = 0;
#pragma unroll
        for (int k = 0; k < kMaxSizes; k++) o[4 + k] = nsz[k];
    }
}

// pass 3: exclusive scan of the chunk records per (image, layer); totals -> counts and per-plane work counts.
// 256 threads (round 3; was 1024): a workgroup of 16 waves needs four free wave slots with 56 registers on EVERY SIMD of one CU, which
// in the pipelined path it waited for behind the other chains' resident workgroups (211 us per launch under overlap against 45 us alone);
// four waves fit into the gaps.  A call of a few images has nothing to wait behind and keeps the 1024-thread shape (fewer serial
// rounds: it is latency there).
template <int kScanThreads>
__global__ __launch_bounds__(kScanThreads) void k_qt_scan(Geom g, QtGeom q, int *__restrict__ chunk_cnt, long long *__restrict__ counts,
                                                  int *__restrict__ work_count)
{
    constexpr int NQ = 3 + kMaxSizes;
    __shared__ int s_w[NQ][kScanThreads / 64];
    __shared__ int carry[NQ];
    const int tid = threadIdx.x, l = blockIdx.x, b = blockIdx.y;
    const int lane = tid & 63, wv = tid >> 6;
    int *base = chunk_cnt + ((long long)b * q.chunk_stride + q.chunk_off[l]) * kChunkInts;
    const int n = q.nchunk[l];
    const int nq = 3 + q.nsizes;
    if (tid < NQ) carry[tid] = 0;
    __syncthreads();
    static_assert(kChunkInts == 12 && NQ == 11, "a chunk record is three int4: (nsym, nleaf, ncoef, pad), leaves per size 0..3, 4..7");
    int4 *rec = reinterpret_cast<int4 *>(base);          // (chunk records start on 16-byte boundaries: 48 bytes each, workspace carved at 256)
    for (int start = 0; start < n; start += kScanThreads) {
        const int i = start + tid;
        // the record as three 16-byte loads (a wave reads 3 KiB contiguously) instead of eleven strided dword loads
        int4 r0 = make_int4(0, 0, 0, 0), r1 = r0, r2 = r0;
        if (i < n) { r0 = rec[3 * i]; r1 = rec[3 * i + 1]; r2 = rec[3 * i + 2]; }
        int v[NQ] = { r0.x, r0.y, r0.z, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w }, inc[NQ];
#pragma unroll
        for (int c = 0; c < NQ; c++) {
            if (c >= nq) v[c] = 0;
            inc[c] = wave_incl_scan(v[c], lane);
            if (lane == 63) s_w[c][wv] = inc[c];
        }
        __syncthreads();
        int o[NQ];
#pragma unroll
        for (int c = 0; c < NQ; c++) {
            int p = carry[c];
            for (int k = 0; k < wv; k++) p += s_w[c][k];
            o[c] = p + inc[c] - v[c];
        }
        if (i < n) {
            rec[3 * i] = make_int4(o[0], o[1], o[2], r0.w);
            rec[3 * i + 1] = make_int4(o[3], o[4], o[5], o[6]);
            rec[3 * i + 2] = make_int4(o[7], o[8], o[9], o[10]);
        }
        __syncthreads();
        if (tid < NQ) {
            int t = 0;
            for (int k = 0; k < kScanThreads / 64; k++) t += s_w[tid][k];
            carry[tid] += t;
        }
        __syncthreads();
    }
    if (tid == 0) {
        long long *o = counts + ((long long)b * 3 + l) * 4;
        o[0] = carry[2];      // n_coeffs
        o[1] = carry[1];      // n_leaves
        o[2] = carry[0];      // n_states
        o[3] = q.root[l];
    }
    if (work_count && tid < kMaxSizes) work_count[((long long)b * 3 + l) * kMaxSizes + tid] = tid < q.nsizes ? carry[3 + tid] : 0;
}

// pass 4: emit symbols, leaf table and the per-size DCT work lists; one wave per chunk.  Positions come from the
// scans (deterministic, Morton-ordered lists, no global atomics).
__global__ __launch_bounds__(256) void k_qt_emit(Geom g, QtGeom q, QtBuffers qb)
{
    const int b = blockIdx.y;
    int l;
    unsigned chunk;
    if (!locate_chunk_block(q, g.nl, (int)blockIdx.x, l, chunk)) return;
    const int lane = threadIdx.x & 63;
    chunk += threadIdx.x >> 6;
    if ((long long)chunk >= q.nchunk[l]) return;
    const int *coff = qb.chunk_cnt + ((long long)b * q.chunk_stride + q.chunk_off[l] + chunk) * kChunkInts;
    CellNodes c[4];
    const unsigned code = qb.lane_code[((long long)b * q.chunk_stride + q.chunk_off[l] + chunk) * 64 + lane];
    const unsigned long long originators = __ballot(code != 0);
    if (originators == 0) return;         // nothing originates in this chunk (about half of the root square lies outside the plane)
    unpack_lane(code, chunk * 256u + (unsigned)lane * 4u, q.ltot[l], c);
    int ccx, ccy, lx, ly;
    morton_decode(chunk, ccx, ccy);
    morton_decode((unsigned)lane, lx, ly);
    const int cx0 = ccx * 16 + lx * 2, cy0 = ccy * 16 + ly * 2;
    int nsym = 0, nleaf = 0, ncoef = 0, n0 = 0;   // n0: level-0 leaves of this lane (a lane has at most one larger leaf, at cell 0)
#pragma unroll
    for (int i = 0; i < 4; i++) {
        nsym += c[i].nsym;
        if (c[i].leaf_lvl >= 0) { nleaf++; int s = q.cell << c[i].leaf_lvl; ncoef += s * s; }
        if (c[i].leaf_lvl == 0) n0++;
    }
    int sym_pos = coff[0], leaf_pos = coff[1], rank0 = 0, coef_pos = coff[2], rank_big = 0;
    if (originators != 1ull) {            // (lane 0 alone -- a chunk without edges, k_qt_count's short path -- starts at the chunk's offsets)
        // one scan for the three small counters (prefix sums < 1024 each), one for the coefficient offsets
        const int pk = nsym | nleaf << 10 | n0 << 20;
        const int pks = wave_incl_scan(pk, lane) - pk;
        sym_pos += pks & 1023;
        leaf_pos += (pks >> 10) & 1023;
        rank0 = (pks >> 20) & 1023;
        coef_pos += wave_incl_scan(ncoef, lane) - ncoef;
        const int big = c[0].leaf_lvl;                     // > 0 when this lane holds a leaf larger than a cell
        for (int k = 1; k < q.nsizes; k++) {
            unsigned long long m = __ballot(big == k);
            if (big == k) rank_big = __popcll(m & ((1ull << lane) - 1ull));
        }
    }

    unsigned char *st = qb.states + (long long)b * q.state_stride + q.state_off[l];
    int *leaves = qb.leaves + ((long long)b * q.leaf_stride + q.leaf_off[l]) * 4;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        for (int k = 0; k < c[i].nsym; k++) {
            if (sym_pos + k < q.state_cap[l]) st[sym_pos + k] = (unsigned char)((c[i].syms >> (2 * k)) & 3u);
            else *qb.overflow = 1;
        }
        sym_pos += c[i].nsym;
        if (c[i].leaf_lvl >= 0) {
            const int cx = cx0 + (i & 1), cy = cy0 + (i >> 1);
            const int size = q.cell << c[i].leaf_lvl;
            if (leaf_pos < q.leaf_cap[l] && (long long)coef_pos + (long long)size * size <= q.coeff_cap[l]) {
                reinterpret_cast<int4 *>(leaves)[leaf_pos] = make_int4(cx * q.cell, cy * q.cell, size, coef_pos);
                if (qb.work_count) {
                    const int k = c[i].leaf_lvl;       // size == bmin << k (the codec path always has cell == bmin)
                    long long pos = (long long)coff[4 + k] + (k == 0 ? rank0 : rank_big);
                    long long seg = (long long)b * q.work_stride[k] + q.work_off[l][k];
                    if (seg + pos < qb.work_cap[k])
                        qb.work[k][seg + pos] = pack_work(cx * q.cell, cy * q.cell, coef_pos);
                    else
                        *qb.overflow = 1;
                    if (k == 0) rank0++;
                }
            } else {
                *qb.overflow = 1;
            }
            leaf_pos++;
            coef_pos += size * size;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// The chunk-run kernels: a second count / scan / emit set for the shape class the codec uses (min block 4 == cell, at least 16 cells
// per root side, any max block; launch_qt_* choose, option "qt_chunks").  Same outputs bit for bit.  What differs:
//   * the count and emit grids cover the chunks whose origin lies inside the plane only, enumerated by chunk row and column per layer
//     and image (the Morton chunk index is the interleave of the two), and a wave takes a RUN of consecutive ones: layer, image and
//     base pointers are selected into scalar registers where the run enters a layer, not per chunk.  A run may cross the end of a
//     layer or of an image.  Neither kernel waits for the write acknowledgements of one chunk before it can read the next (gfx9 counts
//     loads and stores with one in-order counter): count stores a chunk's results behind the next chunk's loads, emit reads all
//     its run needs in front of the first chunk;
//   * a chunk outside the plane can originate one thing only, the absent-child symbol '10' at its first cell; the scan pass, which
//     walks every chunk record of a layer anyway, evaluates that per lane and stores the symbol at the scanned position;
//   * the per-chunk totals are popcounts of the wave's ballot masks on the scalar unit, not per-cell walks and butterfly sums.
// ------------------------------------------------------------------------------------------------
constexpr int kQtCell = 4;      // the only cell size of this set (chunk_edges' fast path: a chunk is one 64 x 64 bit-plane tile)

// One of three values by layer.  The operands are passed BY VALUE: a conditional expression between two members of a kernel argument
// is an lvalue, which compiles to a load through a selected address, and for a small argument to a scratch copy that takes the
// wave-uniform geometry out of the scalar registers.  (The per-layer arrays of Geom / QtGeom are indexed with the layer where a run
// enters one: loads that depend on the layer stay where they are needed, loads of all three entries are hoisted out of the chunk loop
// and cost more scalar registers than there are.)
template <class T> __device__ __forceinline__ T sel3(T a, T b, T c, int l) { return l == 0 ? a : l == 1 ? b : c; }

__device__ __forceinline__ unsigned part1by1(unsigned v)
{
    v &= 0x0000FFFFu;
    v = (v | (v << 8)) & 0x00FF00FFu;
    v = (v | (v << 4)) & 0x0F0F0F0Fu;
    v = (v | (v << 2)) & 0x33333333u;
    v = (v | (v << 1)) & 0x55555555u;
    return v;
}

struct QtLayer {      // what the chunk kernels need of one layer, wave-uniform
    int w, h, wpr, ncw, nch;      // plane, words per bit-plane row, cells per row / column that lie (partly) inside the plane
    int ncx, nin, ltot, ncell;
    long long bp_base, pyr_base, rec_base;      // of this layer of image b: bit-plane words, pyramid bytes, chunk records in front of it
};
// (called when a run enters another layer or image: the 64-bit products with the image index are formed here, not per chunk)
__device__ __forceinline__ QtLayer select_layer(const Geom &g, const QtGeom &q, const QtRuns &R, int l, int b)
{
    QtLayer L;
    L.w = g.w[l]; L.h = g.h[l]; L.wpr = g.wpr[l];
    L.ncw = (L.w + kQtCell - 1) / kQtCell; L.nch = (L.h + kQtCell - 1) / kQtCell;
    L.ncx = sel3(R.ncx0, R.ncx1, R.ncx2, l); L.nin = sel3(R.nin0, R.nin1, R.nin2, l);
    L.ltot = q.ltot[l]; L.ncell = q.ncell[l];
    L.bp_base = (long long)b * g.bpstride + g.bpoff[l];
    L.pyr_base = (long long)b * q.pyr_stride + q.pyr_off[l];
    L.rec_base = (long long)b * q.chunk_stride + q.chunk_off[l];
    return L;
}

struct QtCursor { int b, l, col, row, r; };      // image, layer, chunk column / row, index among the layer's in-plane chunks
__device__ __forceinline__ QtCursor cursor_at(const QtRuns &R, int gi)
{
    QtCursor c;
    c.b = gi / R.per_image;
    int r = gi - c.b * R.per_image;
    c.l = 0;
    if (r >= R.nin0) { r -= R.nin0; c.l = 1; if (r >= R.nin1) { r -= R.nin1; c.l = 2; } }
    const int ncx = sel3(R.ncx0, R.ncx1, R.ncx2, c.l);
    c.r = r; c.row = r / ncx; c.col = r - c.row * ncx;
    return c;
}
// -> true when the cursor moved to another layer (or image)
__device__ __forceinline__ bool cursor_next(QtCursor &c, const QtLayer &L, int nl)
{
    c.r++; c.col++;
    if (c.col == L.ncx) { c.col = 0; c.row++; }
    if (c.r < L.nin) return false;
    c.r = c.col = c.row = 0;
    if (++c.l == nl) { c.l = 0; c.b++; }
    return true;
}

__device__ __forceinline__ bool pyr_at(const unsigned char *__restrict__ pyr, int ncell, int lv, int cx, int cy)
{
    const int side = ncell >> lv;
    return pyr[lvl_off(ncell, lv) + (long long)(cy >> lv) * side + (cx >> lv)] != 0;
}

// The nodes of level >= 5 that originate at an in-plane chunk's first cell, largest first (wave-uniform): n_up split symbols '01', then
// either a leaf of level up_leaf >= 5 (the chunk lies inside it), or the chunk itself exists as a level-4 node (x4).
struct QtUpper { int n_up, up_leaf; bool x4; };
__device__ __forceinline__ QtUpper upper_walk(const QtGeom &q, const QtLayer &L, const unsigned char *__restrict__ pyr, unsigned chunk, int col, int row)
{
    QtUpper u;
    u.n_up = 0; u.up_leaf = -1; u.x4 = false;
    const int a = chunk == 0 ? L.ltot : min(4 + ((__ffs((int)chunk) - 1) >> 1), L.ltot);
    if ((kQtCell << 5) > q.bmax) {      // every node above a chunk splits (the codec's 4 .. 64 blocks): no pyramid
        u.n_up = a - 4; u.x4 = true;
        return u;
    }
    const int cx = col * 16, cy = row * 16;
    if (a < L.ltot) {      // the level-a node exists only if its parent splits (the parent's origin is inside the plane: the chunk's is)
        const int psize = kQtCell << (a + 1);
        if (!(psize > q.bmax || pyr_at(pyr, L.ncell, a + 1, cx, cy))) return u;
    }
    for (int lv = a; lv >= 5; lv--) {
        if ((kQtCell << lv) > q.bmax || pyr_at(pyr, L.ncell, lv, cx, cy)) u.n_up++;
        else { u.up_leaf = lv; return u; }
    }
    u.x4 = true;
    return u;
}

// bit t of the result = bit (t & ~3) resp. (t & ~15) of m: a node's flag, held at its first lane, spread over its lanes
__device__ __forceinline__ unsigned long long spread4(unsigned long long m) { m &= 0x1111111111111111ull; return (m << 4) - m; }
__device__ __forceinline__ unsigned long long spread16(unsigned long long m) { m &= 0x0001000100010001ull; return (m << 16) - m; }
__device__ __forceinline__ unsigned long long any4(unsigned long long m) { return spread4(m | (m >> 1) | (m >> 2) | (m >> 3)); }
__device__ __forceinline__ unsigned long long any16(unsigned long long m) { return spread16(m | (m >> 4) | (m >> 8) | (m >> 12)); }      // of an any4() mask
__device__ __forceinline__ bool bit_of(unsigned long long m, int lane) { return (m >> lane) & 1ull; }

__global__ __launch_bounds__(256) void k_qt_count_chunks(Geom g, QtGeom q, QtRuns R, const unsigned long long *__restrict__ edge_bits,
                                                         const unsigned char *__restrict__ pyr_all, int4 *__restrict__ chunk_rec,
                                                         unsigned short *__restrict__ lane_code, int *__restrict__ overflow)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) *overflow = 0;      // (set by the scan and emit passes, which run after this kernel has finished)
    const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const int lane = threadIdx.x & 63;
    const int gi0 = wave * R.run, gi1 = min(gi0 + R.run, R.total);
    if (gi0 >= gi1) return;
    int lx, ly;
    morton_decode((unsigned)lane, lx, ly);
    QtCursor c = cursor_at(R, gi0);
    QtLayer L = select_layer(g, q, R, c.l, c.b);
    // What a chunk leaves for the later passes.  Its stores are issued one iteration late, behind the loads of the next chunk: gfx9
    // counts loads and stores with one in-order counter, so a load issued after a chunk's stores can only be waited for together
    // with their write acknowledgements -- once per chunk.  Behind the loads, a fixed number of stores (every lane stores the
    // wave-uniform record: a store by lane 0 alone would sit behind a branch) leaves the wait for the loads exact.
    struct Res { long long rec_i; unsigned code; int4 r0, r1, r2; };
    auto put = [&](const Res &r) __attribute__((always_inline)) {
        lane_code[r.rec_i * 64 + lane] = (unsigned short)r.code;
        chunk_rec[3 * r.rec_i] = r.r0; chunk_rec[3 * r.rec_i + 1] = r.r1; chunk_rec[3 * r.rec_i + 2] = r.r2;
    };
    // this lane's four cells are the 8 x 8-pixel square at rows 8 * ly .., bits 8 * lx .. of the chunk's tile (64 contiguous words).
    // All eight words whatever the plane's height: the bit-plane's rows are padded to whole tiles, and the rows past the plane are
    // masked afterwards.
    auto request = [&](unsigned long long (&raw)[8]) __attribute__((always_inline)) {
        const unsigned long long *tile = edge_bits + L.bp_base + (unsigned)(c.row * L.wpr + c.col) * 64u + 8 * ly;      // (at most 14 levels: fewer than 2^20 tiles)
#pragma unroll
        for (int r = 0; r < 8; r++) raw[r] = tile[r];
    };
    const unsigned long long big1 = (kQtCell << 1) > q.bmax ? ~0ull : 0ull, big2 = (kQtCell << 2) > q.bmax ? ~0ull : 0ull, big3 = (kQtCell << 3) > q.bmax ? ~0ull : 0ull;      // levels that split whatever they hold
    auto work = [&](unsigned long long (&raw)[8]) __attribute__((always_inline)) {
        const unsigned chunk = part1by1((unsigned)c.col) | (part1by1((unsigned)c.row) << 1);
        const long long rec_i = L.rec_base + chunk;
        if (c.row * 64 + 64 > L.h) {      // the plane ends inside this chunk row
            const int rows = L.h - c.row * 64 - 8 * ly;
#pragma unroll
            for (int r = 0; r < 8; r++) raw[r] = r < rows ? raw[r] : 0ull;
        }
        unsigned long long top = raw[0] | raw[1] | raw[2] | raw[3], bot = raw[4] | raw[5] | raw[6] | raw[7];
        const unsigned t8 = (unsigned)(top >> (8 * lx)) & 0xFFu, b8 = (unsigned)(bot >> (8 * lx)) & 0xFFu;
        const unsigned e0 = ((t8 & 0x0Fu) ? 1u : 0u) | ((t8 & 0xF0u) ? 2u : 0u) | ((b8 & 0x0Fu) ? 4u : 0u) | ((b8 & 0xF0u) ? 8u : 0u);
        const unsigned long long E1 = __ballot(e0 != 0);
        const QtUpper u = upper_walk(q, L, pyr_all + L.pyr_base, chunk, c.col, c.row);
        const bool top_exists = u.x4 || u.up_leaf >= 0 || u.n_up > 0;
        const bool S4 = (kQtCell << 4) > q.bmax || E1 != 0;
        int nsym = u.n_up + (u.up_leaf >= 0 ? 1 : 0) + (u.x4 ? 1 : 0);
        int lf[5] = { 0, 0, 0, 0, 0 };      // leaves of levels 0 .. 4
        unsigned code = 0;
        if (!(u.x4 && S4)) {
            // nothing below the chunk node: it is a leaf, or lies inside a larger one, or does not exist.  Every chunk of a flat region.
            lf[4] = u.x4 ? 1 : 0;
            if (lane == 0 && top_exists) code = 1u | ((unsigned)u.n_up << 2);
        } else {
            // masks over the lanes (= level-1 nodes); a level-2 / 3 node's bit is repeated over its 4 / 16 lanes
            const int cx0 = c.col * 16 + 2 * lx, cy0 = c.row * 16 + 2 * ly;
            const bool interior = c.col * 16 + 16 <= L.ncw && c.row * 16 + 16 <= L.nch;
            unsigned long long inx0 = ~0ull, inx1 = ~0ull, iny0 = ~0ull, iny1 = ~0ull;
            if (!interior) {
                inx0 = __ballot(cx0 < L.ncw); inx1 = __ballot(cx0 + 1 < L.ncw);
                iny0 = __ballot(cy0 < L.nch); iny1 = __ballot(cy0 + 1 < L.nch);
            }
            const unsigned long long IN1 = inx0 & iny0, IN2 = spread4(IN1), IN3 = spread16(IN1);
            const unsigned long long E2 = any4(E1), E3 = any16(E2);
            const unsigned long long S1 = E1 | big1, S2 = E2 | big2, S3 = E3 | big3;
            const unsigned long long X3 = ~0ull, X2 = X3 & IN3 & S3, X1 = X2 & IN2 & S2, X0 = X1 & IN1 & S1;      // the nodes that exist
            const unsigned long long F2 = 0x1111111111111111ull, F3 = 0x0001000100010001ull;
            lf[3] = __popcll(X3 & IN3 & ~S3 & F3);
            lf[2] = __popcll(X2 & IN2 & ~S2 & F2);
            lf[1] = __popcll(X1 & IN1 & ~S1);
            lf[0] = __popcll(X0 & inx0 & iny0) + __popcll(X0 & inx1 & iny0) + __popcll(X0 & inx0 & iny1) + __popcll(X0 & inx1 & iny1);
            nsym += 4 + __popcll(X2 & F2) + __popcll(X1) + 4 * __popcll(X0);
            // the lane's 12-bit code (pack_lane): cell 0 originates the nodes of levels a .. 0, cells 1 .. 3 their own
            const bool s1 = bit_of(S1, lane), s2 = bit_of(S2, lane), s3 = bit_of(S3, lane), in1 = bit_of(IN1, lane);
            const int c1 = s1 ? 1 : 0, c2 = s2 ? 1 + c1 : 0, c3 = s3 ? 1 + c2 : 0;
            const int a = 1 + ((__ffs(lane | 64) - 1) >> 1);      // lane > 0: 1 .. 3
            bool ex = a == 1 ? bit_of(X1, lane) : a == 2 ? bit_of(X2, lane) : true;
            int kk = a == 1 ? c1 : a == 2 ? c2 : c3;
            if (lane == 0) { ex = true; kk = u.n_up + 1 + c3; }
            code = !ex ? 0u : !in1 ? 3u : (1u | ((unsigned)kk << 2));
            if (bit_of(X0, lane)) {
                const bool x1 = cx0 + 1 < L.ncw, y1 = cy0 + 1 < L.nch;
                code |= (x1 ? 1u : 3u) << 6 | (y1 ? 1u : 3u) << 8 | (x1 && y1 ? 1u : 3u) << 10;
            }
        }
        Res res;
        res.rec_i = rec_i; res.code = code;
        const int nleaf = lf[0] + lf[1] + lf[2] + lf[3] + lf[4] + (u.up_leaf >= 0 ? 1 : 0);
        int ncoef = 0;
#pragma unroll
        for (int k = 0; k < 5; k++) ncoef += lf[k] * (kQtCell << k) * (kQtCell << k);
        if (u.up_leaf >= 0) ncoef += (kQtCell << u.up_leaf) * (kQtCell << u.up_leaf);
        static_assert(kMaxSizes == 8, "a chunk record holds eight per-size counts");
        res.r0 = make_int4(nsym, nleaf, ncoef, 0);
        res.r1 = make_int4(lf[0], lf[1], lf[2], lf[3]);
        res.r2 = make_int4(lf[4], u.up_leaf == 5 ? 1 : 0, u.up_leaf == 6 ? 1 : 0, u.up_leaf == 7 ? 1 : 0);
        return res;
    };
    unsigned long long raw[8];
    request(raw);
    Res res = work(raw);
    for (int gi = gi0 + 1; gi < gi1; gi++) {
        if (cursor_next(c, L, g.nl)) L = select_layer(g, q, R, c.l, c.b);
        request(raw);
        put(res);
        res = work(raw);
    }
    put(res);
}

// The scan pass of the chunk-run set: as k_qt_scan, but the records of the chunks outside the plane are not in memory -- the thread that
// would have read one works it out (at most the one symbol '10', when the parent of the largest node originating at the chunk's first
// cell is inside the plane and splits) and stores that symbol at its scanned position.  Same rounds, same barriers.
template <int kScanThreads>
__global__ __launch_bounds__(kScanThreads) void k_qt_scan_chunks(Geom g, QtGeom q, QtRuns R, int4 *__restrict__ rec_all, const unsigned char *__restrict__ pyr_all,
                                                                 unsigned char *__restrict__ states, long long *__restrict__ counts,
                                                                 int *__restrict__ work_count, int *__restrict__ overflow)
{
    constexpr int NQ = 3 + kMaxSizes;
    __shared__ int s_w[NQ][kScanThreads / 64];
    __shared__ int carry[NQ];
    const int tid = threadIdx.x, l = blockIdx.x, b = blockIdx.y;
    const int lane = tid & 63, wv = tid >> 6;
    int4 *rec = rec_all + ((long long)b * q.chunk_stride + q.chunk_off[l]) * 3;
    const unsigned char *pyr = pyr_all + (long long)b * q.pyr_stride + q.pyr_off[l];
    unsigned char *st = states + (long long)b * q.state_stride + q.state_off[l];
    const int n = q.nchunk[l], ncell = q.ncell[l], ncx = sel3(R.ncx0, R.ncx1, R.ncx2, l), ncy = sel3(R.ncy0, R.ncy1, R.ncy2, l);
    const long long state_cap = q.state_cap[l];
    const int nq = 3 + q.nsizes;
    if (tid < NQ) carry[tid] = 0;
    __syncthreads();
    static_assert(kChunkInts == 12 && NQ == 11, "a chunk record is three int4: (nsym, nleaf, ncoef, pad), leaves per size 0..3, 4..7");
    for (int start = 0; start < n; start += kScanThreads) {
        const int i = start + tid;
        int4 r0 = make_int4(0, 0, 0, 0), r1 = r0, r2 = r0;
        bool inside = false;
        if (i < n) {
            int ccx, ccy;
            morton_decode((unsigned)i, ccx, ccy);
            inside = ccx < ncx && ccy < ncy;
            if (inside) { r0 = rec[3 * i]; r1 = rec[3 * i + 1]; r2 = rec[3 * i + 2]; }
            else {
                // (i > 0: chunk 0 is inside.)  The largest node originating here has level a < ltot; its parent has level a + 1 >= 5
                const int p = 5 + ((__ffs(i) - 1) >> 1), sh = p - 4;
                const int pcx = (ccx >> sh) << sh, pcy = (ccy >> sh) << sh;
                if (pcx < ncx && pcy < ncy && ((kQtCell << p) > q.bmax || pyr_at(pyr, ncell, p, pcx * 16, pcy * 16))) r0.x = 1;
            }
        }
        int v[NQ] = { r0.x, r0.y, r0.z, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w }, inc[NQ];
#pragma unroll
        for (int c = 0; c < NQ; c++) {
            if (c >= nq) v[c] = 0;
            inc[c] = wave_incl_scan(v[c], lane);
            if (lane == 63) s_w[c][wv] = inc[c];
        }
        __syncthreads();
        int o[NQ];
#pragma unroll
        for (int c = 0; c < NQ; c++) {
            int p = carry[c];
            for (int k = 0; k < wv; k++) p += s_w[c][k];
            o[c] = p + inc[c] - v[c];
        }
        if (inside) {
            rec[3 * i] = make_int4(o[0], o[1], o[2], r0.w);
            rec[3 * i + 1] = make_int4(o[3], o[4], o[5], o[6]);
            rec[3 * i + 2] = make_int4(o[7], o[8], o[9], o[10]);
        } else if (r0.x) {
            if (o[0] < state_cap) st[o[0]] = (unsigned char)2;      // '10'
            else *overflow = 1;
        }
        __syncthreads();
        if (tid < NQ) {
            int t = 0;
            for (int k = 0; k < kScanThreads / 64; k++) t += s_w[tid][k];
            carry[tid] += t;
        }
        __syncthreads();
    }
    if (tid == 0) {
        long long *o = counts + ((long long)b * 3 + l) * 4;
        o[0] = carry[2];      // n_coeffs
        o[1] = carry[1];      // n_leaves
        o[2] = carry[0];      // n_states
        o[3] = q.root[l];
    }
    if (work_count && tid < kMaxSizes) work_count[((long long)b * 3 + l) * kMaxSizes + tid] = tid < q.nsizes ? carry[3 + tid] : 0;
}

// The emit pass of the chunk-run set: runs of in-plane chunks as in k_qt_count_chunks.
//   * Everything the run reads -- its chunks' lane codes and records -- is requested in front of the first chunk, and kept in
//     registers (the codes two to a register, shifted down chunk by chunk; the records one value per lane, fetched with v_readlane).
//     gfx9 counts loads and stores with one in-order counter: a load issued after a chunk's stores could only be waited for
//     together with the write acknowledgements of those stores, chunk after chunk.
//   * A chunk's symbols and leaf table are put together in LDS (wave-private: no workgroup barrier) and written out with
//     consecutive lanes on consecutive elements.  Written from the lanes that found them, a leaf store touches up to 64 different
//     64-byte lines with 16 bytes each, and a symbol store as many with one byte each: the pass was bound by write requests.
//     The level-0 work list is compacted from the staged leaf table (ballot ranks) on the way out; the entries of the sizes above
//     the cell, few per chunk, are placed size by size from the lanes that hold them (wave-uniform k: list, segment and capacity
//     are scalars).
constexpr int kQtMaxRun = 16;                // chunks per wave at most (QtRuns::run)
constexpr int kQtStageStates = 512;          // symbols a chunk can originate: 341 inside it, plus the levels above it at its first cell

__device__ __forceinline__ void wave_lds_sync()      // LDS operations of one wave execute in order; this keeps the compiler from reordering them
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(256) void k_qt_emit_chunks(Geom g, QtGeom q, QtRuns R, QtBuffers qb, const int *__restrict__ chunk_rec,
                                                        const unsigned short *__restrict__ lane_code)
{
    __shared__ int4 s_leaf_all[4][kQtChunk];
    __shared__ unsigned char s_state_all[4][kQtStageStates];
    const int wv = threadIdx.x >> 6;
    int4 *s_leaf = s_leaf_all[wv];
    unsigned char *s_state = s_state_all[wv];
    const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + wv));
    const int lane = threadIdx.x & 63;
    const int gi0 = wave * R.run, n = min(R.run, R.total - gi0);
    if (n <= 0) return;
    int lx, ly;
    morton_decode((unsigned)lane, lx, ly);
    const QtCursor c0 = cursor_at(R, gi0);
    const QtLayer L0 = select_layer(g, q, R, c0.l, c0.b);

    // ---- everything the run reads
    unsigned pk[kQtMaxRun / 2];                // lane codes of chunks 2j (low half) and 2j + 1 of the run
    long long my_rec = 0;                      // record index of run chunk lane >> 2
    {
        QtCursor c = c0;
        QtLayer L = L0;
        unsigned code[kQtMaxRun];
#pragma unroll
        for (int i = 0; i < kQtMaxRun; i++) {      // (past the run's end: its last chunk again)
            const unsigned chunk = part1by1((unsigned)c.col) | (part1by1((unsigned)c.row) << 1);
            const long long rec_i = L.rec_base + chunk;
            code[i] = lane_code[rec_i * 64 + lane];
            if ((lane >> 2) == i) my_rec = rec_i;
            if (i + 1 < n && cursor_next(c, L, g.nl)) L = select_layer(g, q, R, c.l, c.b);
        }
#pragma unroll
        for (int j = 0; j < kQtMaxRun / 2; j++) pk[j] = code[2 * j] | (code[2 * j + 1] << 16);
    }
    const int *my = chunk_rec + my_rec * kChunkInts + (lane & 3);
    const int v_pos = my[0], v_szlo = my[4], v_szhi = my[8];      // of run chunk i: lanes 4i .. 4i + 2 symbol / leaf / coefficient offset; list offsets of sizes 0 .. 3, 4 .. 7

    // the layer's output layout, selected when the run enters the layer
    struct Out { long long state_cap, leaf_cap, coeff_cap, seg0; unsigned char *st; int4 *leaves; };
    auto select_out = [&](int l, int b) {
        Out o;
        o.state_cap = q.state_cap[l]; o.leaf_cap = q.leaf_cap[l]; o.coeff_cap = q.coeff_cap[l];
        o.st = qb.states + (long long)b * q.state_stride + q.state_off[l];
        o.leaves = reinterpret_cast<int4 *>(qb.leaves) + ((long long)b * q.leaf_stride + q.leaf_off[l]);
        o.seg0 = (long long)b * q.work_stride[0] + q.work_off[l][0];
        return o;
    };
    QtCursor c = c0;
    QtLayer L = L0;
    Out O = select_out(c.l, c.b);
    const bool lists = qb.work_count != nullptr;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    for (int i = 0; i < n; i++) {
        const unsigned code = pk[0] & 0xFFFFu;
#pragma unroll
        for (int j = 0; j < kQtMaxRun / 2 - 1; j++) pk[j] = (pk[j] >> 16) | (pk[j + 1] << 16);
        pk[kQtMaxRun / 2 - 1] >>= 16;
        const unsigned long long originators = __ballot(code != 0);
        if (originators != 0) {
            const unsigned chunk = part1by1((unsigned)c.col) | (part1by1((unsigned)c.row) << 1);
            const int sym_base = __builtin_amdgcn_readlane(v_pos, 4 * i), leaf_base = __builtin_amdgcn_readlane(v_pos, 4 * i + 1);
            const int coef_base = __builtin_amdgcn_readlane(v_pos, 4 * i + 2), szoff0 = __builtin_amdgcn_readlane(v_szlo, 4 * i);
            const long long state_cap = O.state_cap, leaf_cap = O.leaf_cap, coeff_cap = O.coeff_cap;
            unsigned char *st = O.st;
            int4 *leaves = O.leaves;
            const long long seg0 = O.seg0 + szoff0;
            // cell 0: k0 split symbols then a leaf (type 1), or one absent child (type 3); cells 1 .. 3: 0 none, 1 leaf, 3 absent child
            const unsigned t = code & 3u;
            const int k0 = (int)((code >> 2) & 15u);
            const unsigned ci[3] = { (code >> 6) & 3u, (code >> 8) & 3u, (code >> 10) & 3u };
            const int a_chunk = chunk == 0 ? L.ltot : min(4 + ((__ffs((int)chunk) - 1) >> 1), L.ltot);
            const int a = lane == 0 ? a_chunk : 1 + ((__ffs(lane) - 1) >> 1);      // level of the largest node originating at the lane's cell 0
            const int lvl0 = t == 1u ? a - k0 : -1;
            const int size0 = lvl0 >= 0 ? kQtCell << lvl0 : 0;
            const int nsym0 = t == 0u ? 0 : t == 3u ? 1 : k0 + (t == 1u ? 1 : 0);
            const int x0 = (c.col * 16 + 2 * lx) * kQtCell, y0 = (c.row * 16 + 2 * ly) * kQtCell;
            bool fit0 = false;
            int coef0 = coef_base;
            if (originators == 1ull && __ballot((code >> 6) != 0u) == 0ull) {      // (wave-uniform: the other branch holds DPP scans and the LDS staging)
                // lane 0's first cell alone (a chunk without a split): written from that lane
                if (lane == 0) {
                    for (int k = 0; k < nsym0; k++) {
                        if (sym_base + k < state_cap) st[sym_base + k] = (unsigned char)(t == 3u ? 2 : k < k0 ? 1 : 0); else *qb.overflow = 1;
                    }
                    if (lvl0 >= 0) {
                        fit0 = leaf_base < leaf_cap && (long long)coef_base + (long long)size0 * size0 <= coeff_cap;
                        if (fit0) leaves[leaf_base] = make_int4(x0, y0, size0, coef_base); else *qb.overflow = 1;
                        if (fit0 && lists && lvl0 == 0) {
                            if (seg0 < qb.work_cap[0]) qb.work[0][seg0] = pack_work(x0, y0, coef_base); else *qb.overflow = 1;
                        }
                    }
                }
            } else {
                const int nl13 = (ci[0] == 1u ? 1 : 0) + (ci[1] == 1u ? 1 : 0) + (ci[2] == 1u ? 1 : 0);
                const int nsym = nsym0 + (ci[0] ? 1 : 0) + (ci[1] ? 1 : 0) + (ci[2] ? 1 : 0);
                const int nleaf = (lvl0 >= 0 ? 1 : 0) + nl13;
                const int ncoef = size0 * size0 + nl13 * kQtCell * kQtCell;
                // one scan for the two small counters (prefix sums < 1024 each), one for the coefficient offsets
                const int pk2 = nsym | nleaf << 10;
                const int inc2 = wave_incl_scan(pk2, lane), inc_c = wave_incl_scan(ncoef, lane);
                const int tot2 = __builtin_amdgcn_readlane(inc2, 63);
                const int tsym = tot2 & 1023, tleaf = (tot2 >> 10) & 1023;
                int lsym = (inc2 - pk2) & 1023, lleaf = ((inc2 - pk2) >> 10) & 1023, coef_pos = coef_base + inc_c - ncoef;
                coef0 = coef_pos;
                // stage: symbols and leaf table of the chunk, in order
                for (int k = 0; k < nsym0; k++) s_state[lsym + k] = (unsigned char)(t == 3u ? 2 : k < k0 ? 1 : 0);
                lsym += nsym0;
                if (lvl0 >= 0) {
                    fit0 = leaf_base + lleaf < leaf_cap && (long long)coef_pos + (long long)size0 * size0 <= coeff_cap;
                    s_leaf[lleaf++] = make_int4(x0, y0, size0, coef_pos);
                    coef_pos += size0 * size0;
                }
#pragma unroll
                for (int j = 0; j < 3; j++)
                    if (ci[j]) {
                        s_state[lsym++] = (unsigned char)(ci[j] == 1u ? 0 : ci[j] == 2u ? 1 : 2);
                        if (ci[j] == 1u) {
                            s_leaf[lleaf++] = make_int4(x0 + ((j + 1) & 1) * kQtCell, y0 + ((j + 1) >> 1) * kQtCell, kQtCell, coef_pos);
                            coef_pos += kQtCell * kQtCell;
                        }
                    }
                wave_lds_sync();
                // write out: consecutive lanes, consecutive elements
                for (int j = lane; j < tsym; j += 64) {
                    if (sym_base + j < state_cap) st[sym_base + j] = s_state[j]; else *qb.overflow = 1;
                }
                int run0 = 0;      // level-0 leaves of the chunk written so far
                for (int j0 = 0; j0 < tleaf; j0 += 64) {
                    const int j = j0 + lane;
                    const bool valid = j < tleaf;
                    int4 e = make_int4(0, 0, 0, 0);
                    if (valid) e = s_leaf[j];
                    const bool fit = valid && leaf_base + j < leaf_cap && (long long)e.w + (long long)e.z * e.z <= coeff_cap;
                    if (fit) leaves[leaf_base + j] = e;
                    else if (valid) *qb.overflow = 1;
                    if (lists) {
                        const bool is0 = valid && e.z == kQtCell;
                        const unsigned long long m0 = __ballot(is0);
                        if (is0 && fit) {
                            const long long pos = seg0 + run0 + __popcll(m0 & lt_mask);
                            if (pos < qb.work_cap[0]) qb.work[0][pos] = pack_work(e.x, e.y, e.w); else *qb.overflow = 1;
                        }
                        run0 += __popcll(m0);
                    }
                }
                wave_lds_sync();
            }
            if (lists && __ballot(lvl0 > 0) != 0) {
                for (int k = 1; k < q.nsizes; k++) {
                    const unsigned long long mk = __ballot(lvl0 == k);
                    if (mk == 0) continue;
                    const int szoff = __builtin_amdgcn_readlane(k < 4 ? v_szlo : v_szhi, 4 * i + (k & 3));
                    const long long seg = (long long)c.b * q.work_stride[k] + q.work_off[c.l][k] + szoff;
                    if (lvl0 == k && fit0) {
                        const long long pos = seg + __popcll(mk & lt_mask);
                        if (pos < qb.work_cap[k]) qb.work[k][pos] = pack_work(x0, y0, coef0); else *qb.overflow = 1;
                    }
                }
            }
        }
        if (i + 1 < n && cursor_next(c, L, g.nl)) { L = select_layer(g, q, R, c.l, c.b); O = select_out(c.l, c.b); }
    }
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
static int chunk_blocks(const Geom &g, const QtGeom &q)      // workgroups of 4 chunks (one wave each), all layers of one image
{
    int n = 0;
    for (int l = 0; l < g.nl; l++) n += (q.nchunk[l] + 3) / 4;
    return n;
}

bool qt_needs_upper(const Geom &g, const QtGeom &q)
{
    // only the levels above a chunk (>= 5) live in global memory, and only when a node of that size can still be a leaf
    for (int l = 0; l < g.nl; l++) if (q.ltot[l] > 4 && (q.cell << 5) <= q.bmax) return true;
    return false;
}

// The chunk-run kernels serve min block 4 == cell with at least one whole chunk per layer; everything else takes the general set.
bool qt_chunk_runs(const Geom &g, const QtGeom &q, const Tuning &t, QtRuns &R)
{
    memset(&R, 0, sizeof R);
    if (!t.qt_chunks || q.cell != kQtCell || q.bmin != kQtCell || g.nl < 1 || g.nl > 3) return false;
    long long per_image = 0;
    int ncx[3] = { 0, 0, 0 }, ncy[3] = { 0, 0, 0 };
    for (int l = 0; l < g.nl; l++) {
        if (q.ltot[l] < 4) return false;
        ncx[l] = (g.w[l] + 63) / 64; ncy[l] = (g.h[l] + 63) / 64;
        per_image += (long long)ncx[l] * ncy[l];
    }
    R.ncx0 = ncx[0]; R.ncx1 = ncx[1]; R.ncx2 = ncx[2];
    R.ncy0 = ncy[0]; R.ncy1 = ncy[1]; R.ncy2 = ncy[2];
    R.nin0 = ncx[0] * ncy[0]; R.nin1 = ncx[1] * ncy[1]; R.nin2 = ncx[2] * ncy[2];
    const long long total = per_image * g.B;
    if (total >= (1ll << 30)) return false;
    R.per_image = (int)per_image; R.total = (int)total;
    // a few waves per SIMD deep for a large call (1024 SIMDs), one chunk per wave while that does not yet fill the chip
    R.run = (int)std::min<long long>(kQtMaxRun, std::max<long long>(1, (total + 4095) / 4096));
    if (t.qt_chunk_run > 0) R.run = std::min(t.qt_chunk_run, kQtMaxRun);
    return true;
}
static unsigned run_blocks(const QtRuns &R) { return (unsigned)(((R.total + R.run - 1) / R.run + 3) / 4); }

void launch_qt_cells(hipStream_t st, const Geom &g, const QtGeom &q, const unsigned long long *edge_bits, const QtBuffers &qb)
{
    if (qt_needs_upper(g, q)) hipLaunchKernelGGL(k_qt_upper, dim3(chunk_blocks(g, q), g.B), dim3(256), 0, st, g, q, edge_bits, qb.pyr);
}
// runs: what qt_chunk_runs() gave for this call, or null for the general kernels -- decided once per call (api_encode.hip run_quadtree)
void launch_qt_count(hipStream_t st, const Geom &g, const QtGeom &q, const QtBuffers &qb, const QtRuns *runs)
{
    if (runs)
        hipLaunchKernelGGL(k_qt_count_chunks, dim3(run_blocks(*runs)), dim3(256), 0, st, g, q, *runs, qb.edge_bits, qb.pyr, reinterpret_cast<int4 *>(qb.chunk_cnt),
                           qb.lane_code, qb.overflow);
    else
        hipLaunchKernelGGL(k_qt_count, dim3(chunk_blocks(g, q), g.B), dim3(256), 0, st, g, q, qb.edge_bits, qb.pyr, qb.chunk_cnt, qb.lane_code);
}
void launch_qt_scan(hipStream_t st, const Geom &g, const QtGeom &q, const QtBuffers &qb, const QtRuns *runs)
{
    if (runs) {
        int4 *rec = reinterpret_cast<int4 *>(qb.chunk_cnt);
        if (g.B <= 4) hipLaunchKernelGGL(k_qt_scan_chunks<1024>, dim3(g.nl, g.B), dim3(1024), 0, st, g, q, *runs, rec, qb.pyr, qb.states, qb.counts, qb.work_count, qb.overflow);
        else hipLaunchKernelGGL(k_qt_scan_chunks<256>, dim3(g.nl, g.B), dim3(256), 0, st, g, q, *runs, rec, qb.pyr, qb.states, qb.counts, qb.work_count, qb.overflow);
        return;
    }
    if (g.B <= 4) hipLaunchKernelGGL(k_qt_scan<1024>, dim3(g.nl, g.B), dim3(1024), 0, st, g, q, qb.chunk_cnt, qb.counts, qb.work_count);
    else hipLaunchKernelGGL(k_qt_scan<256>, dim3(g.nl, g.B), dim3(256), 0, st, g, q, qb.chunk_cnt, qb.counts, qb.work_count);
}
void launch_qt_emit(hipStream_t st, const Geom &g, const QtGeom &q, const QtBuffers &qb, const QtRuns *runs)
{
    if (runs) hipLaunchKernelGGL(k_qt_emit_chunks, dim3(run_blocks(*runs)), dim3(256), 0, st, g, q, *runs, qb, qb.chunk_cnt, qb.lane_code);
    else hipLaunchKernelGGL(k_qt_emit, dim3(chunk_blocks(g, q), g.B), dim3(256), 0, st, g, q, qb);
}

}  // namespace aej
