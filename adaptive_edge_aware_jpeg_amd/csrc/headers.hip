// headers.hip -- the quadtree headers of .ajpg layers decoded on the device: packed 2-bit state symbols -> the leaf table and counts that
// aej_decode_batch reads (Jpeg.decompress's host work, jpeg.py:285-296: Jpeg._decode_leaf_sizes, then aej_leaf_positions_host).
//
// One wave per layer, every layer of the batch in one launch; inside a layer both walks are serial (lane 0), as the host's are.  Neither
// walk keeps a stack of nodes: a stack of quadtree siblings holds at most four nodes per level, all of the level's size, so the walk keeps
// a 3-bit count per level (packed into 64-bit registers) and a mask of the levels with nodes left -- the top of the stack is the deepest
// such level.  Same pops, pushes and order as the host's stack, so the same result on ANY symbol string, well-formed or not.
#include "aej_launch.h"

namespace aej {


namespace {

// status values (include/aej.h, AEJ_HEADER_*)
enum { kOk = 0, kTooManyLeaves = 1, kBadSize = 2, kNoTiling = 3, kCoeffCount = 4, kBadArg = 5 };

// 3-bit counts, levels 0..20 in c[0], 21..41 in c[1]
struct Levels {
    unsigned long long c0 = 0, c1 = 0, nz = 0;
    __device__ int get(int l) const { return l < 21 ? (int)((c0 >> (3 * l)) & 7) : (int)((c1 >> (3 * (l - 21))) & 7); }
    __device__ void set(int l, int v)
    {
        if (l < 21) c0 = (c0 & ~(7ull << (3 * l))) | ((unsigned long long)v << (3 * l));
        else c1 = (c1 & ~(7ull << (3 * (l - 21)))) | ((unsigned long long)v << (3 * (l - 21)));
        nz = v ? nz | (1ull << l) : nz & ~(1ull << l);
    }
    __device__ int top() const { return 63 - __clzll((long long)nz); }
};

__device__ __forceinline__ int ilog2_exact(long long s) { return 63 - __clzll(s); }

__global__ __launch_bounds__(64) void headers_kernel(const unsigned char *__restrict__ states, const long long *__restrict__ desc,
                                                     const long long *__restrict__ inflated, int nlayers, HdrGeom g,
                                                     unsigned char *__restrict__ codes, int *__restrict__ leaves, long long *__restrict__ counts,
                                                     int *__restrict__ status)
{
    const int i = blockIdx.x;
    if (i >= nlayers || threadIdx.x != 0) return;
    const int b = i / 3, l = i % 3;
    const long long soff = desc[3 * i], ns = desc[3 * i + 1], root = desc[3 * i + 2];
    const long long lbase = (long long)b * g.leaf_stride + g.leaf_off[l];
    const long long span = g.leaf_span[l];
    unsigned char *code = codes + lbase;                  // one log2(size) byte per leaf, 16-byte aligned (leaf_off, leaf_stride)
    int st = kOk;
    long long nleaf = 0, ncoef = 0;
    if (soff < 0 || ns < 0 || root < 0) st = kBadArg;

    // ---- walk 1: symbols -> leaf sizes (Jpeg._decode_leaf_sizes): 0 = leaf, 1 = four children, anything else = no node.
    // Level t holds nodes of size root >> t; from level z on the size is 0 and one (unbounded) counter holds them all.
    int z = 0;
    while (z < 40 && (root >> z) > 0) z++;
    Levels lv;
    long long zc = 0;
    auto push = [&](int t, int k) {
        if (t >= z) { zc += k; lv.nz |= 1ull << z; }
        else lv.set(t, k);
    };
    if (st == kOk) push(0, 1);
    const unsigned char *sp = states + soff;
    const long long nbytes = (ns + 3) / 4;
    unsigned long long sbuf = 0, pk = 0;
    int sleft = 0;
    long long si = 0;
    while (st == kOk && lv.nz && si < ns) {
        const int t = lv.top();
        const long long size = t >= z ? 0 : root >> t;
        if (t >= z) { if (--zc == 0) lv.nz &= ~(1ull << z); }
        else lv.set(t, lv.get(t) - 1);
        if (sleft == 0) {                                   // the next 32 symbols, first symbol in the top bits
            const long long bi = si >> 2;
            sbuf = 0;
            for (int j = 0; j < 8; j++) sbuf |= (unsigned long long)(bi + j < nbytes ? sp[bi + j] : 0) << (56 - 8 * j);
            sleft = 32;
        }
        const int s = (int)(sbuf >> 62);
        sbuf <<= 2;
        sleft--;
        si++;
        if (s == 0) {
            if (nleaf >= span) { st = kTooManyLeaves; break; }
            if (size < g.bmin || size > g.bmax) { st = kBadSize; break; }
            if (size & (size - 1)) { st = kNoTiling; break; }       // no node of the position walk has this size
            pk |= (unsigned long long)ilog2_exact(size) << (8 * (nleaf & 7));
            nleaf++;
            ncoef += size * size;
            if ((nleaf & 7) == 0) { *reinterpret_cast<unsigned long long *>(code + nleaf - 8) = pk; pk = 0; }
        } else if (s == 1) {
            push(t + 1 < z ? t + 1 : z, 4);
        }
    }
    if (st == kOk && (nleaf & 7)) *reinterpret_cast<unsigned long long *>(code + (nleaf & ~7LL)) = pk;

    // ---- walk 2: leaf positions (aej_leaf_positions_host): children pushed (x+h, y+h), (x, y+h), (x+h, y), (x, y), popped in reverse;
    // the node popped with count c left on its level is child 4 - c.  Its position differs from the last popped node's only below 2 * size.
    if (st == kOk) {
        const int P = g.proot[l], H = g.h[l], W = g.w[l];
        Levels pv;
        pv.set(0, 1);
        int x = 0, y = 0;
        long long li = 0, coff = 0;
        const long long nchunk = (span + 15) / 16;
        long long chunk = 0;
        uint4 cur = *reinterpret_cast<const uint4 *>(code), nxt = cur;
        if (nchunk > 1) nxt = *reinterpret_cast<const uint4 *>(code + 16);
        int4 *out = reinterpret_cast<int4 *>(leaves) + lbase;
        while (pv.nz) {
            const int t = pv.top();
            const int c = pv.get(t);
            pv.set(t, c - 1);
            const int s = P >> t;
            if (t > 0) {
                const int child = 4 - c;
                x = (x & ~(2 * s - 1)) | ((child & 1) ? s : 0);
                y = (y & ~(2 * s - 1)) | ((child >> 1) ? s : 0);
            }
            if (x >= W || y >= H) continue;
            if (li >= nleaf) { st = kNoTiling; break; }
            if ((li >> 4) != chunk) {                      // codes come 16 at a time, the next 16 already on their way
                chunk = li >> 4;
                cur = nxt;
                if (chunk + 1 < nchunk) nxt = *reinterpret_cast<const uint4 *>(code + 16 * (chunk + 1));
            }
            const int k = (int)(li & 15);
            const unsigned word = (k >> 2) == 0 ? cur.x : (k >> 2) == 1 ? cur.y : (k >> 2) == 2 ? cur.z : cur.w;
            const int sz = 1 << ((word >> (8 * (k & 3))) & 31);
            if (s == sz) {
                out[li] = make_int4(x, y, sz, (int)coff);
                coff += (long long)sz * sz;
                li++;
            } else if (s > 1) {
                pv.set(t + 1, 4);                          // (the children of a 1-pixel node have size 0: the host walk skips them)
            }
        }
        if (st == kOk && li != nleaf) st = kNoTiling;
    }
    if (st == kOk) {
        const long long got = inflated[i];
        if (got < 0 || (got & 3) || got / 4 != ncoef || ncoef > g.coeff_span[l]) st = kCoeffCount;
    }
    long long *cnt = counts + 4 * (long long)i;
    cnt[0] = st == kOk ? ncoef : 0;
    cnt[1] = st == kOk ? nleaf : 0;         // a layer in error hands aej_decode_batch no leaves
    cnt[2] = ns;
    cnt[3] = root;
    status[i] = st;
}

}  // namespace

void launch_headers(hipStream_t st, const unsigned char *states, const long long *desc, const long long *inflated, int nlayers, const HdrGeom &g,
                    unsigned char *codes, int *leaves, long long *counts, int *status)
{
    if (nlayers > 0) hipLaunchKernelGGL(headers_kernel, dim3(nlayers), dim3(64), 0, st, states, desc, inflated, nlayers, g, codes, leaves, counts, status);
}

}  // namespace aej
