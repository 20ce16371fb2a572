// jfiftrans.hip -- lossless transcode: JPEG files Huffman-decoded to their quantised coefficients (jpegdec.hip, jpegprog.hip) and
// entropy-coded again under optimal tables, as a baseline (jfif.hip, optimize) or a progressive file (jfifprog.hip), with no IDCT,
// colour, FDCT or second quantisation in between (aej_jfif_transcode_*, include/aej.h).  What jpegtran -optimize / -progressive do.
//
// The decoders leave a file's blocks in MCU order with the dummy edge blocks, natural order inside a block; the coders read the same
// MCU order, zigzag order inside a block (a one-component file: its real blocks in raster order, both sides).  Files are grouped by the
// (H, W, hs, vs, components) of their output; a group runs the existing entropy stages once, every
// file of it one "quality" of a one-image batch, so that JfifParams::hdr -- per quality in the coders -- carries each file's own
// markers (SOI, JFIF APP0 with the source's density, the source's quantisation tables and frame header).  Stages:
//   k_jt_bridge     one wave per block: lane z reads natural index k_zigzag8.natural[z] of the source block and writes position z of the coder's
//                   block (128 contiguous bytes in, 128 out); the range check of libjpeg's encoder (AC |v| <= 1023, DC -1024 .. 1023)
//                   is one ballot, and a block that fails marks its file by one atomicCAS and is written as zeros.  So are the blocks
//                   of a file whose decode had failed before this launch; whether the GOOD blocks of a file that fails in this launch
//                   arrive as data or as zeros depends on when their wave reads the status word, and does not matter: the file's
//                   length becomes 0, and every block the coders are given is in range, so their per-block stream bound holds
//   k_jt_transform  in the place of k_jt_bridge when a file of the call has a lossless transform (aej_jfif_transform_*; flips, rotations,
//                   transposition: jfif_transform_core.h).  Still one wave per OUTPUT block, lane z writing position z of the coder's block:
//                   the wave is block b of its file in the OUTPUT group's MCU order, reads block jx_source_block(b) of the SOURCE's MCU
//                   order (another sampling after a transposition, fewer MCUs after a trim) and there natural index
//                   jx_source_index(k_zigzag8.natural[z]), negated where the mirror says so -- one 128-byte block in, one out, as the bridge.  A
//                   dummy output block is written as libjpeg writes it: lane 0 takes the DC of the real block before it in the MCU, the
//                   AC lanes read nothing and write 0.  Range ballot and status protocol are the bridge's (the limits are symmetric but
//                   for the DC, which no transform negates).  A file whose transform is "none" goes through it unchanged, dummies too.
//   k_jt_cut        in the place of both when a file of the call has a crop or drops its chroma (aej_jfif_transform_*_cut; JxGeom::cut):
//                   k_jt_transform with jx_source_block reading the crop offset, the whole transform's grid and the source's own component
//                   count from the file's JxGeom, so that the output's blocks may be fewer than the source's and of one component where
//                   the source has three; a file of the call without either takes the path it takes in k_jt_transform.  A call without
//                   such a file never launches it
//   (per group)     launch_jfif_entropy / launch_jfifprog_entropy: histogram .. file lengths, unchanged; a source's restart markers
//                   are gone with its entropy coding, and the output gets those of JtPlan::rst_blocks / rst_rows (jfiftrans_close gives
//                   every group its interval; 0, 0: none)
//   k_jt_sos_ids    progressive groups with component ids other than 1, 2, 3 only: the ids in the SOS markers k_jfp_tables wrote
//   k_jt_place      one thread: the files' offsets in the packed output, group after group
//   (per group)     launch_jfif_scatter / launch_jfifprog_scatter
//   k_jt_finish     one thread per file: length and offset in the caller's order; a failed file's length is 0
// Everything after the bridge is launch_jfiftrans_chains, which the ragged encoder (jfifmany.hip) runs too: its front end fills
// JtFile::dst from pixels, its plan is made of the same jfiftrans_group / jfiftrans_add / jfiftrans_close, and with JtPlan::annexk its
// baseline files carry the Annex K tables (launch_jfif_entropy_annexk) instead of their own.
// Bounds: every index derives from the host layout (JtPlan): a wave's block lies inside [0, n_blocks) of the file jt_find_file returns,
// src and dst are that file's own ranges of the decoder's and the group's coefficient buffers, the status index is below the call's
// file count, and an SOS marker is patched only inside the kJfpPiece bytes of its own piece.  With a transform the file's JxGeom, made
// by jx_geom on the host, is all the mapping reads: jfiftrans_plan has checked that its n_out is the group's block count (the size of
// dst, and the file's n_blocks) and its n_src the count the decoder holds (the size of src); jx_source_block maps [0, n_out) into
// [0, n_src) -- a mirrored axis is a whole number of MCUs, a transposed block of an h x v grid lies in the v x h grid, the walk back from
// a dummy block stays inside its MCU -- and the kernel still drops a wave whose source block would lie outside.  With a cut the same holds:
// the output's MCU (mx + cx, my + cy) lies inside the whole transform's grid because the box lies inside the transformed image (jx_geom
// refuses any other), and a luma block of a chroma drop lies inside the source's MCU grid because its MCU does.
#include "aej_common.h"
#include "aej_ctx.h"
#include "aej_launch.h"
#include "jfif_huff_core.h"

namespace aej {

constexpr int kJtThreads = 256;

__device__ __forceinline__ int jt_find_file(const JtFile *f, int n, long long t)      // last file whose src_base <= t (jd_find_file)
{
    return find_last(f, n, t, [](const JtFile &F) { return F.src_base; });
}

__global__ __launch_bounds__(kJtThreads) void k_jt_bridge(const JtFile *__restrict__ files, int n, long long n_blocks, int *__restrict__ status)
{
    const long long t = (long long)blockIdx.x * (kJtThreads / 64) + (threadIdx.x >> 6);      // uniform over the wave
    if (t >= n_blocks) return;
    const int z = threadIdx.x & 63;
    const JtFile F = files[jt_find_file(files, n, t)];
    const long long b = t - F.src_base;
    if (b >= F.n_blocks) return;                             // never: the files' ranges tile [0, n_blocks)
    const int v = F.src[b * 64 + k_zigzag8.natural[z]];
    const bool bad = z == 0 ? (v < -1024 || v > 1023) : (v < -1023 || v > 1023);
    const bool any_bad = __ballot(bad) != 0ull;
    if (any_bad && z == 0) atomicCAS(status + F.status_index, 0, AEJ_JPEGDEC_COEF_RANGE);
    const bool failed = any_bad || status[F.status_index] != 0;
    F.dst[b * 64 + z] = failed ? (short)0 : (short)v;
}

// The bridge with a lossless transform (header comment): geom[i] belongs to files[i].
__global__ __launch_bounds__(kJtThreads) void k_jt_transform(const JtFile *__restrict__ files, const JxGeom *__restrict__ geom, int n, long long n_blocks,
                                                             int *__restrict__ status)
{
    const long long t = (long long)blockIdx.x * (kJtThreads / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // scalar: the maps are per wave
    if (t >= n_blocks) return;
    const int z = threadIdx.x & 63;
    const int fi = jt_find_file(files, n, t);
    const JtFile F = files[fi];
    const JxGeom G = geom[fi];
    const long long b = t - F.src_base;
    if (b >= F.n_blocks || b >= G.n_out) return;             // never: the files' ranges tile [0, n_blocks), and n_blocks is n_out
    int sb = (int)b, si = k_zigzag8.natural[z];
    bool dummy = false, negate = false;
    if (G.xf != kJxNone) {
        sb = jx_source_block(G, (int)b, &dummy);
        si = jx_source_index(G, si, &negate);
    }
    if (sb < 0 || sb >= G.n_src) return;                     // never (header comment)
    int v = dummy && z != 0 ? 0 : F.src[(long long)sb * 64 + si];
    if (negate) v = -v;
    const bool bad = z == 0 ? (v < -1024 || v > 1023) : (v < -1023 || v > 1023);
    const bool any_bad = __ballot(bad) != 0ull;
    if (any_bad && z == 0) atomicCAS(status + F.status_index, 0, AEJ_JPEGDEC_COEF_RANGE);
    const bool failed = any_bad || status[F.status_index] != 0;
    F.dst[b * 64 + z] = failed ? (short)0 : (short)v;
}

// The bridge with a crop or a chroma drop (header comment): k_jt_transform's shape -- one wave per OUTPUT block, the mapping scalar, lane z
// writing position z -- with the cut's fields of JxGeom read.  No LDS: a wave reads one 128-byte block and writes one.
__global__ __launch_bounds__(kJtThreads) void k_jt_cut(const JtFile *__restrict__ files, const JxGeom *__restrict__ geom, int n, long long n_blocks,
                                                       int *__restrict__ status)
{
    const long long t = (long long)blockIdx.x * (kJtThreads / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // scalar: the maps are per wave
    if (t >= n_blocks) return;
    const int z = threadIdx.x & 63;
    const int fi = jt_find_file(files, n, t);
    const JtFile F = files[fi];
    const JxGeom G = geom[fi];
    const long long b = t - F.src_base;
    if (b >= F.n_blocks || b >= G.n_out) return;             // never: the files' ranges tile [0, n_blocks), and n_blocks is n_out
    int sb = (int)b, si = k_zigzag8.natural[z];
    bool dummy = false, negate = false;
    if (G.cut) {
        sb = jx_source_block(G, (int)b, &dummy, true);
        si = jx_source_index(G, si, &negate);
    } else if (G.xf != kJxNone) {
        sb = jx_source_block(G, (int)b, &dummy);
        si = jx_source_index(G, si, &negate);
    }
    if (sb < 0 || sb >= G.n_src) return;                     // never (header comment)
    int v = dummy && z != 0 ? 0 : F.src[(long long)sb * 64 + si];
    if (negate) v = -v;
    const bool bad = z == 0 ? (v < -1024 || v > 1023) : (v < -1023 || v > 1023);
    const bool any_bad = __ballot(bad) != 0ull;
    if (any_bad && z == 0) atomicCAS(status + F.status_index, 0, AEJ_JPEGDEC_COEF_RANGE);
    const bool failed = any_bad || status[F.status_index] != 0;
    F.dst[b * 64 + z] = failed ? (short)0 : (short)v;
}

// the component ids of the SOS markers of a progressive group: k_jfp_tables writes index + 1; the frame header in the file's prefix
// (the last 19 bytes before dht_off) has the source's.  One thread per (file, scan).
__global__ __launch_bounds__(kJtThreads) void k_jt_sos_ids(JfpGeom g, const JfifParams *__restrict__ par, unsigned char *__restrict__ fhdr,
                                                           const int *__restrict__ fhdr_len)
{
    const long long idx = (long long)blockIdx.x * kJtThreads + threadIdx.x;
    if (idx >= (long long)g.segs * g.nscan) return;
    const long long seg = idx / g.nscan;
    const int si = (int)(idx % g.nscan);
    const JfifParams &p = par[seg / g.B];
    const int nf = 1 + g.nchroma, sofn = jfif_sof_bytes(nf);                             // components of the frame; its header's bytes
    const int nc = g.sc[si].Ss == 0 ? nf : 1, hl = fhdr_len[idx], at = hl - (8 + 2 * nc);
    if (p.dht_off < sofn || p.dht_off > kJfifHdrMax || at < 0 || hl > kJfpPiece) return;
    const unsigned char *sof = p.hdr + p.dht_off - sofn;
    unsigned char *q = fhdr + idx * kJfpPiece + at;
    for (int c = 0; c < nc; c++) {
        const int k = q[5 + 2 * c] - 1;
        if (k >= 0 && k < nf) q[5 + 2 * c] = sof[10 + 3 * k];
    }
}

__global__ void k_jt_place(int n, const long long *__restrict__ glen, long long *__restrict__ goff, long long *__restrict__ total)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    long long off = 0;
    for (int o = 0; o < n; o++) {
        goff[o] = off;
        off += glen[o];
    }
    *total = off;
}

__global__ __launch_bounds__(kJtThreads) void k_jt_finish(const JtFile *__restrict__ files, int n, const int *__restrict__ status,
                                                          const long long *__restrict__ glen, const long long *__restrict__ goff,
                                                          long long *__restrict__ lengths, long long *__restrict__ offsets)
{
    const int i = blockIdx.x * kJtThreads + threadIdx.x;
    if (i >= n) return;
    const JtFile &F = files[i];
    lengths[i] = status && status[F.status_index] ? 0 : glen[F.out_pos];      // (the encoder of jfifmany.hip has no status words)
    offsets[i] = goff[F.out_pos];
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
template <class D>
static void jt_source(const D &d, JtSource &s)
{
    s = JtSource{};
    s.width = d.width; s.height = d.height; s.hs = d.hs; s.vs = d.vs; s.ncomp = d.ncomp == 1 ? 1 : 3;
    for (int c = 0; c < s.ncomp; c++) {
        s.comp_id[c] = d.comp_id[c];
        s.comp_tq[c] = d.comp_tq[c];
        for (int i = 0; i < 64; i++) s.qt[c][i] = d.qt[c][i];
    }
    s.units = 0; s.xdensity = 1; s.ydensity = 1;
}
void jfiftrans_source(const aej_jpegdec_desc &d, JtSource &s) { jt_source(d, s); }
void jfiftrans_source(const aej_jpegprog_frame &f, JtSource &s) { jt_source(f, s); }

// SOI, JFIF 1.01 APP0 with the source's density, one DQT per distinct table id in order of first reference, SOF0 / SOF2.  One component:
// its table as table 0, sampled 1 x 1
int jfiftrans_prefix_host(const JtSource &s, bool prog, unsigned char *o, int capacity)
{
    unsigned char b[2 + 18 + 3 * 69 + 19];
    int n = 0;
    auto put = [&](std::initializer_list<int> v) { for (int x : v) b[n++] = (unsigned char)x; };
    put({ 0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, s.units, s.xdensity >> 8, s.xdensity & 255, s.ydensity >> 8, s.ydensity & 255, 0, 0 });
    const int nc = s.ncomp == 1 ? 1 : 3;
    for (int c = 0; c < nc; c++) {
        bool seen = false;
        for (int e = 0; e < c; e++) seen |= s.comp_tq[e] == s.comp_tq[c];
        if (seen) continue;
        put({ 0xFF, 0xDB, 0, 67, nc == 1 ? 0 : s.comp_tq[c] & 15 });
        for (int i = 0; i < 64; i++) b[n++] = (unsigned char)s.qt[c][kZigzag8.natural[i]];
    }
    put({ 0xFF, prog ? 0xC2 : 0xC0, 0, jfif_sof_bytes(nc) - 2, 8, s.height >> 8, s.height & 255, s.width >> 8, s.width & 255, nc });
    if (nc == 1) put({ s.comp_id[0], 0x11, 0 });
    for (int c = 0; c < 3 && nc == 3; c++) put({ s.comp_id[c], c == 0 ? (s.hs << 4) | s.vs : 0x11, s.comp_tq[c] });
    if (n > capacity) return -1;
    memcpy(o, b, n);
    return n;
}

JtSource jfiftrans_transformed(const JtSource &s, const JxGeom &g)
{
    JtSource o = s;
    o.width = g.oW; o.height = g.oH; o.hs = g.ohs; o.vs = g.ovs;
    o.ncomp = g.nc;                                          // a chroma drop: the luma component alone, its id and its table
    for (int c = 0; c < 3 && g.t; c++)
        for (int i = 0; i < 64; i++) o.qt[c][i] = s.qt[c][(i & 7) * 8 + (i >> 3)];
    return o;
}

void jfiftrans_coefs_host(const JxGeom &g, const short *src, short *dst)
{
    for (int b = 0; b < g.n_out; b++) {
        bool dummy = false;
        const int sb = g.cut ? jx_source_block(g, b, &dummy, true) : g.xf != kJxNone ? jx_source_block(g, b, &dummy) : b;
        for (int z = 0; z < 64; z++) {
            bool negate = false;
            const int si = g.cut || g.xf != kJxNone ? jx_source_index(g, kZigzag8.natural[z], &negate) : kZigzag8.natural[z];
            const int v = dummy && z != 0 ? 0 : src[(long long)sb * 64 + si];
            dst[(long long)b * 64 + z] = (short)(negate ? -v : v);
        }
    }
}

JtGroup *jfiftrans_group(JtPlan &plan, int H, int W, int hs, int vs, int ncomp)
{
    for (JtGroup &c : plan.groups)
        if (c.g.H == H && c.g.W == W && c.g.hs == hs && c.g.vs == vs && c.g.ncomp == ncomp) return &c;
    JtGroup grp{};
    grp.foreign_ids = false;
    if (!jfif_geom_sampled(1, H, W, 1, grp.g, hs, vs, 1, ncomp)) return nullptr;
    plan.groups.push_back(grp);
    return &plan.groups.back();
}

void jfiftrans_add(JtPlan &plan, JtGroup &grp, int i, long long n_out)
{
    grp.files.push_back(i);
    plan.files[i].src_base = plan.n_blocks;
    plan.files[i].n_blocks = n_out;
    plan.n_blocks += n_out;
}

int jfiftrans_close(JtPlan &plan)
{
    long long first = 0;
    for (JtGroup &c : plan.groups) {
        const int ng = (int)c.files.size();
        if (!jfif_geom_sampled(1, c.g.H, c.g.W, ng, c.g, c.g.hs, c.g.vs, 1, c.g.ncomp) || !jfif_geom_restart(c.g, plan.rst_blocks, plan.rst_rows) ||
            (plan.prog && !jfifprog_geom(c.g, c.p, plan.rst_blocks, plan.rst_rows)))
            return c.files[0];
        c.first = first;
        c.par.assign(ng, JfifParams{});
        for (int k = 0; k < ng; k++) plan.files[c.files[k]].out_pos = (int)(first + k);
        first += ng;
    }
    return -1;
}

int jfiftrans_plan(const std::vector<JtSource> &src, const std::vector<long long> &n_blocks, bool prog, const int *xf, int trim, JtPlan &plan,
                   int *why, int rst_blocks, int rst_rows, bool allow440, const int *boxes, bool drop)
{
    auto refuse = [&](int i, int w) { if (why) *why = w; return i; };
    const int n = (int)src.size();
    if (n < 1 || n > 65535 || n_blocks.size() != src.size()) return refuse(0, kJxBadArg);
    plan = JtPlan{};
    plan.prog = prog;
    plan.rst_blocks = rst_blocks; plan.rst_rows = rst_rows;  // a source's own markers are never carried over: the call's options alone decide
    plan.files.assign(n, JtFile{});
    plan.geom.assign(n, JxGeom{});
    for (int i = 0; i < n; i++) {
        const JtSource &s = src[i];
        JxGeom &x = plan.geom[i];
        const int rc = jx_geom(s.height, s.width, s.hs, s.vs, xf ? xf[i] : kJxNone, trim, x, s.ncomp, allow440, boxes ? boxes + 4 * i : nullptr, drop);
        if (rc != kJxOk) return refuse(i, rc);
        plan.transform |= x.xf != kJxNone;
        plan.cut |= x.cut != 0;
        JtGroup *grp = jfiftrans_group(plan, x.oH, x.oW, x.ohs, x.ovs, x.nc);
        if (!grp || n_blocks[i] != x.n_src || grp->g.nblk != x.n_out) return refuse(i, kJxBadArg);
        jfiftrans_add(plan, *grp, i, x.n_out);
        grp->foreign_ids |= s.comp_id[0] != 1 || (x.nc == 3 && (s.comp_id[1] != 2 || s.comp_id[2] != 3));      // the output's components only
    }
    const int bad = jfiftrans_close(plan);
    if (bad >= 0) return refuse(bad, kJxBadArg);
    for (JtGroup &c : plan.groups) {
        for (size_t k = 0; k < c.files.size(); k++) {
            const JtSource s = jfiftrans_transformed(src[c.files[k]], plan.geom[c.files[k]]);
            JfifParams &p = c.par[k];
            const int len = jfiftrans_prefix_host(s, prog, p.hdr, kJfifHdrMax - 14);
            if (len < 0) return refuse(c.files[k], kJxBadArg);
            p.dht_off = p.hdr_len = len;
            if (!prog && s.ncomp == 1) {                     // k_jfif_tables takes the SOS from the end of the markers
                const unsigned char sos[10] = { 0xFF, 0xDA, 0, 8, 1, s.comp_id[0], 0x00, 0, 63, 0 };
                memcpy(p.hdr + len, sos, 10);
                p.hdr_len = len + 10;
            } else if (!prog) {
                const unsigned char sos[14] = { 0xFF, 0xDA, 0, 12, 3, s.comp_id[0], 0x00, s.comp_id[1], 0x11, s.comp_id[2], 0x11, 0, 63, 0 };
                memcpy(p.hdr + len, sos, 14);
                p.hdr_len = len + 14;
            }
        }
    }
    return -1;
}

unsigned long long jfiftrans_carve(void *base, JtPlan &plan)
{
    Carver c(base);
    const long long n = (long long)plan.files.size();
    plan.d_files = c.take<JtFile>(n);
    if (plan.transform || plan.cut) plan.d_geom = c.take<JxGeom>(n);
    plan.glen = c.take<long long>(n);
    plan.goff = c.take<long long>(n);
    plan.total = c.take<long long>(1);
    for (JtGroup &grp : plan.groups) {
        const JfifGeom &g = grp.g;
        if (plan.prog) {
            jfifprog_carve_coded(c, g, grp.p, grp.w, grp.pw);
        } else {
            jfif_carve_coded(c, g, grp.w);
        }
        for (size_t k = 0; k < grp.files.size(); k++)
            plan.files[grp.files[k]].dst = grp.w.coef ? grp.w.coef + (long long)k * g.nblk * 64 : nullptr;
    }
    return c.bytes();
}

hipError_t launch_jfiftrans(hipStream_t st, JtPlan &plan, int *status, unsigned char *out, unsigned long long cap, long long *lengths,
                            long long *offsets)
{
    const int n = (int)plan.files.size();
    hipError_t e = hipMemcpyAsync(plan.d_files, plan.files.data(), sizeof(JtFile) * n, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)((plan.n_blocks + kJtThreads / 64 - 1) / (kJtThreads / 64)));
    if (plan.cut) {
        if ((e = hipMemcpyAsync(plan.d_geom, plan.geom.data(), sizeof(JxGeom) * n, hipMemcpyHostToDevice, st)) != hipSuccess) return e;
        hipLaunchKernelGGL(k_jt_cut, grid, dim3(kJtThreads), 0, st, plan.d_files, plan.d_geom, n, plan.n_blocks, status);
    } else if (plan.transform) {
        if ((e = hipMemcpyAsync(plan.d_geom, plan.geom.data(), sizeof(JxGeom) * n, hipMemcpyHostToDevice, st)) != hipSuccess) return e;
        hipLaunchKernelGGL(k_jt_transform, grid, dim3(kJtThreads), 0, st, plan.d_files, plan.d_geom, n, plan.n_blocks, status);
    } else {
        hipLaunchKernelGGL(k_jt_bridge, grid, dim3(kJtThreads), 0, st, plan.d_files, n, plan.n_blocks, status);
    }
    return launch_jfiftrans_chains(st, plan, status, out, cap, lengths, offsets);
}

hipError_t launch_jfiftrans_chains(hipStream_t st, JtPlan &plan, const int *status, unsigned char *out, unsigned long long cap, long long *lengths,
                                   long long *offsets)
{
    const int n = (int)plan.files.size();
    hipError_t e = hipSuccess;
    for (JtGroup &c : plan.groups) {
        if ((e = hipMemcpyAsync(c.w.par, c.par.data(), sizeof(JfifParams) * c.par.size(), hipMemcpyHostToDevice, st)) != hipSuccess) return e;
        long long *len = plan.glen + c.first, *off = plan.goff + c.first;
        if (!plan.prog) {
            if ((e = plan.annexk ? launch_jfif_entropy_annexk(st, c.g, c.w, len, off) : launch_jfif_entropy(st, c.g, c.w, len, off)) != hipSuccess) return e;
            continue;
        }
        if ((e = launch_jfifprog_entropy(st, c.p, c.pw, c.w.coef, c.w.par, len, off)) != hipSuccess) return e;
        if (c.foreign_ids)
            hipLaunchKernelGGL(k_jt_sos_ids, dim3((unsigned)(((long long)c.p.segs * c.p.nscan + kJtThreads - 1) / kJtThreads)), dim3(kJtThreads), 0, st,
                               c.p, c.w.par, c.pw.fhdr, c.pw.fhdr_len);
    }
    hipLaunchKernelGGL(k_jt_place, dim3(1), dim3(1), 0, st, n, plan.glen, plan.goff, plan.total);
    for (JtGroup &c : plan.groups) {
        if (!out) break;
        e = plan.prog ? launch_jfifprog_scatter(st, c.p, c.pw, c.w.par, plan.glen + c.first, plan.goff + c.first, out, cap)
                      : launch_jfif_scatter(st, c.g, c.w, plan.glen + c.first, plan.goff + c.first, out, cap);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_jt_finish, dim3((unsigned)((n + kJtThreads - 1) / kJtThreads)), dim3(kJtThreads), 0, st, plan.d_files, n, status, plan.glen,
                       plan.goff, lengths, offsets);
    return hipGetLastError();
}

}  // namespace aej
