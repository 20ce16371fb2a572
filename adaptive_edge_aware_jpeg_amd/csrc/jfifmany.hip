// jfifmany.hip -- the ragged front end of the standard-JPEG encoder: packed RGB images of any sizes, each with its own quality, to the
// quantised coefficients the entropy coders read, every image of a call in one launch (aej_jfif_many_*, include/aej.h).  The files are
// those jfif.hip writes for each image alone: the arithmetic is jfif_arith.h's, shared with it, and the entropy stages, placement and
// scatter are the transcoder's (launch_jfiftrans_chains, jfiftrans.hip): images are grouped by (H, W, sampling, components), a group
// runs one chain, every image of it one "quality" slot with its own quantisers and markers (jfif_params_host: Pillow's, not the
// transcoder's).  An image is packed RGB, or grey (JmGeom::nc = 1: packed uint8 [H][W], a one-component file); both kinds mix in a call.
//
//   k_jm_coefs      eight lanes per 8 x 8 block, 32 blocks per workgroup, every block of every image in one grid.  A lane group finds
//                   its image by binary search over the images' first blocks (as jt_find_file) and its block's place and kind from the
//                   image's JmGeom (jm_block, jfif_many_core.h).  Lane r converts row r of the block -- colour, edge replication,
//                   h2v1 / h2v2 down-sampling (jm_row) -- and runs the row pass of the islow FDCT on its 8 values; the rows cross
//                   through LDS (row stride 9 words: the column reads of a group hit 8 banks); lane c runs the column pass on column c
//                   and quantises it with the image's own table -- each image has one quality, so no int32 DCT plane is kept, which is
//                   where this differs from k_jfif_fdct + k_jfif_quant -- into the block's zigzag order in LDS; then every lane stores
//                   16 of the block's 128 bytes, so a wave writes 1 KiB contiguously.  A dummy luma block of an edge MCU transforms the
//                   real block before it in the MCU and keeps its DC alone, as libjpeg writes it.  A grey image's lane groups take
//                   the same steps with jm_block's and jm_row's one-component branch: raster-order blocks, the sample as Y, the luma
//                   quantiser.
//   (then)          launch_jfiftrans_chains: per group histogram / tables (optimize), k_jfif_annexk (not), or the progressive chain
// Bounds: every index derives from the host-computed JmImage records, checked by jfifmany_plan before any launch.  A lane group whose
// block lies at or past the call's block count, or past its image's n_blocks, reads and writes nothing (it still reaches the barriers).
// jm_row clamps every row to [0, H) and column to [0, W), so reads stay inside [src_offset, src_offset + 3 H W) (grey: H W) of the source, which
// the host has checked against the buffer's size; a block's stores are the 128 bytes at dst + 64 b with b < n_blocks, inside the
// n_blocks * 64 shorts of the image's segment of its group's w.coef (jfiftrans_carve).
#include "aej_common.h"
#include "aej_ctx.h"
#include "aej_launch.h"
#include "jfif_many_core.h"

namespace aej {

constexpr int kJmThreads = 256, kJmBlocks = kJmThreads / 8, kJmStride = 9;

__device__ __forceinline__ int jm_find_image(const JmImage *f, int n, long long t)      // last image whose blk_base <= t (jt_find_file)
{
    return find_last(f, n, t, [](const JmImage &I) { return I.blk_base; });
}

template <int HS, int VS>
__global__ __launch_bounds__(kJmThreads) void k_jm_coefs(const JmImage *__restrict__ images, int n, long long n_blocks,
                                                         const unsigned char *__restrict__ src)
{
    __shared__ int rows[kJmBlocks][8 * kJmStride];
    __shared__ __attribute__((aligned(16))) short zz[kJmBlocks][64];
    const int grp = threadIdx.x >> 3, l = threadIdx.x & 7;
    const long long t = (long long)blockIdx.x * kJmBlocks + grp;
    bool live = t < n_blocks;
    const JmImage *I = images;
    JmGeom g{};
    JmBlock blk{};
    long long b = 0;
    long long d[8];
    if (live) {
        I = images + jm_find_image(images, n, t);
        b = t - I->blk_base;
        g = I->g;
        if (g.nc != 1) { g.hs = HS; g.vs = VS; }             // the call's sampling, known at compile time (a grey image is 1 x 1)
        live = b < g.n_blocks;                               // never false: the images' ranges tile [0, n_blocks)
    }
    if (live) {
        blk = jm_block(g, (int)b);
        jm_row(src + I->src_offset, g, blk, l, d);
        jf_fdct8<true>(d, 1);
#pragma unroll
        for (int c = 0; c < 8; c++) rows[grp][l * kJmStride + c] = (int)d[c];
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int r = 0; r < 8; r++) d[r] = rows[grp][r * kJmStride + l];
        jf_fdct8<false>(d, 1);
        const unsigned short *qt = I->qt[blk.comp > 0];
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const int z = k_zigzag8.position[r * 8 + l];
            zz[grp][z] = jm_store(blk, r * 8 + l, d[r], qt[z]);
        }
    }
    __syncthreads();
    if (live) reinterpret_cast<int4 *>(I->dst + b * 64)[l] = reinterpret_cast<const int4 *>(zz[grp])[l];
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
static void jm_tables(int quality, unsigned short qt[2][64])      // zigzag order, as JfifParams::qt
{
    int t[2][64];
    jfif_quant_tables(quality, t[0], t[1]);
    for (int c = 0; c < 2; c++)
        for (int i = 0; i < 64; i++) qt[c][i] = (unsigned short)t[c][kZigzag8.natural[i]];
}

long long jfifmany_coefs_host(int W, int H, int quality, int ss, const unsigned char *rgb, short *dst, int ncomp)
{
    JmGeom g;
    if (!jm_geom(H, W, ss, g, ncomp) || quality < 1 || quality > 100) return -1;
    if (!rgb || !dst) return g.n_blocks;
    unsigned short qt[2][64];
    jm_tables(quality, qt);
    for (int b = 0; b < g.n_blocks; b++) jm_block_coefs(rgb, g, b, &qt[0][0], dst + (long long)b * 64);
    return g.n_blocks;
}

int jfifmany_plan(const aej_jfif_many_desc *descs, int n, long long src_bytes, int ss, bool opt, bool prog, JmPlan &plan,
                  const char **why, int rst_blocks, int rst_rows)
{
    auto refuse = [&](int i, const char *w) { if (why) *why = w; return i; };
    if (!descs || n < 1 || n > 65535 || ss < 0 || ss > 2) return refuse(0, "1 .. 65535 images and subsampling 0, 1 or 2 required");
    plan = JmPlan{};
    plan.t.prog = prog;
    plan.t.annexk = !prog && !opt;
    plan.t.rst_blocks = rst_blocks; plan.t.rst_rows = rst_rows;
    plan.t.files.assign(n, JtFile{});
    plan.images.assign(n, JmImage{});
    plan.hs = ss == 0 ? 1 : 2; plan.vs = ss == 2 ? 2 : 1;
    for (int i = 0; i < n; i++) {                            // every descriptor before any grouping
        const aej_jfif_many_desc &d = descs[i];
        if (d.width < 1 || d.width > 65535 || d.height < 1 || d.height > 65535) return refuse(i, "width and height in 1..65535 required");
        if (d.quality < 1 || d.quality > 100) return refuse(i, "quality outside 1..100");
        if (d.components != 0 && d.components != 1 && d.components != 3) return refuse(i, "components other than 0 (three), 1 or 3");
        const long long bytes = (d.components == 1 ? 1LL : 3LL) * d.width * d.height;
        if (src_bytes >= 0 && (d.src_offset < 0 || d.src_offset > src_bytes || bytes > src_bytes - d.src_offset))
            return refuse(i, "pixels outside the source buffer");
    }
    for (int i = 0; i < n; i++) {
        const aej_jfif_many_desc &d = descs[i];
        JmImage &I = plan.images[i];
        const int nc = d.components == 1 ? 1 : 3;
        if (!jm_geom(d.height, d.width, ss, I.g, nc)) return refuse(i, "width and height in 1..65535 required");
        JtGroup *grp = jfiftrans_group(plan.t, d.height, d.width, I.g.hs, I.g.vs, nc);
        if (!grp || grp->g.nblk != I.g.n_blocks) return refuse(i, "a size the coders refuse");
        I.blk_base = plan.t.n_blocks;
        I.src_offset = d.src_offset;
        jm_tables(d.quality, I.qt);
        jfiftrans_add(plan.t, *grp, i, I.g.n_blocks);
    }
    if ((plan.t.n_blocks + kJmBlocks - 1) / kJmBlocks > 0x7fffffffLL) return refuse(0, "more blocks than one launch covers");
    const int bad = jfiftrans_close(plan.t);
    if (bad >= 0) return refuse(bad, "a size the coders refuse");
    for (JtGroup &c : plan.t.groups) {
        for (size_t k = 0; k < c.files.size(); k++) {        // Pillow's markers of this image's quality, size and layout
            const aej_jfif_many_desc &d = descs[c.files[k]];
            JfifParams &p = c.par[k];
            jfif_params_host(d.quality, d.height, d.width, p, ss, c.g.ncomp, prog ? 0 : c.g.R);      // (a progressive scan's DRI is k_jfp_tables')
            if (prog) p.hdr[p.dht_off - jfif_sof_bytes(c.g.ncomp) + 1] = 0xC2;      // the frame header is the last segment before the tables: SOF0 -> SOF2
        }
    }
    return -1;
}

unsigned long long jfifmany_carve(void *base, JmPlan &plan)
{
    Carver c(base);
    plan.d_images = c.take<JmImage>((long long)plan.images.size());
    const unsigned long long off = (c.bytes() + 255) & ~255ull;
    const unsigned long long rest = jfiftrans_carve(base ? static_cast<char *>(base) + off : nullptr, plan.t);
    for (size_t i = 0; i < plan.images.size(); i++) plan.images[i].dst = plan.t.files[i].dst;
    return off + rest;
}

hipError_t launch_jfifmany(hipStream_t st, JmPlan &plan, const unsigned char *src, unsigned char *out, unsigned long long cap, long long *lengths,
                           long long *offsets)
{
    const int n = (int)plan.images.size(), hs = plan.hs, vs = plan.vs;
    hipError_t e = hipMemcpyAsync(plan.d_images, plan.images.data(), sizeof(JmImage) * n, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return e;
    if ((e = hipMemcpyAsync(plan.t.d_files, plan.t.files.data(), sizeof(JtFile) * n, hipMemcpyHostToDevice, st)) != hipSuccess) return e;      // k_jt_finish reads it
    const dim3 grid((unsigned)((plan.t.n_blocks + kJmBlocks - 1) / kJmBlocks)), th(kJmThreads);
    if (hs == 1) hipLaunchKernelGGL((k_jm_coefs<1, 1>), grid, th, 0, st, plan.d_images, n, plan.t.n_blocks, src);
    else if (vs == 1) hipLaunchKernelGGL((k_jm_coefs<2, 1>), grid, th, 0, st, plan.d_images, n, plan.t.n_blocks, src);
    else hipLaunchKernelGGL((k_jm_coefs<2, 2>), grid, th, 0, st, plan.d_images, n, plan.t.n_blocks, src);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return launch_jfiftrans_chains(st, plan.t, nullptr, out, cap, lengths, offsets);
}

}  // namespace aej
