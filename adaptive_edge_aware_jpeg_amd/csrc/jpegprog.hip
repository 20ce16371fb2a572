// jpegprog.hip -- progressive JPEG files (SOF2) decoded on the device, pixel-identical to Pillow with libjpeg-turbo for every complete
// progression (aej_jpegprog_*, include/aej.h).  The host walks all markers (jpegprog_parse, jpegparse.hip); the device does the rest, over
// every file of the call at once:
//   un-stuffing      jpegdec.hip's k_jd_count / k_jd_scan_chunks / k_jd_scatter / k_jd_segments, unchanged, with one stream per SCAN where
//                    the baseline path has one per file (launch_jpegdec_unstuff)
//   k_jp_level       one launch per dependency level: a workgroup serves kJpItem restart segments of one scan, stages that scan's
//                    Huffman tables in LDS, and each thread decodes one segment (jpegprog_core.h: DC first, AC first, AC refinement)
//                    into the file's coefficients; a DC refinement scan takes one thread per unit, block i reading bit i
//   k_jp_status      one thread per scan: a scan's status becomes its file's
//   k_jd_idct, k_jd_rgb   jpegdec.hip's reconstruction, unchanged (launch_jpegdec_recon); k_jd_scaled for files decoded at scale 2, 4, 8
// Scans of one level touch disjoint (component, coefficient) cells, so nothing in a launch waits for anything else in it; the levels
// are launch boundaries.  Bounds: every index derives from the host-validated layout; a segment's reads stay inside its scan's clean
// stream, its stores inside its file's blocks (jp_slot), its loops inside its unit count and bit length.
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "aej_ctx.h"

namespace aej {

constexpr int kJpUnstuffS = 1 << 20;      // the un-stuffing kernels size subsequence slots nobody uses here; one per MiB keeps them few

// kFour: k_jp_level4, which a call with a four-component or RGB-coded file runs for all of its files: a fourth table slot in LDS for an
// interleaved DC scan of four components (fadobe[file].dc3), a fourth DC predictor, component 3's blocks in jp_slot
template <bool kFour>
__device__ __forceinline__ void jp_level(const JpScan *__restrict__ scans, const JdFile *__restrict__ sfiles,
                                         const aej_jpegdec_desc *__restrict__ sdescs, const JpItem *__restrict__ items,
                                         const JdSeg *__restrict__ segs, const unsigned char *__restrict__ clean,
                                         short *__restrict__ coef, int *__restrict__ sstatus, aej_jpegdec_huff *tab,
                                         const aej_jpeg_adobe *__restrict__ fadobe)
{
    const JpItem it = items[blockIdx.x];
    const JpScan sc = scans[it.scan];
    const int ntab = sc.kind == kJpDcFirst ? min(sc.ncomp, 3) : sc.kind == kJpDcRefine ? 0 : 1;
    const unsigned *src = reinterpret_cast<const unsigned *>(sc.kind == kJpDcFirst ? sdescs[it.scan].dc : sdescs[it.scan].ac);
    unsigned *dst = reinterpret_cast<unsigned *>(tab);
    for (int i = threadIdx.x; i < ntab * (int)(sizeof(aej_jpegdec_huff) / 4); i += kJpItem) dst[i] = src[i];
    if (kFour && sc.kind == kJpDcFirst && sc.ncomp == 4) {
        const unsigned *src3 = reinterpret_cast<const unsigned *>(&fadobe[sc.file].dc3);
        for (int i = threadIdx.x; i < (int)(sizeof(aej_jpegdec_huff) / 4); i += kJpItem) dst[3 * (sizeof(aej_jpegdec_huff) / 4) + i] = src3[i];
    }
    __syncthreads();
    const unsigned char *cl = clean + sfiles[it.scan].clean_off;
    short *c = coef + sc.blk_base * 64;
    const long long units = (long long)sc.units_x * sc.units_y;
    int rc = kJdRunStop;
    if (sc.kind == kJpDcRefine) {
        const long long u = (long long)it.first + threadIdx.x;
        if (u >= units) return;
        const long long g = sc.restart_interval ? u / sc.restart_interval : 0;
        if (g >= sc.n_segments) return;
        rc = jp_dc_refine_unit<kFour>(sc, cl, segs[sc.seg_base + g], u, c);
    } else {
        const long long g = (long long)it.first + threadIdx.x;
        if (g >= sc.n_segments) return;
        const JdSeg sg = segs[sc.seg_base + g];
        const long long u0 = min((long long)sg.first_mcu, units);
        const int nu = (int)min((long long)sg.n_mcu, units - u0);
        JpBits b(cl, sg.start * 8, (sg.start + sg.nbytes) * 8);
        rc = sc.kind == kJpDcFirst ? jp_dc_first<kFour>(sc, tab, b, u0, nu, c)
           : sc.kind == kJpAcFirst ? jp_ac_first<kFour>(sc, tab[0], b, u0, nu, c) : jp_ac_refine<kFour>(sc, tab[0], b, u0, nu, c);
    }
    if (rc != kJdRunStop) atomicCAS(sstatus + it.scan, 0, jp_status(rc));
}

__global__ __launch_bounds__(kJpItem) void k_jp_level(const JpScan *__restrict__ scans, const JdFile *__restrict__ sfiles,
                                                      const aej_jpegdec_desc *__restrict__ sdescs, const JpItem *__restrict__ items,
                                                      const JdSeg *__restrict__ segs, const unsigned char *__restrict__ clean,
                                                      short *__restrict__ coef, int *__restrict__ sstatus)
{
    __shared__ aej_jpegdec_huff tab[3];
    jp_level<false>(scans, sfiles, sdescs, items, segs, clean, coef, sstatus, tab, nullptr);
}

__global__ __launch_bounds__(kJpItem) void k_jp_level4(const JpScan *__restrict__ scans, const JdFile *__restrict__ sfiles,
                                                       const aej_jpegdec_desc *__restrict__ sdescs, const JpItem *__restrict__ items,
                                                       const JdSeg *__restrict__ segs, const unsigned char *__restrict__ clean,
                                                       short *__restrict__ coef, int *__restrict__ sstatus, const aej_jpeg_adobe *__restrict__ fadobe)
{
    __shared__ aej_jpegdec_huff tab[4];
    jp_level<true>(scans, sfiles, sdescs, items, segs, clean, coef, sstatus, tab, fadobe);
}

__global__ __launch_bounds__(256) void k_jp_status(const JpScan *__restrict__ scans, int ns, const int *__restrict__ sstatus, int *__restrict__ status)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= ns) return;
    const int v = sstatus[s];
    if (v) atomicCAS(status + scans[s].file, 0, v);
}

// ---- host: validation, layout, launch sequence -----------------------------------------------------------------------------------------
// Everything the kernels index with is recomputed or checked here; the dependency levels are derived again rather than trusted.
bool jpegprog_layout(const aej_jpegprog_frame *frames, const aej_jpegprog_scan *scans_in, int n, JpLayout &y, const JdResolved &r)
{
    const aej_jpeg_adobe *adobe = r.adobe;
    y = JpLayout{};
    if (!frames || !scans_in || n < 1) return false;
    y.ffiles.assign(n, JdFile{});
    y.fdescs.resize(n);
    struct Ref { int level, file, idx; const aej_jpegprog_scan *s; };
    std::vector<Ref> order;
    long long s0 = 0;
    for (int i = 0; i < n; i++) {
        const aej_jpegprog_frame &f = frames[i];
        const aej_jpeg_adobe *x = adobe ? adobe + i : nullptr;
        if (!jpeg_frame_ok(f, x) || f.n_scans < 1 || f.n_scans > 4096) return false;
        aej_jpegdec_desc &d = y.fdescs[i];
        memset(&d, 0, sizeof d);
        d.width = f.width; d.height = f.height; d.ncomp = f.ncomp; d.hs = f.hs; d.vs = f.vs; d.mcux = f.mcux; d.mcuy = f.mcuy;
        d.blocks_per_mcu = f.blocks_per_mcu; d.n_segments = 1; d.sof = f.sof; d.precision16 = f.precision16;
        memcpy(d.qt, f.qt, sizeof d.qt);
        jpeg_recon_layout(d, r.shifts.empty() ? 0 : r.shifts[i], y.ffiles[i], y.fz, r.boxes ? r.boxes + 4 * i : nullptr, false, x);      // a boxed file: all coefficients, k_jd_sbox
        int cell_level[4][64];
        for (int c = 0; c < 4; c++) for (int k = 0; k < 64; k++) cell_level[c][k] = -1;
        for (int j = 0; j < f.n_scans; j++) {
            const aej_jpegprog_scan &s = scans_in[s0 + j];
            if (s.ncomp < 1 || s.ncomp > f.ncomp || (s.ncomp > 1 && s.ncomp != f.ncomp)) return false;
            for (int k = 0; k < s.ncomp; k++)
                if (s.comp[k] < 0 || s.comp[k] >= f.ncomp || (s.ncomp > 1 && s.comp[k] != k)) return false;
            if (s.ss < 0 || s.ss > s.se || s.se > 63 || (s.ss == 0 && s.se != 0) || (s.ss > 0 && s.ncomp != 1)) return false;
            if (s.al < 0 || s.al > 13 || s.ah < 0 || s.ah > 14 || s.restart_interval < 0 || s.data_length < 0) return false;
            int ux, uy;
            jp_scan_units(f, s.ncomp, s.comp[0], ux, uy, x);
            const long long units = (long long)ux * uy;
            if (s.units_x != ux || s.units_y != uy) return false;
            if (s.n_segments != (s.restart_interval ? (units + s.restart_interval - 1) / s.restart_interval : 1)) return false;
            int level = 0;
            for (int k = 0; k < s.ncomp; k++)
                for (int z = s.ss; z <= s.se; z++) level = std::max(level, cell_level[s.comp[k]][z] + 1);
            for (int k = 0; k < s.ncomp; k++)
                for (int z = s.ss; z <= s.se; z++) cell_level[s.comp[k]][z] = level;
            order.push_back(Ref{ level, i, (int)(s0 + j), &s });
            y.n_levels = std::max(y.n_levels, level + 1);
        }
        s0 += f.n_scans;
    }
    std::stable_sort(order.begin(), order.end(), [](const Ref &a, const Ref &b) { return a.level < b.level; });
    const int ns = (int)order.size();
    y.scans.resize(ns);
    y.sfiles.assign(ns, JdFile{});
    y.sdescs.resize(ns);
    y.src.resize(ns);
    y.level_items.assign(y.n_levels + 1, 0);
    for (int t = 0; t < ns; t++) {
        const aej_jpegprog_scan &s = *order[t].s;
        const aej_jpegprog_frame &f = frames[order[t].file];
        y.src[t] = order[t].idx;
        aej_jpegdec_desc &d = y.sdescs[t];             // what the un-stuffing kernels read of a stream: its segments and unit counts
        memset(&d, 0, sizeof d);
        d.mcux = s.units_x; d.mcuy = s.units_y; d.restart_interval = s.restart_interval; d.n_segments = s.n_segments;
        memcpy(d.dc, s.dc, sizeof d.dc);
        d.ac[0] = s.ac;
        JdFile &F = y.sfiles[t];
        jpeg_stream_layout(s.data_length, s.n_segments, kJpUnstuffS, F, y.sz);
        JpScan &o = y.scans[t];
        o.file = order[t].file;
        o.kind = s.ss == 0 ? (s.ah ? kJpDcRefine : kJpDcFirst) : (s.ah ? kJpAcRefine : kJpAcFirst);
        o.level = order[t].level;
        o.ncomp = s.ncomp; o.comp0 = s.comp[0];
        o.ss = s.ss; o.se = s.se; o.al = s.al;
        o.nf = f.ncomp; o.hs = f.hs; o.vs = f.vs; o.mcux = f.mcux; o.bpm = f.blocks_per_mcu;
        o.units_x = s.units_x; o.units_y = s.units_y;
        o.restart_interval = s.restart_interval; o.n_segments = s.n_segments;
        o.seg_base = F.seg_base;
        o.blk_base = y.ffiles[o.file].blk_base; o.n_blocks = y.ffiles[o.file].n_blocks;
        o.h3 = adobe && f.ncomp == 4 ? adobe[o.file].h3 : 0; o.v3 = adobe && f.ncomp == 4 ? adobe[o.file].v3 : 0;
        const long long work = o.kind == kJpDcRefine ? (long long)s.units_x * s.units_y : s.n_segments;
        for (long long first = 0; first < work; first += kJpItem) y.items.push_back(JpItem{ t, (int)first });
        y.level_items[o.level + 1] = (long long)y.items.size();
    }
    for (int l = 1; l <= y.n_levels; l++) y.level_items[l] = std::max(y.level_items[l], y.level_items[l - 1]);
    if (y.fz.grpa > 0) y.fadobe.assign(adobe, adobe + n);      // a call with a four-component or RGB-coded file: uploaded with the rest
    return true;
}

unsigned long long jpegprog_carve(void *base, const JpLayout &y, JpBufs &w)
{
    Carver c(base);
    const size_t ns = y.scans.size(), nf = y.ffiles.size();
    w.blob = c.take<char>(jpegprog_blob(y, nullptr));
    Carver b(w.blob);                                  // the parts of the upload, as jpegprog_blob packs them
    w.s.files = b.take<JdFile>(ns);
    w.s.descs = b.take<aej_jpegdec_desc>(ns);
    w.scans = b.take<JpScan>(ns);
    w.items = b.take<JpItem>(y.items.size());
    w.f.files = b.take<JdFile>(nf);
    w.f.descs = b.take<aej_jpegdec_desc>(nf);
    w.f.adobe = y.fadobe.empty() ? nullptr : b.take<aej_jpeg_adobe>(nf);
    w.s.adobe = nullptr;
    w.s.cnt = c.take<int>(y.sz.chunks * 3);
    w.s.pre = c.take<long long>(y.sz.chunks * 3);
    w.s.clean_len = c.take<long long>(ns);
    w.s.segs = c.take<JdSeg>(y.sz.segs);
    w.s.clean = c.take<unsigned char>(y.sz.clean);
    w.sstatus = c.take<int>(ns);
    w.f.coef = c.take<short>(y.fz.blocks * 64);
    w.f.planes = c.take<unsigned char>(y.fz.planes);
    return c.bytes();
}

// the one upload: per-scan streams and descriptors, scans, work items, per-file layout and descriptors (each part 256-byte aligned)
unsigned long long jpegprog_blob(const JpLayout &y, std::vector<unsigned char> *out)
{
    unsigned long long off = 0;
    auto put = [&](const void *src, size_t bytes) {
        if (out) { out->resize(off + (bytes + 255) / 256 * 256); if (bytes) memcpy(out->data() + off, src, bytes); }
        off += (bytes + 255) / 256 * 256;
    };
    put(y.sfiles.data(), sizeof(JdFile) * y.sfiles.size());
    put(y.sdescs.data(), sizeof(aej_jpegdec_desc) * y.sdescs.size());
    put(y.scans.data(), sizeof(JpScan) * y.scans.size());
    put(y.items.data(), sizeof(JpItem) * y.items.size());
    put(y.ffiles.data(), sizeof(JdFile) * y.ffiles.size());
    put(y.fdescs.data(), sizeof(aej_jpegdec_desc) * y.fdescs.size());
    if (!y.fadobe.empty()) put(y.fadobe.data(), sizeof(aej_jpeg_adobe) * y.fadobe.size());
    return off;
}

// levels [0, n_levels) of the entropy stage; the coefficients are zeroed first
hipError_t launch_jpegprog_entropy(hipStream_t st, const JpLayout &y, const JpBufs &w, const void *blob_host, unsigned long long blob_bytes,
                                   const unsigned char *data, int n_levels, int *status)
{
    const int ns = (int)y.scans.size(), nf = (int)y.ffiles.size();
    hipError_t e = hipMemcpyAsync(w.blob, blob_host, blob_bytes, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(status, 0, sizeof(int) * nf, st)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(w.f.coef, 0, (size_t)y.fz.blocks * 128, st)) != hipSuccess) return e;
    if ((e = launch_jpegdec_unstuff(st, ns, y.sz, w.s, data, kJpUnstuffS, w.sstatus)) != hipSuccess) return e;
    for (int l = 0; l < std::min(n_levels, y.n_levels); l++) {
        const long long lo = y.level_items[l], hi = y.level_items[l + 1];
        if (hi > lo && y.fz.grpa > 0)
            hipLaunchKernelGGL(k_jp_level4, dim3((unsigned)(hi - lo)), dim3(kJpItem), 0, st, w.scans, w.s.files, w.s.descs, w.items + lo, w.s.segs,
                               w.s.clean, w.f.coef, w.sstatus, w.f.adobe);
        else if (hi > lo)
            hipLaunchKernelGGL(k_jp_level, dim3((unsigned)(hi - lo)), dim3(kJpItem), 0, st, w.scans, w.s.files, w.s.descs, w.items + lo, w.s.segs,
                               w.s.clean, w.f.coef, w.sstatus);
    }
    hipLaunchKernelGGL(k_jp_status, dim3((ns + 255) / 256), dim3(256), 0, st, w.scans, ns, w.sstatus, status);
    return hipGetLastError();
}

hipError_t launch_jpegprog_recon(hipStream_t st, const JpLayout &y, const JpBufs &w, unsigned char *out)
{
    return launch_jpegdec_recon(st, (int)y.ffiles.size(), y.fz, w.f, out);
}

// ---- host: the same decode stepped through on the CPU (aej_test_jpegprog_coefs_host) -------------------------------------------------------
int jpegprog_coefs_host(const aej_jpegprog_frame &frame, const aej_jpegprog_scan *scans_in, const unsigned char *file, unsigned long long nbytes,
                        int n_levels, short *coef, unsigned long long coef_blocks)
{
    JpLayout y;
    if (!jpegprog_layout(&frame, scans_in, 1, y, {})) return AEJ_ERR_ARG;
    if ((unsigned long long)y.fz.blocks > coef_blocks) return AEJ_ERR_CAPACITY;
    memset(coef, 0, (size_t)y.fz.blocks * 128);
    for (size_t t = 0; t < y.scans.size(); t++) {
        const JpScan &sc = y.scans[t];
        const aej_jpegprog_scan &in = scans_in[y.src[t]];
        if (sc.level >= n_levels) continue;
        if (in.data_offset < 0 || (unsigned long long)in.data_offset + (unsigned long long)in.data_length > nbytes) return AEJ_ERR_ARG;
        const unsigned char *s = file + in.data_offset;
        std::vector<unsigned> words((size_t)(in.data_length / 4 + 8), 0u);
        unsigned char *clean = reinterpret_cast<unsigned char *>(words.data());
        std::vector<JdSeg> segs(1, JdSeg{});
        long long o = 0;
        for (long long p = 0; p < in.data_length; p++) {
            const int c = jd_byte_class(s, in.data_length, p);
            if (c == kJdByteEnd) break;
            if (c == kJdByteData) clean[o++] = s[p];
            else if (c == kJdByteRst) { JdSeg g{}; g.start = o; segs.push_back(g); }
        }
        if ((int)segs.size() != sc.n_segments) return AEJ_JPEGDEC_BAD_RESTART;
        const long long units = (long long)sc.units_x * sc.units_y, ri = sc.restart_interval ? sc.restart_interval : units;
        for (size_t g = 0; g < segs.size(); g++) {
            segs[g].nbytes = (g + 1 < segs.size() ? segs[g + 1].start : o) - segs[g].start;
            segs[g].first_mcu = (int)std::min((long long)g * ri, units);
            segs[g].n_mcu = (int)std::min(ri, units - segs[g].first_mcu);
        }
        const aej_jpegdec_desc &d = y.sdescs[t];
        for (const JdSeg &sg : segs) {
            int rc = kJdRunStop;
            if (sc.kind == kJpDcRefine) {
                for (long long u = sg.first_mcu; u < sg.first_mcu + sg.n_mcu && rc == kJdRunStop; u++) rc = jp_dc_refine_unit(sc, clean, sg, u, coef);
            } else {
                JpBits b(clean, sg.start * 8, (sg.start + sg.nbytes) * 8);
                rc = sc.kind == kJpDcFirst ? jp_dc_first(sc, d.dc, b, sg.first_mcu, sg.n_mcu, coef)
                   : sc.kind == kJpAcFirst ? jp_ac_first(sc, d.ac[0], b, sg.first_mcu, sg.n_mcu, coef) : jp_ac_refine(sc, d.ac[0], b, sg.first_mcu, sg.n_mcu, coef);
            }
            if (rc != kJdRunStop) return jp_status(rc);
        }
    }
    return 0;
}

}  // namespace aej
