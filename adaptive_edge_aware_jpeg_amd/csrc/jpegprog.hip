// jpegprog.hip -- progressive JPEG files (SOF2) decoded on the device, pixel-identical to Pillow with libjpeg-turbo for every complete
// progression (aej_jpegprog_*, include/aej.h).  The host walks all markers (jpegprog_parse); the device does the rest, over every file
// of the call at once:
//   un-stuffing      jpegdec.hip's k_jd_count / k_jd_scan_chunks / k_jd_scatter / k_jd_segments, unchanged, with one stream per SCAN where
//                    the baseline path has one per file (launch_jpegdec_unstuff)
//   k_jp_level       one launch per dependency level: a workgroup serves kJpItem restart segments of one scan, stages that scan's
//                    Huffman tables in LDS, and each thread decodes one segment (jpegprog_core.h: DC first, AC first, AC refinement)
//                    into the file's coefficients; a DC refinement scan takes one thread per unit, block i reading bit i
//   k_jp_status      one thread per scan: a scan's status becomes its file's
//   k_jd_idct, k_jd_rgb   jpegdec.hip's reconstruction, unchanged (launch_jpegdec_recon)
// Scans of one level touch disjoint (component, coefficient) cells, so nothing in a launch waits for anything else in it; the levels
// are launch boundaries.  Bounds: every index derives from the host-validated layout; a segment's reads stay inside its scan's clean
// stream, its stores inside its file's blocks (jp_slot), its loops inside its unit count and bit length.
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "aej_common.h"
#include "aej_launch.h"

namespace aej {

constexpr int kJpUnstuffS = 1 << 20;      // the un-stuffing kernels size subsequence slots nobody uses here; one per MiB keeps them few

__global__ __launch_bounds__(kJpItem) void k_jp_level(const JpScan *__restrict__ scans, const JdFile *__restrict__ sfiles,
                                                      const aej_jpegdec_desc *__restrict__ sdescs, const JpItem *__restrict__ items,
                                                      const JdSeg *__restrict__ segs, const unsigned char *__restrict__ clean,
                                                      short *__restrict__ coef, int *__restrict__ sstatus)
{
    __shared__ aej_jpegdec_huff tab[3];
    const JpItem it = items[blockIdx.x];
    const JpScan sc = scans[it.scan];
    const int ntab = sc.kind == kJpDcFirst ? min(sc.ncomp, 3) : sc.kind == kJpDcRefine ? 0 : 1;
    const unsigned *src = reinterpret_cast<const unsigned *>(sc.kind == kJpDcFirst ? sdescs[it.scan].dc : sdescs[it.scan].ac);
    unsigned *dst = reinterpret_cast<unsigned *>(tab);
    for (int i = threadIdx.x; i < ntab * (int)(sizeof(aej_jpegdec_huff) / 4); i += kJpItem) dst[i] = src[i];
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
        rc = jp_dc_refine_unit(sc, cl, segs[sc.seg_base + g], u, c);
    } else {
        const long long g = (long long)it.first + threadIdx.x;
        if (g >= sc.n_segments) return;
        const JdSeg sg = segs[sc.seg_base + g];
        const long long u0 = min((long long)sg.first_mcu, units);
        const int nu = (int)min((long long)sg.n_mcu, units - u0);
        JpBits b(cl, sg.start * 8, (sg.start + sg.nbytes) * 8);
        rc = sc.kind == kJpDcFirst ? jp_dc_first(sc, tab, b, u0, nu, c)
           : sc.kind == kJpAcFirst ? jp_ac_first(sc, tab[0], b, u0, nu, c) : jp_ac_refine(sc, tab[0], b, u0, nu, c);
    }
    if (rc != kJdRunStop) atomicCAS(sstatus + it.scan, 0, jp_status(rc));
}

__global__ __launch_bounds__(256) void k_jp_status(const JpScan *__restrict__ scans, int ns, const int *__restrict__ sstatus, int *__restrict__ status)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= ns) return;
    const int v = sstatus[s];
    if (v) atomicCAS(status + scans[s].file, 0, v);
}

// ---- host: the marker walk -------------------------------------------------------------------------------------------------------------
static void jp_scan_units(const aej_jpegprog_frame &f, int ncomp, int comp0, int &ux, int &uy)
{
    if (ncomp > 1 || f.ncomp == 1 || comp0 > 0) { ux = f.mcux; uy = f.mcuy; }      // chroma is sampled 1x1: its block grid is the MCU grid
    else { ux = (f.width + 7) / 8; uy = (f.height + 7) / 8; }
}

int jpegprog_parse(const unsigned char *b, unsigned long long n, aej_jpegprog_frame &f, std::vector<aej_jpegprog_scan> &scans, std::string &msg)
{
    memset(&f, 0, sizeof f);
    scans.clear();
    auto bad = [&](const std::string &m) { msg = m; return (int)AEJ_ERR_ARG; };
    auto unsup = [&](const std::string &m) { msg = m; return (int)AEJ_ERR_UNSUPPORTED; };
    if (!b || n < 4 || b[0] != 0xFF || b[1] != 0xD8) return bad("not a JPEG file (no SOI marker)");
    uint16_t qt[4][64];
    bool qdef[4] = {}, q16[4] = {}, sof = false, jfif = false, adobe = false, qlatched[3] = {};
    int adobe_transform = -1, ri = 0, nf = 0;
    int coef_al[3][64], cell_level[3][64];
    for (int c = 0; c < 3; c++)
        for (int k = 0; k < 64; k++) { coef_al[c][k] = -1; cell_level[c][k] = -1; }
    JdHuffSrc hs[2][4];
    unsigned long long p = 2;
    for (;;) {
        if (p >= n) return bad("no EOI marker (the file ends after " + std::to_string(scans.size()) + " scans)");
        if (b[p] != 0xFF) return bad("bytes between markers");
        while (p < n && b[p] == 0xFF) p++;
        if (p >= n) return bad("no EOI marker (the file ends in a marker)");
        const int m = b[p++];
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
        if (m == 0xD8) return bad("second SOI marker");
        if (m == 0xD9) break;
        if (p + 2 > n) return bad("truncated marker segment");
        const unsigned L = (unsigned)b[p] << 8 | b[p + 1];
        if (L < 2 || p + L > n) return bad("truncated marker segment");
        const unsigned char *s = b + p + 2;
        const unsigned len = L - 2;
        switch (m) {
        case 0xC0: case 0xC1: return unsup("not a progressive file (SOF" + std::to_string(m - 0xC0) + ")");
        case 0xC2: {
            if (sof) return bad("two SOF markers");
            if (len < 6) return bad("truncated SOF segment");
            if (s[0] != 8) return unsup("sample precision " + std::to_string(s[0]) + " (only 8-bit)");
            f.height = s[1] << 8 | s[2];
            f.width = s[3] << 8 | s[4];
            nf = s[5];
            if (len != 6u + 3u * nf) return bad("SOF length does not match its component count");
            if (f.height == 0) return unsup("DNL (height defined after the scan)");
            if (f.width == 0) return bad("zero image width");
            if (nf != 1 && nf != 3) return unsup(std::to_string(nf) + " components (only 1 or 3)");
            for (int i = 0; i < nf; i++) {
                f.comp_id[i] = s[6 + 3 * i];
                f.comp_h[i] = s[7 + 3 * i] >> 4;
                f.comp_v[i] = s[7 + 3 * i] & 15;
                f.comp_tq[i] = s[8 + 3 * i];
                if (f.comp_h[i] < 1 || f.comp_h[i] > 4 || f.comp_v[i] < 1 || f.comp_v[i] > 4 || f.comp_tq[i] > 3)
                    return bad("bad component sampling factor or table index");
                for (int j = 0; j < i; j++) if (f.comp_id[j] == f.comp_id[i]) return bad("two frame components with one id");
            }
            if (nf == 3) {
                const int h0 = f.comp_h[0], v0 = f.comp_v[0];
                if (f.comp_h[1] != 1 || f.comp_v[1] != 1 || f.comp_h[2] != 1 || f.comp_v[2] != 1 ||
                    !((h0 == 1 && v0 == 1) || (h0 == 2 && v0 == 1) || (h0 == 2 && v0 == 2)))
                    return unsup("sampling factors " + std::to_string(h0) + "x" + std::to_string(v0) + "," + std::to_string(f.comp_h[1]) + "x" +
                                 std::to_string(f.comp_v[1]) + "," + std::to_string(f.comp_h[2]) + "x" + std::to_string(f.comp_v[2]));
                f.hs = h0; f.vs = v0;
                f.blocks_per_mcu = h0 * v0 + 2;
            } else {
                f.hs = f.vs = 1;
                f.blocks_per_mcu = 1;
            }
            f.mcux = (f.width + 8 * f.hs - 1) / (8 * f.hs);
            f.mcuy = (f.height + 8 * f.vs - 1) / (8 * f.vs);
            f.ncomp = nf;
            f.sof = m;
            sof = true;
            break;
        }
        case 0xC3: return unsup("lossless JPEG (SOF3)");
        case 0xC5: case 0xC6: case 0xC7: return unsup("hierarchical JPEG (SOF" + std::to_string(m - 0xC0) + ")");
        case 0xC9: case 0xCA: case 0xCB: case 0xCD: case 0xCE: case 0xCF: case 0xCC:
            return unsup("arithmetic coding (" + std::string(m == 0xCC ? "DAC" : "SOF" + std::to_string(m - 0xC0)) + ")");
        case 0xDC: return unsup("DNL marker");
        case 0xC4: {
            unsigned i = 0;
            while (i < len) {
                const int tc = s[i] >> 4, th = s[i] & 15;
                if (tc > 1 || th > 3) return bad("bad DHT table class or index");
                if (i + 17 > len) return bad("truncated DHT segment");
                JdHuffSrc &t = hs[tc][th];
                int cnt = 0;
                for (int l = 1; l <= 16; l++) { t.bits[l] = s[i + l]; cnt += s[i + l]; }
                if (cnt > 256 || i + 17 + cnt > len) return bad("bad DHT symbol count");
                memset(t.vals, 0, sizeof t.vals);
                memcpy(t.vals, s + i + 17, cnt);
                t.count = cnt;
                if (tc == 0)
                    for (int v = 0; v < cnt; v++) if (t.vals[v] > 15) return bad("DC Huffman symbol above 15");
                aej_jpegdec_huff tmp;
                if (!jd_build_huff(t, tmp)) return bad("over-subscribed Huffman table");
                t.defined = true;
                i += 17 + cnt;
            }
            break;
        }
        case 0xDB: {
            unsigned i = 0;
            while (i < len) {
                const int pq = s[i] >> 4, tq = s[i] & 15;
                if (pq > 1 || tq > 3) return bad("bad DQT precision or index");
                const unsigned need = 1 + 64u * (pq + 1);
                if (i + need > len) return bad("truncated DQT segment");
                for (int z = 0; z < 64; z++)
                    qt[tq][jd_natural(z)] = pq ? (uint16_t)(s[i + 1 + 2 * z] << 8 | s[i + 2 + 2 * z]) : s[i + 1 + z];
                qdef[tq] = true;
                q16[tq] = pq == 1;
                i += need;
            }
            break;
        }
        case 0xDD:
            if (len != 2) return bad("bad DRI length");
            ri = s[0] << 8 | s[1];
            break;
        case 0xE0:
            if (len >= 5 && !memcmp(s, "JFIF\0", 5)) jfif = true;
            break;
        case 0xEE:
            if (len >= 12 && !memcmp(s, "Adobe", 5)) { adobe = true; adobe_transform = s[11]; }
            break;
        case 0xDA: {
            if (!sof) return bad("SOS before SOF");
            const std::string at = "scan " + std::to_string(scans.size()) + ": ";
            if (len < 1) return bad("truncated SOS segment");
            const int ns = s[0];
            if (ns < 1 || ns > 4 || len != 4u + 2u * ns) return bad(at + "SOS length does not match its component count");
            if (scans.empty() && nf == 3) {
                const bool rgb_ids = f.comp_id[0] == 'R' && f.comp_id[1] == 'G' && f.comp_id[2] == 'B';
                if (!jfif && adobe && adobe_transform == 0) return unsup("Adobe APP14 transform 0 (RGB colour)");
                if (!jfif && !adobe && rgb_ids) return unsup("component ids 'R','G','B' without JFIF (RGB colour)");
            }
            aej_jpegprog_scan sc;
            memset(&sc, 0, sizeof sc);
            sc.ncomp = ns;
            for (int i = 0; i < ns; i++) {
                int c = -1;
                for (int j = 0; j < nf; j++) if (f.comp_id[j] == s[1 + 2 * i]) c = j;
                if (c < 0) return bad(at + "a component the frame does not have");
                if (i > 0 && c <= sc.comp[i - 1]) return bad(at + "components out of the frame's order");
                sc.comp[i] = c;
                sc.td[i] = s[2 + 2 * i] >> 4;
                sc.ta[i] = s[2 + 2 * i] & 15;
                if (sc.td[i] > 3 || sc.ta[i] > 3) return bad(at + "bad Huffman table selector");
            }
            sc.ss = s[1 + 2 * ns]; sc.se = s[2 + 2 * ns]; sc.ah = s[3 + 2 * ns] >> 4; sc.al = s[3 + 2 * ns] & 15;
            if (sc.ss > sc.se || sc.se > 63) return bad(at + "spectral selection " + std::to_string(sc.ss) + ".." + std::to_string(sc.se));
            if (sc.ss == 0 && sc.se != 0) return bad(at + "a DC scan with Se != 0");
            if (sc.ss > 0 && ns != 1) return bad(at + "an AC scan with " + std::to_string(ns) + " components");
            if (sc.al > 13) return bad(at + "Al " + std::to_string(sc.al) + " above 13");
            if (sc.ah != 0 && sc.al != sc.ah - 1) return bad(at + "a refinement with Al != Ah - 1");
            if (ns > 1 && ns != nf) return unsup(at + "an interleaved scan of " + std::to_string(ns) + " of " + std::to_string(nf) + " components");
            int level = 0;
            for (int i = 0; i < ns; i++) {
                const int c = sc.comp[i];
                if (sc.ss > 0 && coef_al[c][0] < 0) return bad(at + "an AC scan of a component before its DC scan");
                for (int k = sc.ss; k <= sc.se; k++) {
                    if (sc.ah == 0 && coef_al[c][k] >= 0) return bad(at + "a first scan of a coefficient already seen");
                    if (sc.ah != 0 && coef_al[c][k] != sc.ah)
                        return bad(at + "Ah " + std::to_string(sc.ah) + " is not the previous Al of coefficient " + std::to_string(k));
                    coef_al[c][k] = sc.al;
                    level = std::max(level, cell_level[c][k] + 1);
                }
                if (!qlatched[c]) {
                    const int tq = f.comp_tq[c];
                    if (!qdef[tq]) return bad("undefined quantisation table " + std::to_string(tq));
                    memcpy(f.qt[c], qt[tq], sizeof f.qt[c]);
                    f.precision16 |= q16[tq];
                    qlatched[c] = true;
                }
                if (sc.ss == 0 && sc.ah == 0) {
                    if (!hs[0][sc.td[i]].defined) return bad(at + "undefined Huffman table");
                    jd_build_huff(hs[0][sc.td[i]], sc.dc[i]);
                }
                if (sc.ss > 0) {
                    if (!hs[1][sc.ta[i]].defined) return bad(at + "undefined Huffman table");
                    jd_build_huff(hs[1][sc.ta[i]], sc.ac);
                }
            }
            for (int i = 0; i < ns; i++)
                for (int k = sc.ss; k <= sc.se; k++) cell_level[sc.comp[i]][k] = level;
            sc.level = level;
            f.n_levels = std::max(f.n_levels, level + 1);
            sc.restart_interval = ri;
            jp_scan_units(f, ns, sc.comp[0], sc.units_x, sc.units_y);
            const long long units = (long long)sc.units_x * sc.units_y;
            sc.n_segments = ri ? (int)((units + ri - 1) / ri) : 1;
            unsigned long long q = p + L;
            sc.data_offset = (long long)q;
            for (;;) {                                   // the scan ends at the first marker that is not RSTn
                if (q >= n) return bad(at + "the scan runs past the end of the file (no EOI marker)");
                if (b[q] != 0xFF) { q++; continue; }
                if (q + 1 >= n) return bad(at + "the scan runs past the end of the file (no EOI marker)");
                const int x = b[q + 1];
                if (x == 0xFF) { q++; continue; }
                if (x == 0x00 || (x >= 0xD0 && x <= 0xD7)) { q += 2; continue; }
                break;
            }
            sc.data_length = (long long)q - sc.data_offset;
            scans.push_back(sc);
            p = q;
            continue;
        }
        default:
            break;                                   // APPn, COM, JPGn, ...
        }
        p += L;
    }
    if (!sof) return bad("EOI before SOF");
    if (scans.empty()) return bad("EOI before SOS");
    for (int c = 0; c < nf; c++)
        for (int k = 0; k < 64; k++)
            if (coef_al[c][k] != 0)
                return unsup("incomplete progression: coefficient " + std::to_string(k) + " of component " + std::to_string(c) +
                             (coef_al[c][k] < 0 ? " never arrives" : " stops at Al " + std::to_string(coef_al[c][k])) +
                             " (libjpeg-turbo would smooth between blocks)");
    f.n_scans = (int)scans.size();
    return 0;
}

// ---- host: validation, layout, launch sequence -----------------------------------------------------------------------------------------
static long long jp_align(long long v, long long a) { return (v + a - 1) / a * a; }

// Everything the kernels index with is recomputed or checked here; the dependency levels are derived again rather than trusted.
bool jpegprog_layout(const aej_jpegprog_frame *frames, const aej_jpegprog_scan *scans_in, int n, JpLayout &y)
{
    y = JpLayout{};
    if (!frames || !scans_in || n < 1) return false;
    y.ffiles.assign(n, JdFile{});
    y.fdescs.resize(n);
    struct Ref { int level, file, idx; const aej_jpegprog_scan *s; };
    std::vector<Ref> order;
    long long s0 = 0;
    for (int i = 0; i < n; i++) {
        const aej_jpegprog_frame &f = frames[i];
        const bool color = f.ncomp == 3 && ((f.hs == 1 && f.vs == 1) || (f.hs == 2 && (f.vs == 1 || f.vs == 2)));
        if (!(color || (f.ncomp == 1 && f.hs == 1 && f.vs == 1))) return false;
        if (f.width < 1 || f.height < 1 || f.width > 65535 || f.height > 65535 || f.n_scans < 1 || f.n_scans > 4096) return false;
        if (f.mcux != (f.width + 8 * f.hs - 1) / (8 * f.hs) || f.mcuy != (f.height + 8 * f.vs - 1) / (8 * f.vs)) return false;
        if (f.blocks_per_mcu != (f.ncomp == 1 ? 1 : f.hs * f.vs + 2)) return false;
        aej_jpegdec_desc &d = y.fdescs[i];
        memset(&d, 0, sizeof d);
        d.width = f.width; d.height = f.height; d.ncomp = f.ncomp; d.hs = f.hs; d.vs = f.vs; d.mcux = f.mcux; d.mcuy = f.mcuy;
        d.blocks_per_mcu = f.blocks_per_mcu; d.n_segments = 1; d.sof = f.sof; d.precision16 = f.precision16;
        memcpy(d.qt, f.qt, sizeof d.qt);
        JdFile &F = y.ffiles[i];
        F.blk_base = y.fz.blocks;
        F.n_blocks = (long long)f.mcux * f.mcuy * f.blocks_per_mcu;
        y.fz.blocks += F.n_blocks;
        F.pw0 = f.mcux * 8 * f.hs; F.ph0 = f.mcuy * 8 * f.vs;
        F.pw1 = f.ncomp == 3 ? f.mcux * 8 : 0; F.ph1 = f.ncomp == 3 ? f.mcuy * 8 : 0;
        F.plane_off = y.fz.planes;
        y.fz.planes += jp_align((long long)F.pw0 * F.ph0 + 2LL * F.pw1 * F.ph1, 256);
        F.px_base = y.fz.px;
        y.fz.px += (long long)f.width * f.height;
        int cell_level[3][64];
        for (int c = 0; c < 3; c++) for (int k = 0; k < 64; k++) cell_level[c][k] = -1;
        for (int j = 0; j < f.n_scans; j++) {
            const aej_jpegprog_scan &s = scans_in[s0 + j];
            if (s.ncomp < 1 || s.ncomp > f.ncomp || (s.ncomp > 1 && s.ncomp != f.ncomp)) return false;
            for (int k = 0; k < s.ncomp; k++)
                if (s.comp[k] < 0 || s.comp[k] >= f.ncomp || (s.ncomp > 1 && s.comp[k] != k)) return false;
            if (s.ss < 0 || s.ss > s.se || s.se > 63 || (s.ss == 0 && s.se != 0) || (s.ss > 0 && s.ncomp != 1)) return false;
            if (s.al < 0 || s.al > 13 || s.ah < 0 || s.ah > 14 || s.restart_interval < 0 || s.data_length < 0) return false;
            int ux, uy;
            jp_scan_units(f, s.ncomp, s.comp[0], ux, uy);
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
        F.scan_len = s.data_length;
        F.clean_off = y.sz.clean;
        y.sz.clean += jp_align(s.data_length, 4) + 16;
        F.chunk_base = y.sz.chunks;
        F.n_chunks = (s.data_length + kJdChunk - 1) / kJdChunk;
        y.sz.chunks += F.n_chunks;
        F.seg_base = y.sz.segs;
        y.sz.segs += s.n_segments;
        F.slot_base = y.sz.slots;
        F.n_slots = s.n_segments + (s.data_length * 8 + kJpUnstuffS - 1) / kJpUnstuffS + 1;
        y.sz.slots += F.n_slots;
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
        const long long work = o.kind == kJpDcRefine ? (long long)s.units_x * s.units_y : s.n_segments;
        for (long long first = 0; first < work; first += kJpItem) y.items.push_back(JpItem{ t, (int)first });
        y.level_items[o.level + 1] = (long long)y.items.size();
    }
    for (int l = 1; l <= y.n_levels; l++) y.level_items[l] = std::max(y.level_items[l], y.level_items[l - 1]);
    return true;
}

unsigned long long jpegprog_carve(void *base, const JpLayout &y, JpBufs &w)
{
    unsigned long long off = 0;
    auto take = [&](unsigned long long bytes) { void *p = base ? (char *)base + off : nullptr; off += (bytes + 255) / 256 * 256; return p; };
    const size_t ns = y.scans.size(), nf = y.ffiles.size();
    w.blob = take(jpegprog_blob(y, nullptr));
    char *q = (char *)w.blob;
    auto part = [&](size_t bytes) { char *r = q; if (q) q += (bytes + 255) / 256 * 256; return (void *)r; };
    w.s.files = (JdFile *)part(sizeof(JdFile) * ns);
    w.s.descs = (aej_jpegdec_desc *)part(sizeof(aej_jpegdec_desc) * ns);
    w.scans = (JpScan *)part(sizeof(JpScan) * ns);
    w.items = (JpItem *)part(sizeof(JpItem) * y.items.size());
    w.f.files = (JdFile *)part(sizeof(JdFile) * nf);
    w.f.descs = (aej_jpegdec_desc *)part(sizeof(aej_jpegdec_desc) * nf);
    w.s.cnt = (int *)take(y.sz.chunks * 3 * 4);
    w.s.pre = (long long *)take(y.sz.chunks * 3 * 8);
    w.s.clean_len = (long long *)take(ns * 8);
    w.s.segs = (JdSeg *)take(y.sz.segs * sizeof(JdSeg));
    w.s.clean = (unsigned char *)take(y.sz.clean);
    w.sstatus = (int *)take(ns * 4);
    w.f.coef = (short *)take(y.fz.blocks * 128);
    w.f.planes = (unsigned char *)take(y.fz.planes);
    return off;
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
        if (hi > lo)
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
    if (!jpegprog_layout(&frame, scans_in, 1, y)) return AEJ_ERR_ARG;
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
