// jpegparse.hip -- the marker walk of both JPEG decoders (aej_jpegdec_parse_host, aej_jpegprog_parse_host).  Host code only.
// JpgParse holds what a file's markers have said so far and reads every segment the two kinds of file share: the frame header, DHT,
// DQT, DRI, JFIF APP0, Adobe APP14 and the frame types nobody decodes here.  The two entry points keep what is their own:
//   jpegdec_parse    SOF0 / SOF1: the rules of the one sequential scan, its tables, where its bytes lie
//   jpegprog_parse   SOF2: the scan script (T.81 G.1.1.1), dependency levels, tables latched per scan, each scan's bytes up to EOI
// Both fill a descriptor that is all zero before the call; after a refusal it holds what had been read up to there.
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "aej_common.h"
#include "aej_launch.h"

namespace aej {

// libjpeg's jpeg_make_d_derived_tbl: canonical codes, over-subscription check, then the decode tables
bool jd_build_huff(const JdHuffSrc &s, aej_jpegdec_huff &h)
{
    memset(&h, 0, sizeof h);
    int size[257], code[257], p = 0;
    for (int l = 1; l <= 16; l++)
        for (int i = 0; i < s.bits[l]; i++) size[p++] = l;
    size[p] = 0;
    int c = 0, si = size[0];
    p = 0;
    while (size[p]) {
        while (size[p] == si) code[p++] = c++;
        if (c >= (1 << si)) return false;
        c <<= 1;
        si++;
    }
    p = 0;
    for (int l = 1; l <= 16; l++) {
        if (s.bits[l]) {
            h.valoff[l] = p - code[p];
            p += s.bits[l];
            h.maxcode[l] = code[p - 1];
        } else {
            h.maxcode[l] = -1;
        }
    }
    h.maxcode[17] = -1;
    memcpy(h.vals, s.vals, sizeof h.vals);
    p = 0;
    for (int l = 1; l <= 9; l++)
        for (int i = 0; i < s.bits[l]; i++, p++) {
            const int lo = code[p] << (9 - l);
            for (int e = 0; e < (1 << (9 - l)); e++) h.lut[lo + e] = (uint16_t)((l << 8) | s.vals[p]);
        }
    return true;
}

namespace {

enum { kJpgSegment, kJpgEOI, kJpgEndOfFile, kJpgStrayBytes, kJpgEndInMarker };      // JpgParse::next; a refusal is its negative AEJ_ERR_*

struct JpScript {                      // what the scans so far have done to each (component, coefficient) cell; -1: nothing yet
    int coef_al[4][64], cell_level[4][64];
    bool qlatched[4] = {};
    JpScript() { memset(coef_al, -1, sizeof coef_al); memset(cell_level, -1, sizeof cell_level); }
};

struct JpgParse {
    const unsigned char *b;
    unsigned long long n, p = 2;       // the file; where the next marker is expected
    std::string &msg;
    // the marker in hand (next): its payload, and where the segment ends
    int m = 0;
    const unsigned char *s = nullptr;
    unsigned len = 0;
    unsigned long long end = 0;
    // tables and settings in force
    uint16_t qt[4][64];
    bool qdef[4] = {}, q16[4] = {};
    JdHuffSrc huff[2][4];
    int ri = 0;
    bool jfif = false, adobe = false;
    int adobe_transform = -1;
    // the frame: aej_jpegprog_frame has every frame field of aej_jpegdec_desc (store)
    aej_jpegprog_frame f = {};
    bool sof = false;
    int nf = 0;                        // components the frame header lists
    bool allow440 = false;             // the caller takes luma sampled 1 x 2 over 1 x 1 chroma (4:4:0) too: the _440 entries
    bool allow_adobe = false;          // the caller takes four components and RGB-coded files too (the _adobe entries): x says what the file is
    aej_jpeg_adobe x = {};

    JpgParse(const unsigned char *data, unsigned long long bytes, std::string &m_) : b(data), n(bytes), msg(m_) {}
    int bad(const std::string &t) { msg = t; return (int)AEJ_ERR_ARG; }
    int unsup(const std::string &t) { msg = t; return (int)AEJ_ERR_UNSUPPORTED; }
    bool soi() const { return b && n >= 4 && b[0] == 0xFF && b[1] == 0xD8; }

    // The next marker that is not TEM or RSTn, fill bytes skipped.  kJpgSegment: m, s, len and end are set; kJpgEOI; the three ways a
    // file can stop, which each parser words itself.
    int next()
    {
        for (;;) {
            if (p >= n) return kJpgEndOfFile;
            if (b[p] != 0xFF) return kJpgStrayBytes;
            while (p < n && b[p] == 0xFF) p++;
            if (p >= n) return kJpgEndInMarker;
            m = b[p++];
            if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
            if (m == 0xD8) return bad("second SOI marker");
            if (m == 0xD9) return kJpgEOI;
            if (p + 2 > n) return bad("truncated marker segment");
            const unsigned L = (unsigned)b[p] << 8 | b[p + 1];
            if (L < 2 || p + L > n) return bad("truncated marker segment");
            s = b + p + 2;
            len = L - 2;
            end = p + L;
            return kJpgSegment;
        }
    }

    // the frame header of the marker in hand.  A progressive file's scans name their components, so two with one id are refused, and
    // its sampling is checked here; the baseline parser checks it at SOS.
    int frame(bool progressive)
    {
        if (sof) return bad("two SOF markers");
        if (len < 6) return bad("truncated SOF segment");
        if (s[0] != 8) return unsup("sample precision " + std::to_string(s[0]) + " (only 8-bit)");
        f.height = s[1] << 8 | s[2];
        f.width = s[3] << 8 | s[4];
        nf = s[5];
        if (len != 6u + 3u * nf) return bad("SOF length does not match its component count");
        if (f.height == 0) return unsup("DNL (height defined after the scan)");
        if (f.width == 0) return bad("zero image width");
        if (nf != 1 && nf != 3 && !(allow_adobe && nf == 4)) return unsup(std::to_string(nf) + " components (only 1 or 3)");
        for (int i = 0; i < nf; i++) {
            f.comp_id[i] = s[6 + 3 * i];
            f.comp_h[i] = s[7 + 3 * i] >> 4;
            f.comp_v[i] = s[7 + 3 * i] & 15;
            f.comp_tq[i] = s[8 + 3 * i];
            if (f.comp_h[i] < 1 || f.comp_h[i] > 4 || f.comp_v[i] < 1 || f.comp_v[i] > 4 || f.comp_tq[i] > 3)
                return bad("bad component sampling factor or table index");
            for (int j = 0; progressive && j < i; j++) if (f.comp_id[j] == f.comp_id[i]) return bad("two frame components with one id");
        }
        if (progressive) {
            const int rc = sampling();
            if (rc) return rc;
            f.ncomp = nf;
        }
        f.sof = m;
        sof = true;
        return 0;
    }

    int dht()
    {
        unsigned i = 0;
        while (i < len) {
            const int tc = s[i] >> 4, th = s[i] & 15;
            if (tc > 1 || th > 3) return bad("bad DHT table class or index");
            if (i + 17 > len) return bad("truncated DHT segment");
            JdHuffSrc &t = huff[tc][th];
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
        return 0;
    }

    int dqt()
    {
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
        return 0;
    }

    int dri()
    {
        if (len != 2) return bad("bad DRI length");
        ri = s[0] << 8 | s[1];
        return 0;
    }
    void app0() { if (len >= 5 && !memcmp(s, "JFIF\0", 5)) jfif = true; }
    void app14() { if (len >= 12 && !memcmp(s, "Adobe", 5)) { adobe = true; adobe_transform = s[11]; } }

    // every segment but SOS: the frame header of this parser's kind, the tables and settings, the frame types and markers neither
    // decoder takes; anything else (APPn, COM, JPGn, ...) is passed over
    int segment(bool progressive)
    {
        switch (m) {
        case 0xC0: case 0xC1: return progressive ? unsup("not a progressive file (SOF" + std::to_string(m - 0xC0) + ")") : frame(false);
        case 0xC2: return progressive ? frame(true) : unsup("progressive JPEG (SOF2)");
        case 0xC3: return unsup("lossless JPEG (SOF3)");
        case 0xC5: case 0xC6: case 0xC7: return unsup("hierarchical JPEG (SOF" + std::to_string(m - 0xC0) + ")");
        case 0xC9: case 0xCA: case 0xCB: case 0xCD: case 0xCE: case 0xCF: case 0xCC:
            return unsup("arithmetic coding (" + std::string(m == 0xCC ? "DAC" : "SOF" + std::to_string(m - 0xC0)) + ")");
        case 0xDC: return unsup("DNL marker");
        case 0xC4: return dht();
        case 0xDB: return dqt();
        case 0xDD: return dri();
        case 0xE0: app0(); return 0;
        case 0xEE: app14(); return 0;
        default: return 0;
        }
    }

    // reads on to the next SOS (kJpgSegment, the SOS in hand) or to where next() stops
    int to_scan(bool progressive)
    {
        for (;;) {
            int k = next();
            if (k != kJpgSegment || m == 0xDA || (k = segment(progressive)) != 0) return k;
            p = end;
        }
    }

    // three components are YCbCr unless the file says RGB; four (allow_adobe alone) are CMYK unless APP14 says YCCK: libjpeg's
    // default_decompress_parms.  With allow_adobe the two RGB refusals become x.colour.
    int colour_rule()
    {
        if (nf == 4) {
            if (adobe && adobe_transform != 0 && adobe_transform != 2)
                return unsup("Adobe APP14 transform " + std::to_string(adobe_transform) + " in a four-component file (libjpeg reads it as YCCK with a warning)");
            x.colour = adobe && adobe_transform == 2 ? AEJ_JPEG_YCCK : AEJ_JPEG_CMYK;
            return 0;
        }
        if (nf != 3) return 0;
        const bool rgb_ids = f.comp_id[0] == 'R' && f.comp_id[1] == 'G' && f.comp_id[2] == 'B';
        if (!jfif && adobe && adobe_transform == 0) {
            if (!allow_adobe) return unsup("Adobe APP14 transform 0 (RGB colour)");
            x.colour = AEJ_JPEG_RGB;
        }
        if (!jfif && !adobe && rgb_ids) {
            if (!allow_adobe) return unsup("component ids 'R','G','B' without JFIF (RGB colour)");
            x.colour = AEJ_JPEG_RGB;
        }
        return 0;
    }

    // 4:4:4, 4:2:2 or 4:2:0, with allow440 also 4:4:0 (one component: a non-interleaved scan, whatever its sampling factors say) and
    // the MCU grid
    int sampling()
    {
        if (nf == 3 || nf == 4) {
            const int h0 = f.comp_h[0], v0 = f.comp_v[0], h3 = f.comp_h[3], v3 = f.comp_v[3];
            if (f.comp_h[1] != 1 || f.comp_v[1] != 1 || f.comp_h[2] != 1 || f.comp_v[2] != 1 ||
                !((h0 == 1 && v0 == 1) || (h0 == 2 && v0 == 1) || (h0 == 2 && v0 == 2) || (allow440 && h0 == 1 && v0 == 2)) ||
                (nf == 4 && !((h3 == h0 && v3 == v0) || (h3 == 1 && v3 == 1))))      // component 3: component 0's factors, or 1 x 1
                return unsup("sampling factors " + std::to_string(h0) + "x" + std::to_string(v0) + "," + std::to_string(f.comp_h[1]) + "x" +
                             std::to_string(f.comp_v[1]) + "," + std::to_string(f.comp_h[2]) + "x" + std::to_string(f.comp_v[2]) +
                             (nf == 4 ? "," + std::to_string(h3) + "x" + std::to_string(v3) : std::string()));
            f.hs = h0; f.vs = v0;
            f.blocks_per_mcu = h0 * v0 + 2;
            if (nf == 4) { x.h3 = h3; x.v3 = v3; x.tq3 = f.comp_tq[3]; f.blocks_per_mcu += h3 * v3; }
        } else {
            f.hs = f.vs = 1;
            f.blocks_per_mcu = 1;
        }
        f.mcux = (f.width + 8 * f.hs - 1) / (8 * f.hs);
        f.mcuy = (f.height + 8 * f.vs - 1) / (8 * f.vs);
        return 0;
    }

    int undefined_qt(int c) { return bad("undefined quantisation table " + std::to_string(f.comp_tq[c])); }
    void latch_qt(int c)               // component c takes the table its frame entry names, as it stands now (component 3: in x)
    {
        memcpy(c == 3 ? x.qt3 : f.qt[c], qt[f.comp_tq[c]], sizeof f.qt[0]);
        f.precision16 |= q16[f.comp_tq[c]];
    }

    void store(aej_jpegdec_desc &d) const
    {
        d.width = f.width; d.height = f.height; d.ncomp = f.ncomp; d.hs = f.hs; d.vs = f.vs; d.mcux = f.mcux; d.mcuy = f.mcuy;
        d.blocks_per_mcu = f.blocks_per_mcu; d.sof = f.sof; d.precision16 = f.precision16;
        memcpy(d.comp_id, f.comp_id, 4); memcpy(d.comp_h, f.comp_h, 4); memcpy(d.comp_v, f.comp_v, 4); memcpy(d.comp_tq, f.comp_tq, 4);
        memcpy(d.qt, f.qt, sizeof d.qt);
    }

    // ---- baseline: the markers up to the one scan -------------------------------------------------------------------------------------------
    int baseline(aej_jpegdec_desc &d)
    {
        if (!soi()) return bad("not a JPEG file (no SOI marker)");
        int rc = to_scan(false);
        if (rc < 0) return rc;
        if (rc == kJpgStrayBytes) return bad("bytes between markers in the header");
        if (rc != kJpgSegment) return bad(rc == kJpgEOI ? "EOI before SOS" : "no SOS marker (the file ends in its header)");
        if (!sof) return bad("SOS before SOF");
        if (len < 1) return bad("truncated SOS segment");
        const int ns = s[0];
        if (len != 4u + 2u * ns || ns < 1) return bad("SOS length does not match its component count");
        if (ns < nf)
            return unsup("multi-scan sequential JPEG (the first scan holds " + std::to_string(ns) + " of " + std::to_string(nf) + " components)");
        if (ns != nf) return bad("SOS lists more components than the frame");
        for (int i = 0; i < ns; i++)
            if (s[1 + 2 * i] != f.comp_id[i]) return unsup("scan components in another order than the frame's");
        if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0)
            return bad("bad spectral selection / approximation for a sequential scan");
        if ((rc = colour_rule()) || (rc = sampling())) return rc;
        for (int i = 0; i < nf; i++) {
            const int td = s[2 + 2 * i] >> 4, ta = s[2 + 2 * i] & 15;
            if (!qdef[f.comp_tq[i]]) return undefined_qt(i);
            if (td > 3 || ta > 3 || !huff[0][td].defined || !huff[1][ta].defined) return bad("undefined Huffman table");
            latch_qt(i);
            jd_build_huff(huff[0][td], i == 3 ? x.dc3 : d.dc[i]);
            jd_build_huff(huff[1][ta], i == 3 ? x.ac3 : d.ac[i]);
        }
        const long long mcus = (long long)f.mcux * f.mcuy;
        d.restart_interval = ri;
        d.n_segments = ri ? (int)((mcus + ri - 1) / ri) : 1;
        f.ncomp = nf;
        d.scan_offset = (long long)end;
        d.scan_length = (long long)(n - end);
        return 0;
    }

    // ---- progressive: every marker up to EOI ---------------------------------------------------------------------------------------------------
    // the SOS in hand and the scan's bytes after it; leaves p at the marker that ends the scan
    int progressive_scan(JpScript &S, std::vector<aej_jpegprog_scan> &scans)
    {
        if (!sof) return bad("SOS before SOF");
        const std::string at = "scan " + std::to_string(scans.size()) + ": ";
        if (len < 1) return bad("truncated SOS segment");
        const int ns = s[0];
        if (ns < 1 || ns > 4 || len != 4u + 2u * ns) return bad(at + "SOS length does not match its component count");
        if (scans.empty()) {
            const int rc = colour_rule();
            if (rc) return rc;
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
            if (sc.ss > 0 && S.coef_al[c][0] < 0) return bad(at + "an AC scan of a component before its DC scan");
            for (int k = sc.ss; k <= sc.se; k++) {
                if (sc.ah == 0 && S.coef_al[c][k] >= 0) return bad(at + "a first scan of a coefficient already seen");
                if (sc.ah != 0 && S.coef_al[c][k] != sc.ah)
                    return bad(at + "Ah " + std::to_string(sc.ah) + " is not the previous Al of coefficient " + std::to_string(k));
                S.coef_al[c][k] = sc.al;
                level = std::max(level, S.cell_level[c][k] + 1);
            }
            if (!S.qlatched[c]) {
                if (!qdef[f.comp_tq[c]]) return undefined_qt(c);
                latch_qt(c);
                S.qlatched[c] = true;
            }
            if (sc.ss == 0 && sc.ah == 0) {
                if (!huff[0][sc.td[i]].defined) return bad(at + "undefined Huffman table");
                jd_build_huff(huff[0][sc.td[i]], i == 3 ? x.dc3 : sc.dc[i]);
            }
            if (sc.ss > 0) {
                if (!huff[1][sc.ta[i]].defined) return bad(at + "undefined Huffman table");
                jd_build_huff(huff[1][sc.ta[i]], sc.ac);
            }
        }
        for (int i = 0; i < ns; i++)
            for (int k = sc.ss; k <= sc.se; k++) S.cell_level[sc.comp[i]][k] = level;
        sc.level = level;
        f.n_levels = std::max(f.n_levels, level + 1);
        sc.restart_interval = ri;
        jp_scan_units(f, ns, sc.comp[0], sc.units_x, sc.units_y, &x);
        const long long units = (long long)sc.units_x * sc.units_y;
        sc.n_segments = ri ? (int)((units + ri - 1) / ri) : 1;
        unsigned long long q = end;
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
        return 0;
    }

    int progressive(std::vector<aej_jpegprog_scan> &scans)
    {
        if (!soi()) return bad("not a JPEG file (no SOI marker)");
        JpScript S;
        for (;;) {
            int rc = to_scan(true);
            if (rc == kJpgSegment) rc = progressive_scan(S, scans);      // leaves p behind the scan's bytes
            if (rc < 0) return rc;
            if (rc == kJpgEOI) break;
            if (rc == kJpgEndOfFile) return bad("no EOI marker (the file ends after " + std::to_string(scans.size()) + " scans)");
            if (rc == kJpgStrayBytes) return bad("bytes between markers");
            if (rc == kJpgEndInMarker) return bad("no EOI marker (the file ends in a marker)");
        }
        if (!sof) return bad("EOI before SOF");
        if (scans.empty()) return bad("EOI before SOS");
        for (int c = 0; c < nf; c++)
            for (int k = 0; k < 64; k++)
                if (S.coef_al[c][k] != 0)
                    return unsup("incomplete progression: coefficient " + std::to_string(k) + " of component " + std::to_string(c) +
                                   (S.coef_al[c][k] < 0 ? " never arrives" : " stops at Al " + std::to_string(S.coef_al[c][k])) +
                                   " (libjpeg-turbo would smooth between blocks)");
        f.n_scans = (int)scans.size();
        return 0;
    }
};

}  // namespace

int jpegdec_parse(const unsigned char *b, unsigned long long n, aej_jpegdec_desc &d, std::string &msg, bool allow440, aej_jpeg_adobe *adobe)
{
    memset(&d, 0, sizeof d);
    JpgParse P(b, n, msg);
    P.allow440 = allow440;
    P.allow_adobe = adobe != nullptr;
    const int rc = P.baseline(d);
    P.store(d);
    if (adobe) *adobe = P.x;
    return rc;
}

int jpegprog_parse(const unsigned char *b, unsigned long long n, aej_jpegprog_frame &f, std::vector<aej_jpegprog_scan> &scans, std::string &msg,
                   bool allow440, aej_jpeg_adobe *adobe)
{
    scans.clear();
    JpgParse P(b, n, msg);
    P.allow440 = allow440;
    P.allow_adobe = adobe != nullptr;
    const int rc = P.progressive(scans);
    f = P.f;
    if (adobe) *adobe = P.x;
    return rc;
}

}  // namespace aej
