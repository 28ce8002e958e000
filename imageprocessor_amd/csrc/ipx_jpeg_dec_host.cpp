// ipx_jpeg_dec_host.cpp -- the host part of image.Decode for JPEGs: marker parsing and table preparation.
//
// The reference decodes every upload with image.Decode (image_processor.go:47); for JPEG files that is Go's image/jpeg
// (reader.go: decode, processSOF, processDHT, processDQT, processDRI, processSOS; Go 1.24 stdlib, go.mod:3).  The
// entropy decoding and the inverse transform run on the GPU (ipx_jpeg_dec.hip); what stays here is what is serial and
// tiny: walk the markers, collect the tables the single scan refers to, and lay them out the way the kernels read them
// (an 8-bit first-level Huffman table plus the canonical mincode / maxcode arrays for longer codes; quantisers
// de-zig-zagged).  Anything outside the baseline subset the kernels implement is reported as IPX_ERR_UNSUPPORTED for
// that image, so that the worker keeps Go's CPU path for it: CMYK / RGB (Adobe) files (four-component files are taken under
// IPX_JPEG_CMYK=1: ipx_jpeg_dec_cmyk.hip), sampling factors Go's processSOF refuses (4:1:1 / 4:1:0, which it takes, are taken under IPX_JPEG_411=1), 12-bit samples.  Progressive files, files coded in several scans and Huffman table ids above 1 are marked host_scans: their
// scans are decoded on the host (ipx_jpeg_dec_prog.cpp) and only the transform onwards runs on the GPU.  A file has to end the way
// Go's marker loop wants it to (EOI after the last scan), or it is malformed here as it is there.
#include <algorithm>
#include <chrono>
#include <cstring>

#include "ipx_decode_common.h"

namespace ipx {

namespace {

const uint8_t kUnzig[64] = {
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct RawHuff { bool ok = false; uint8_t counts[16]; uint8_t vals[256]; int nvals = 0; };

inline uint32_t be16(const uint8_t *p) { return (uint32_t)p[0] << 8 | p[1]; }

// huffman.go's table, in the two forms the kernel uses
bool build_huff(const RawHuff &r, uint16_t lut[256], int32_t maxcode[18], int32_t valoff[18], uint8_t vals[256], uint32_t bound[8])
{
    memset(lut, 0, 256 * sizeof(uint16_t));
    memcpy(vals, r.vals, 256);
    int32_t code = 0, idx = 0;
    for (int len = 1; len <= 16; len++) {
        code <<= 1;
        const int cnt = r.counts[len - 1];
        if (cnt == 0) { maxcode[len] = -1; valoff[len] = 0; if (len >= 9) bound[len - 9] = (uint32_t)code << (16 - len); continue; }
        if (code + cnt > (1 << len)) return false;            // "bad Huffman table": more codes than the length can hold
        valoff[len] = idx - code;                              // symbol index = valoff + code
        if (len <= 8)
            for (int k = 0; k < cnt; k++) {
                const int c = code + k, sym = r.vals[idx + k];
                for (int fill = 0; fill < (1 << (8 - len)); fill++) lut[(c << (8 - len)) | fill] = (uint16_t)(len << 8 | sym);
            }
        code += cnt; idx += cnt;
        maxcode[len] = code - 1;
        if (len >= 9) bound[len - 9] = (uint32_t)code << (16 - len);   // canonical codes: a 16-bit window below this has a code of at most len bits
    }
    maxcode[0] = -1; valoff[0] = 0; maxcode[17] = 0x7fffffff; valoff[17] = 0;
    return true;
}

}  // namespace

// 0 ok; IPX_ERR_INVALID malformed; IPX_ERR_UNSUPPORTED a valid file outside the GPU subset
// cmyk (IPX_JPEG_CMYK=1, ipx_jpeg_dec_cmyk.hip): a four-component frame with one of the two sampling vectors Go's processSOF takes is
// IPX_OK with ncomp 4 and host_scans set -- its tables and scans are the host decoder's alone -- instead of IPX_ERR_UNSUPPORTED
// s411 (IPX_JPEG_411=1): a three-component frame with Y (4,1) or (4,2) and 1x1 chroma is IPX_OK with h0 = 4 and ratio IPX_YCBCR_411 / _410
int jpeg_parse(const uint8_t *d, size_t len, JpegDecInfo *info, JpegDecTables *tab, bool cmyk, bool s411)
{
    memset(info, 0, sizeof *info);
    if (len < 4 || d[0] != 0xff || d[1] != 0xd8) return IPX_ERR_INVALID;
    uint16_t quant[4][64];
    memset(quant, 0, sizeof quant);                            // a table no DQT defined is all zero in Go's decoder, and the file decodes (to flat grey)
    RawHuff hf[2][4];
    int ncomp = 0, ch[4] = {0, 0, 0, 0}, cv[4] = {0, 0, 0, 0}, ctq[4] = {0, 0, 0, 0}, cid[4] = {0, 0, 0, 0};
    bool jfif = false, adobe = false;
    int adobe_transform = 0;
    size_t i = 2;
    for (;;) {
        if (i + 2 > len) return IPX_ERR_INVALID;
        if (d[i] != 0xff) { i++; continue; }                   // decode(): bytes that belong to no segment are skipped ("libjpeg is liberal")
        while (i + 1 < len && d[i + 1] == 0xff) i++;
        if (i + 2 > len) return IPX_ERR_INVALID;
        const int m = d[i + 1];
        i += 2;
        if (m == 0xd9) return IPX_ERR_INVALID;                 // "missing SOS marker"
        if (m == 0x00 || (m >= 0xd0 && m <= 0xd7)) continue;
        if (i + 2 > len) return IPX_ERR_INVALID;
        const size_t n = be16(d + i);
        if (n < 2 || i + n > len) return IPX_ERR_INVALID;
        const uint8_t *s = d + i + 2;
        const size_t sn = n - 2;
        switch (m) {
        case 0xc0: case 0xc1: case 0xc2: {
            if (m == 0xc2) info->host_scans = info->progressive = 1;   // progressive: the scans refine each other (ipx_jpeg_dec_prog.cpp)
            if (ncomp || sn < 6) return IPX_ERR_INVALID;
            if (s[0] != 8) return IPX_ERR_UNSUPPORTED;
            info->h = (int)be16(s + 1); info->w = (int)be16(s + 3);
            ncomp = s[5];
            if (ncomp == 4 && !cmyk) return IPX_ERR_UNSUPPORTED;
            if ((ncomp != 3 && ncomp != 1 && ncomp != 4) || sn != (size_t)(6 + 3 * ncomp) || info->w <= 0 || info->h <= 0) return IPX_ERR_INVALID;
            if ((long long)info->w * info->h > (1LL << 28)) return IPX_ERR_UNSUPPORTED;   // 268 Mpixel: beyond any batch this path is meant for
            for (int c = 0; c < ncomp; c++) {
                cid[c] = s[6 + 3 * c]; ch[c] = s[7 + 3 * c] >> 4; cv[c] = s[7 + 3 * c] & 15; ctq[c] = s[8 + 3 * c];
                if (ctq[c] > 3 || ch[c] < 1 || ch[c] > 4 || cv[c] < 1 || cv[c] > 4) return IPX_ERR_INVALID;
                for (int j = 0; j < c; j++) if (cid[j] == cid[c]) return IPX_ERR_INVALID;   // "repeated component identifier"
                // processSOF refuses a factor of 3 for every component, a single one included -- before it sets that one's (h, v) to (1, 1)
                // (found by tools/fuzz_corrupt.py: a Gray file whose V_1 a bit flip had made 3 decoded here and fails in Go)
                if (ch[c] == 3 || cv[c] == 3) return IPX_ERR_UNSUPPORTED;
            }
            if (ncomp == 1) { ch[0] = cv[0] = 1; break; }   // processSOF: a single component is non-interleaved, its (h, v) is effectively (1, 1)
            if (ncomp == 4) {
                // processSOF: (h, v) = 11 11 11 11 or 22 11 11 22, everything else is "unsupported subsampling ratio"
                if (ch[0] != cv[0] || ch[0] > 2 || ch[1] != 1 || cv[1] != 1 || ch[2] != 1 || cv[2] != 1 || ch[3] != ch[0] || cv[3] != cv[0]) return IPX_ERR_UNSUPPORTED;
                info->host_scans = 1;
                break;
            }
            // processSOF: Y (1|2)x(1|2), or (4,1) / (4,2), over 1x1 chroma; v = 4 and every other vector are "unsupported subsampling ratio"
            if (ch[1] != 1 || cv[1] != 1 || ch[2] != 1 || cv[2] != 1 || cv[0] > 2 || (ch[0] > 2 && !(s411 && ch[0] == 4))) return IPX_ERR_UNSUPPORTED;
            break;
        }
        case 0xc4: {
            size_t k = 0;
            while (k < sn) {
                if (k + 17 > sn) return IPX_ERR_INVALID;
                const int tc = s[k] >> 4, th = s[k] & 15;
                if (tc > 1 || th > 3) return IPX_ERR_INVALID;
                RawHuff &t = hf[tc][th];
                int total = 0;
                for (int b = 0; b < 16; b++) { t.counts[b] = s[k + 1 + b]; total += t.counts[b]; }
                if (total == 0 || total > 256 || k + 17 + (size_t)total > sn) return IPX_ERR_INVALID;
                memset(t.vals, 0, sizeof t.vals);
                memcpy(t.vals, s + k + 17, (size_t)total);
                t.nvals = total; t.ok = true;
                k += 17 + (size_t)total;
            }
            break;
        }
        case 0xdb: {
            size_t k = 0;
            while (k < sn) {
                const int pq = s[k] >> 4, tq = s[k] & 15;
                if (tq > 3 || pq > 1) return IPX_ERR_INVALID;
                const size_t need = pq ? 128 : 64;
                if (k + 1 + need > sn) return IPX_ERR_INVALID;
                for (int z = 0; z < 64; z++) quant[tq][z] = pq ? (uint16_t)be16(s + k + 1 + 2 * z) : s[k + 1 + z];
                k += 1 + need;
            }
            break;
        }
        case 0xdd:
            if (sn != 2) return IPX_ERR_INVALID;
            info->ri = (int)be16(s);
            break;
        case 0xe0: if (sn >= 5 && !memcmp(s, "JFIF\0", 5)) jfif = true; break;
        case 0xee: if (sn >= 12 && !memcmp(s, "Adobe", 5)) { adobe = true; adobe_transform = s[11]; } break;
        case 0xda: {
            if (!ncomp) return IPX_ERR_INVALID;
            if (sn < 1) return IPX_ERR_INVALID;
            info->h0 = ch[0]; info->v0 = cv[0];
            info->ncomp = ncomp;
            info->ratio = ncomp == 1 ? IPX_GRAY : ycbcr_ratio_of(ch[0], cv[0]);
            if (info->host_scans) return IPX_OK;               // the frame is known; the scans are the host decoder's
            if (s[0] != ncomp) {                               // a sequential frame coded in several scans
                if (s[0] < 1 || s[0] > 3) return IPX_ERR_INVALID;
                info->host_scans = 1;
                return IPX_OK;
            }
            if (sn != (size_t)(4 + 2 * ncomp)) return IPX_ERR_INVALID;
            int td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
            for (int c = 0; c < ncomp; c++) {
                if (s[1 + 2 * c] != cid[c]) { info->host_scans = 1; return IPX_OK; }           // components out of frame order
                td[c] = s[2 + 2 * c] >> 4; ta[c] = s[2 + 2 * c] & 15;
                if (td[c] > 3 || ta[c] > 3) return IPX_ERR_INVALID;
                if (td[c] > 1 || ta[c] > 1) { info->host_scans = 1; return IPX_OK; }           // extended sequential: four tables per class
                if (!hf[0][td[c]].ok || !hf[1][ta[c]].ok) return IPX_ERR_INVALID;   // "uninitialized Huffman table"
                info->td[c] = (uint8_t)td[c]; info->ta[c] = (uint8_t)(2 + ta[c]);   // kernel table slots: 0,1 = DC; 2,3 = AC
                // processSOS runs ONE block loop for sequential and progressive scans: an AC symbol (r < 15, s = 0) starts an end-of-band
                // run in a baseline file too, and the next blocks of the scan lose their AC part.  No encoder writes such a symbol into a
                // sequential file, the GPU decoder reads it as a plain EOB -- so a (damaged) table that holds one goes to the host decoder.
                const RawHuff &act = hf[1][ta[c]];
                for (int v = 0; v < act.nvals; v++)
                    if ((act.vals[v] & 15) == 0 && (act.vals[v] >> 4) != 0 && (act.vals[v] >> 4) != 15) { info->host_scans = 1; return IPX_OK; }
            }
            if (ncomp == 3 && !jfif && ((adobe && adobe_transform == 0) || (cid[0] == 'R' && cid[1] == 'G' && cid[2] == 'B'))) return IPX_ERR_UNSUPPORTED;
            info->scan_off = i + n;
            {
                // The scan ends at the first marker that is not a restart marker; what follows has to be what Go's marker loop accepts
                // up to EOI (decode() keeps reading segments until it sees one: a file that stops after its scan is
                // io.ErrUnexpectedEOF there, and a task the reference marks failed).  Another SOS makes it a multi-scan file.
                const uint8_t *sd = d + info->scan_off;
                const size_t rest = len - info->scan_off;
                size_t k = 0, end = rest;
                while (k + 1 < rest) {
                    const uint8_t *q = (const uint8_t *)memchr(sd + k, 0xff, rest - 1 - k);
                    if (!q) break;
                    k = (size_t)(q - sd);
                    const uint8_t m2 = sd[k + 1];
                    if (m2 == 0x00 || (m2 >= 0xd0 && m2 <= 0xd7)) { k += 2; continue; }
                    end = k;
                    break;
                }
                info->scan_len = end;
                size_t p = info->scan_off + end;
                for (;;) {                                     // the tail: Go's marker loop, segments skipped by their length
                    if (p + 2 > len) return IPX_ERR_INVALID;   // no EOI
                    if (d[p] != 0xff) { p++; continue; }       // bytes that belong to no segment are skipped
                    const int m3 = d[p + 1];
                    if (m3 == 0xff) { p++; continue; }         // fill byte
                    p += 2;
                    if (m3 == 0xd9) break;                     // EOI
                    if (m3 == 0x00 || (m3 >= 0xd0 && m3 <= 0xd7)) continue;
                    if (m3 == 0xda) { info->host_scans = 1; return IPX_OK; }
                    if (m3 == 0xc0 || m3 == 0xc1 || m3 == 0xc2) return IPX_ERR_INVALID;        // "multiple SOF markers"
                    if (!((m3 >= 0xe0 && m3 <= 0xef) || m3 == 0xfe || m3 == 0xc4 || m3 == 0xdb || m3 == 0xdd)) return m3 < 0xc0 ? IPX_ERR_INVALID : IPX_ERR_UNSUPPORTED;
                    if (p + 2 > len) return IPX_ERR_INVALID;
                    const size_t n3 = be16(d + p);
                    if (n3 < 2 || p + n3 > len) return IPX_ERR_INVALID;
                    p += n3;
                }
            }
            for (int tc = 0; tc < 2; tc++)
                for (int th = 0; th < 2; th++) {
                    const int slot = tc * 2 + th;
                    if (!hf[tc][th].ok) {
                        memset(tab->lut[slot], 0, sizeof tab->lut[slot]);
                        for (int l = 0; l < 18; l++) { tab->maxcode[slot][l] = -1; tab->valoff[slot][l] = 0; }
                        tab->maxcode[slot][17] = 0x7fffffff;
                        memset(tab->bound[slot], 0, sizeof tab->bound[slot]);
                        continue;
                    }
                    if (!build_huff(hf[tc][th], tab->lut[slot], tab->maxcode[slot], tab->valoff[slot], tab->vals[slot], tab->bound[slot])) return IPX_ERR_INVALID;
                }
            for (int c = 0; c < 3; c++)
                for (int zig = 0; zig < 64; zig++) tab->qnat[c][kUnzig[zig]] = c < ncomp ? quant[ctq[c]][zig] : 0;
            return IPX_OK;
        }
        default:          // APPn and COM are skipped; anything else is "unknown marker": a FormatError below SOF0, an UnsupportedError above
            if (!((m >= 0xe0 && m <= 0xef) || m == 0xfe)) return m < 0xc0 ? IPX_ERR_INVALID : IPX_ERR_UNSUPPORTED;
            break;
        }
        i += n;
    }
}

// ---- the host plan of a batch (JpegBatchPlan, ipx_internal.h) -----------------------------------------------------------------------------

bool jpeg_same_tables(const JpegDecTables &x, const JpegDecTables &y)
{
    return !memcmp(x.lut, y.lut, sizeof x.lut) && !memcmp(x.maxcode, y.maxcode, sizeof x.maxcode) &&
           !memcmp(x.valoff, y.valoff, sizeof x.valoff) && !memcmp(x.vals, y.vals, sizeof x.vals);
}

namespace {

inline int mcus_of(const JpegDecInfo &I) { return ((I.w + 8 * I.h0 - 1) / (8 * I.h0)) * ((I.h + 8 * I.v0 - 1) / (8 * I.v0)); }

// The RSTn markers of a baseline scan, as offsets into it.  Inside entropy-coded data 0xff is followed by 0x00 or by a marker, so every
// 0xff 0xd0..0xd7 pair is an RSTn.  IPX_ERR_UNSUPPORTED for markers out of sequence or not one per restart interval.
int find_restarts(const uint8_t *sd, const JpegDecInfo &I, std::vector<uint32_t> *marks)
{
    const int nmcu = mcus_of(I);
    if (I.ri <= 0 || nmcu <= I.ri) return IPX_OK;
    int expected = 0;
    for (size_t k = 0; k + 1 < I.scan_len;) {
        const uint8_t *q = (const uint8_t *)memchr(sd + k, 0xff, I.scan_len - 1 - k);
        if (!q) break;
        k = (size_t)(q - sd);
        const uint8_t m2 = sd[k + 1];
        if (m2 == 0x00) { k += 2; continue; }
        if (m2 < 0xd0 || m2 > 0xd7) break;                        // EOI or another marker: the scan ends here
        if (m2 != 0xd0 + expected) return IPX_ERR_UNSUPPORTED;
        marks->push_back((uint32_t)k);
        expected = (expected + 1) & 7;
        k += 2;
    }
    return (int)marks->size() != (nmcu + I.ri - 1) / I.ri - 1 ? IPX_ERR_UNSUPPORTED : IPX_OK;   // Go would try to resynchronise
}

// table classes: tab_of[i] = the first image of the batch whose Huffman tables equal image i's (most batches have one class, the
// Annex K tables every encoder defaults to); the piece kernels share one set per workgroup, so pieces are grouped by class
std::vector<int> table_classes(const JpegBatchPlan &P, const int *status)
{
    const int n = (int)P.info.size();
    std::vector<int> tab_of(n, -1), reps;
    for (int i = 0; i < n; i++) {
        if (status[i] != IPX_OK || P.info[i].host_scans) continue;
        for (size_t k = reps.size(); k-- > 0 && tab_of[i] < 0;)     // newest first: neighbours tend to match
            if (jpeg_same_tables(P.tabs[i], P.tabs[reps[k]])) tab_of[i] = reps[k];
        if (tab_of[i] < 0) { tab_of[i] = i; reps.push_back(i); }
        if (reps.size() > 64) break;                                   // a batch of hand-optimised tables: not worth the quadratic search
    }
    for (int i = 0; i < n; i++) if (status[i] == IPX_OK && tab_of[i] < 0) tab_of[i] = i;
    return tab_of;
}

// group the pieces by table class (stable: image order inside a class), each group padded to whole workgroups of 64
void group_by_class(std::vector<JpegDecImage> &items)
{
    bool one_class = true;
    for (auto &it : items) one_class = one_class && it.tab_img == items[0].tab_img;
    if (one_class) return;
    std::stable_sort(items.begin(), items.end(), [](const JpegDecImage &x, const JpegDecImage &y) { return x.tab_img < y.tab_img; });
    std::vector<JpegDecImage> grouped;
    JpegDecImage pad;
    memset(&pad, 0, sizeof pad);
    for (size_t k = 0; k < items.size(); k++) {
        if (k && items[k].tab_img != items[k - 1].tab_img)
            while (grouped.size() & 63) { pad.tab_img = items[k - 1].tab_img; grouped.push_back(pad); }
        grouped.push_back(items[k]);
    }
    items.swap(grouped);
}

}  // namespace

int jpeg_plan_batch(const ipx_bytes *files, int n, const JpegPlanOptions &opt, int *status, JpegBatchPlan *plan)
{
    const int rc = jpeg_plan_parse(files, n, opt, status, plan);
    if (rc) return rc;
    jpeg_plan_place(files, n, opt, status, plan);
    return IPX_OK;
}

int jpeg_plan_parse(const ipx_bytes *files, int n, const JpegPlanOptions &opt, int *status, JpegBatchPlan *plan)
{
    JpegBatchPlan &P = *plan;
    P.info.resize(n); P.tabs.resize(n);
    P.prog.resize(n);
    const auto t0 = std::chrono::steady_clock::now();
    // pieces of a scan: the whole scan, or one per restart interval
    P.marks.assign(n, {});
    std::vector<std::vector<uint32_t>> &marks = P.marks;
    // host preparation runs on a few threads: parsing is trivial, but finding the RSTn markers walks every compressed byte (0.3 GB for
    // a thousand 1080p files).  Files whose scans are walked on the host (progressive, several scans) only have their frame header
    // read here; their scans wait for the batch's geometry.
    const int rc = parallel_light(n, [&](int i) {
        status[i] = !files[i].data ? IPX_ERR_INVALID : (files[i].len >= ((size_t)1 << 30) ? IPX_ERR_UNSUPPORTED : jpeg_parse(files[i].data, files[i].len, &P.info[i], &P.tabs[i], false, opt.s411));
        if (status[i] == IPX_OK && !P.info[i].host_scans) status[i] = find_restarts(files[i].data + P.info[i].scan_off, P.info[i], &marks[i]);
        // a progressive file whose marker pre-pass is wholly clean has its scans walked by jpeg_prog_kernel (opt-in); every other one
        // keeps the host route, which gives the verdict as before
        // (4:1:1 / 4:1:0: the scan walk's block maps know factors 1 and 2 only)
        if (status[i] == IPX_OK && opt.prog_gpu && P.info[i].progressive && P.info[i].h0 <= 2)
            P.info[i].gpu_scans = jpeg_prog_prepass(files[i].data, files[i].len, P.info[i], &P.prog[i], P.tabs[i].qnat) ? 1 : 0;
    }, "jpeg decode: host preparation failed");
    P.parse_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

void jpeg_plan_place(const ipx_bytes *files, int n, const JpegPlanOptions &opt, int *status, JpegBatchPlan *plan)
{
    JpegBatchPlan &P = *plan;
    P.valid.assign(n, 0); P.blob_off.assign(n, 0); P.hslot.assign(n, -1);
    P.route.assign(n, 0xff);
    const std::vector<std::vector<uint32_t>> &marks = P.marks;
    const std::vector<int> tab_of = table_classes(P, status);
    // Sub-sequences of the scans that are decoded in parallel (ipx_jpeg_dec_par.hip): 1 KiB each for a large batch.  A lane walks its
    // sub-sequence symbol by symbol, so a pass over a small batch takes as long as ONE sub-sequence takes while the chip idles (8
    // files: 44 waves, 1.3 ms per pass, three passes); shorter ones until the batch fills about eight waves per CU.
    P.par_sub = opt.max_sub;
    if (opt.forced_sub == 128 || opt.forced_sub == 256 || opt.forced_sub == 512 || opt.forced_sub == 1024) P.par_sub = opt.forced_sub;
    else {
        size_t total = 0;
        for (int i = 0; i < n; i++) if (status[i] == IPX_OK && !P.info[i].host_scans) total += P.info[i].scan_len;
        while (P.par_sub > 256 && total / (size_t)P.par_sub < (size_t)131072) P.par_sub >>= 1;     // (128 measured no better: 3.0 against 3.1 ms for 8 files, worse for 64)
    }
    const std::vector<JpegDecInfo> &info = P.info;
    for (int i = 0; i < n; i++) {
        if (status[i] == IPX_OK) {
            if (P.ref < 0 && (opt.mixed || opt.want_w <= 0 || (info[i].w == opt.want_w && info[i].h == opt.want_h))) P.ref = i;
            // (mixed: the sizes are free; the class still is the reference file's)
            if (P.ref >= 0 && ((!opt.mixed && (info[i].w != info[P.ref].w || info[i].h != info[P.ref].h)) || info[i].h0 != info[P.ref].h0 || info[i].v0 != info[P.ref].v0 ||
                               info[i].ncomp != info[P.ref].ncomp))
                status[i] = IPX_ERR_UNSUPPORTED;
            else if (P.ref < 0) status[i] = IPX_ERR_UNSUPPORTED;   // a size other than the one asked for
        }
        if (status[i] != IPX_OK) continue;
        // coefficients come from the host, straight into a pinned block in the IDCT kernel's layout (slot hslot[i]); bit 1: progressive
        P.route[i] = (uint8_t)(!info[i].host_scans ? IPX_JPEG_ROUTE_PAR : info[i].gpu_scans ? IPX_JPEG_ROUTE_GPU_SCANS : IPX_JPEG_ROUTE_HOST_SCANS);
        if (info[i].host_scans && !info[i].gpu_scans) { P.valid[i] = info[i].progressive ? 3 : 1; P.hslot[i] = P.nhost++; continue; }
        if (info[i].gpu_scans) {
            // the file's bytes go into the blob whole (16-byte aligned: the kernel stages scan data with aligned 16-byte loads); no hslot
            P.valid[i] = 3;
            P.blob_off[i] = P.blob_bytes;
            P.blob_bytes += (files[i].len + 15 + 16) & ~(size_t)15;
            P.gfiles.push_back(i);
            continue;
        }
        const JpegDecInfo &I = info[i];
        const int nmcu = mcus_of(I);
        auto push = [&](size_t a0, size_t a1, int m0, int cnt) {
            JpegDecImage it;
            memset(&it, 0, sizeof it);
            it.scan_off = P.blob_bytes + (a0 & ~(size_t)15); it.scan_len = (uint32_t)(a1 - (a0 & ~(size_t)15));
            it.img = (uint32_t)i; it.first_mcu = (uint32_t)m0; it.n_mcu = (uint32_t)cnt;
            memcpy(it.td, I.td, 3); memcpy(it.ta, I.ta, 3);
            it.valid = 1;
            it.pad = (uint8_t)(a0 & 15);           // bytes to skip: pieces start 16-byte aligned for the kernel's chunk loads
            it.uoff = P.piece_ubytes;              // its unstuffed copy (launch_jpeg_pieces): a region of its own
            it.tab_img = (uint32_t)tab_of[i];
            P.piece_ubytes += ((a1 - a0) + 15 + 16) & ~(size_t)15;
            P.items.push_back(it);
        };
        size_t start = 0;
        int mcu = 0;
        for (uint32_t k : marks[i]) { push(start, k, mcu, I.ri); P.items.back().strict_end = 1; mcu += I.ri; start = (size_t)k + 2; }
        if (marks[i].empty() && opt.use_par && I.scan_len >= (size_t)4 * opt.max_sub && I.scan_len < ((size_t)1 << 28)) {   // (the same files whatever par_sub is)
            // a long scan without restart markers: decoded in parallel inside the scan (ipx_jpeg_dec_par.hip)
            JpegParImage pi;
            memset(&pi, 0, sizeof pi);
            pi.scan_off = P.blob_bytes; pi.scan_len = (uint32_t)I.scan_len; pi.img = (uint32_t)i;
            pi.nsub = (uint32_t)((I.scan_len + P.par_sub - 1) / P.par_sub);
            memcpy(pi.td, I.td, 3); memcpy(pi.ta, I.ta, 3);
            P.par.push_back(pi);
        } else {
            push(start, I.scan_len, mcu, nmcu - mcu);
        }
        P.valid[i] = 1;
        P.blob_off[i] = P.blob_bytes;
        P.blob_bytes += (I.scan_len + 15 + 16) & ~(size_t)15;
    }
    if (P.ref >= 0) group_by_class(P.items);
}

}  // namespace ipx
