// CPU-side sanitizer run of the parsers that read bytes from outside: the JPEG marker parser (ipx_jpeg_dec_host.cpp, fed with
// every upload), the host scan decoder of progressive / multi-scan files (ipx_jpeg_dec_prog.cpp) and the TrueType loader / rasteriser (ipx_font.cpp).  Built with -fsanitize=address,undefined by tools/sanitize/run.sh;
// inputs: seed files given on the command line (*.jpg, *.ttf), mutated with a fixed-seed generator.  Any report aborts the run.
// The JPEG seeds and their mutations then go, in mixed batches of 1, 5 and 70 files, through the host plan of a batch decode
// (jpeg_plan_batch), whose invariants -- what the kernels rely on when they index the blob and the scratch -- are asserted.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../imageprocessor_amd/csrc/ipx_internal.h"

namespace ipx {
void set_error(const char *, ...) {}
int status_of_exception() noexcept { return IPX_ERR_NOMEM; }
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}

static std::vector<uint8_t> slurp(const char *path)
{
    std::vector<uint8_t> v;
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

static void mutate(std::vector<uint8_t> &v, size_t lo, size_t hi)
{
    if (hi <= lo) return;
    switch (rnd() % 5) {
    case 0: for (int k = 1 + rnd() % 4; k > 0; k--) v[lo + rnd() % (hi - lo)] ^= (uint8_t)(1u << (rnd() % 8)); break;
    case 1: for (int k = 1 + rnd() % 4; k > 0; k--) v[lo + rnd() % (hi - lo)] = (uint8_t)rnd(); break;
    case 2: v.resize(lo + rnd() % (hi - lo)); break;
    case 3: { const size_t a = lo + rnd() % (hi - lo), n = std::min<size_t>(v.size() - a, 1 + rnd() % 64); v.erase(v.begin() + a, v.begin() + a + n); break; }
    default: { const size_t a = lo + rnd() % (hi - lo); for (int k = 0; k < 2; k++) if (a + k < v.size()) v[a + k] = k ? 0xff : (uint8_t)(0xff - rnd() % 3); break; }   // large lengths
    }
}

#define PLAN_CHECK(cond) do { if (!(cond)) { fprintf(stderr, "batch plan: %s does not hold (batch of %d)\n", #cond, n); abort(); } } while (0)

static long plan_pieces = 0, plan_padding = 0, plan_par = 0;

// one batch through jpeg_plan_batch
static void check_plan(const std::vector<std::vector<uint8_t>> &batch, const ipx::JpegPlanOptions &opt)
{
    const int n = (int)batch.size();
    std::vector<uint8_t *> heap(n);          // exact-size copies: a read past a file's end is an ASan report
    std::vector<ipx_bytes> files(n);
    for (int i = 0; i < n; i++) {
        heap[i] = (uint8_t *)malloc(batch[i].size() ? batch[i].size() : 1);
        memcpy(heap[i], batch[i].data(), batch[i].size());
        files[i].data = heap[i]; files[i].len = batch[i].size();
    }
    std::vector<int> status(n, 0);
    ipx::JpegBatchPlan P;
    PLAN_CHECK(ipx::jpeg_plan_batch(files.data(), n, opt, status.data(), &P) == IPX_OK);
    const size_t end = P.blob_bytes + 16;
    std::vector<std::pair<size_t, size_t>> regions;                 // the pieces' unstuffed copies
    std::vector<std::vector<std::pair<uint32_t, uint32_t>>> mcus(n); // per image: (first_mcu, n_mcu) of its pieces
    for (size_t k = 0; k < P.items.size(); k++) {
        const ipx::JpegDecImage &it = P.items[k];
        const bool last_class = it.tab_img == P.items.back().tab_img;
        if (k && it.tab_img != P.items[k - 1].tab_img) PLAN_CHECK(k % 64 == 0);          // every class run but the last: whole groups of 64
        if (!it.valid) { PLAN_CHECK(!last_class); plan_padding++; continue; }            // padding
        PLAN_CHECK((int)it.img < n && status[it.img] == IPX_OK && P.valid[it.img] == 1 && !P.info[it.img].host_scans);
        PLAN_CHECK(it.scan_off % 16 == 0 && it.pad < 16 && it.pad <= it.scan_len && it.scan_off + it.scan_len <= end);
        PLAN_CHECK(it.scan_off >= P.blob_off[it.img] && it.scan_off + it.scan_len <= P.blob_off[it.img] + P.info[it.img].scan_len);
        PLAN_CHECK(it.uoff % 16 == 0 && it.uoff + (it.scan_len - it.pad) + 16 <= P.piece_ubytes);
        regions.push_back({(size_t)it.uoff, (size_t)it.uoff + (it.scan_len - it.pad) + 16});
        mcus[it.img].push_back({it.first_mcu, it.n_mcu});
        PLAN_CHECK((int)it.tab_img < n && status[it.tab_img] == IPX_OK && ipx::jpeg_same_tables(P.tabs[it.img], P.tabs[it.tab_img]));
    }
    std::sort(regions.begin(), regions.end());
    for (size_t k = 1; k < regions.size(); k++) PLAN_CHECK(regions[k - 1].second <= regions[k].first);
    for (const ipx::JpegParImage &pi : P.par) {
        PLAN_CHECK((int)pi.img < n && status[pi.img] == IPX_OK && P.valid[pi.img] == 1 && mcus[pi.img].empty());
        PLAN_CHECK(pi.scan_off == P.blob_off[pi.img] && pi.scan_len == P.info[pi.img].scan_len && pi.scan_off + pi.scan_len <= end);
        PLAN_CHECK(P.par_sub >= 128 && pi.nsub == (pi.scan_len + P.par_sub - 1) / P.par_sub);
        mcus[pi.img].push_back({0u, ~0u});
    }
    int nhost = 0;
    for (int i = 0; i < n; i++) {
        const ipx::JpegDecInfo &I = P.info[i];
        if (status[i] != IPX_OK) { PLAN_CHECK(!P.valid[i] && mcus[i].empty() && P.hslot[i] < 0); continue; }
        PLAN_CHECK(P.ref >= 0 && I.w == P.info[P.ref].w && I.h == P.info[P.ref].h && I.h0 == P.info[P.ref].h0 && I.v0 == P.info[P.ref].v0 && I.ncomp == P.info[P.ref].ncomp);
        if (I.gpu_scans) {
            // a progressive file the GPU walks (opt.prog_gpu): its whole bytes in the blob, 16-byte aligned; every scan's readable data
            // inside the file; every table a scan decodes with among the file's definitions
            PLAN_CHECK(opt.prog_gpu && I.host_scans && I.progressive && P.hslot[i] < 0 && mcus[i].empty() && P.valid[i] == 3);
            PLAN_CHECK(std::count(P.gfiles.begin(), P.gfiles.end(), i) == 1 && P.route[i] == IPX_JPEG_ROUTE_GPU_SCANS);
            PLAN_CHECK(P.blob_off[i] % 16 == 0 && P.blob_off[i] + ((files[i].len + 15) & ~(size_t)15) <= end);
            const ipx::JpegProgPlan &G = P.prog[i];
            PLAN_CHECK(!G.scans.empty() && G.scans.size() <= (size_t)ipx::IPX_JPEG_PROG_MAX_SCANS && G.defs.size() <= 3 * G.scans.size());
            for (const ipx::JpegProgScan &s : G.scans) {
                PLAN_CHECK((size_t)s.off + s.len <= files[i].len && s.ns >= 1 && s.ns <= I.ncomp && s.ss <= s.se && s.se < 64 && (s.ss == 0 || s.ns == 1));
                for (int c = 0; c < s.ns; c++) {
                    PLAN_CHECK(s.comp[c] < I.ncomp);
                    if (s.ss == 0 && s.ah == 0) PLAN_CHECK(s.dc_def[c] < G.defs.size());
                    if (s.ss > 0) PLAN_CHECK(s.ac_def[c] < G.defs.size());
                }
            }
            continue;
        }
        if (I.host_scans) { PLAN_CHECK(P.hslot[i] == nhost++ && mcus[i].empty() && (P.valid[i] & 1)); continue; }
        PLAN_CHECK(P.hslot[i] < 0 && !mcus[i].empty());
        if (mcus[i][0].second == ~0u) continue;                                          // a parallel image: the whole scan
        const uint32_t nmcu = (uint32_t)(((I.w + 8 * I.h0 - 1) / (8 * I.h0)) * ((I.h + 8 * I.v0 - 1) / (8 * I.v0)));
        std::sort(mcus[i].begin(), mcus[i].end());
        uint32_t at = 0;
        for (auto &m : mcus[i]) { PLAN_CHECK(m.first == at && m.second > 0); at += m.second; }   // the pieces tile [0, nmcu) exactly
        PLAN_CHECK(at == nmcu);
    }
    PLAN_CHECK(nhost == P.nhost);
    for (uint8_t *h : heap) free(h);
    plan_pieces += (long)P.items.size();
    plan_par += (long)P.par.size();
}

int main(int argc, char **argv)
{
    const int cases = argc > 1 ? atoi(argv[1]) : 2000;
    std::vector<std::vector<uint8_t>> jpeg_seeds;
    long jpeg_ok = 0, jpeg_bad = 0, font_ok = 0, font_bad = 0, host_ok = 0, host_bad = 0;
    for (int a = 2; a < argc; a++) {
        const std::string path = argv[a];
        const std::vector<uint8_t> seed = slurp(argv[a]);
        const bool is_font = path.size() > 4 && path.substr(path.size() - 4) == ".ttf";
        if (!is_font) jpeg_seeds.push_back(seed);
        for (int t = 0; t < cases; t++) {
            std::vector<uint8_t> v = seed;
            if (is_font) {
                // table directory and the tables the loader reads are spread over the file: mutate anywhere, mostly near the front
                if (t) mutate(v, 0, (rnd() & 1) ? std::min<size_t>(v.size(), 4096) : v.size());
                // exact-size heap copy so that any read past the end is an ASan report
                uint8_t *heap = (uint8_t *)malloc(v.size() ? v.size() : 1);
                memcpy(heap, v.data(), v.size());
                ipx_font *font = nullptr;
                if (ipx_font_create(heap, v.size(), &font) == IPX_OK && font) {
                    font_ok++;
                    int32_t w26 = 0; int wpx = 0;
                    (void)ipx_font_text_width(font, "Sample Watermark \xc3\xa9\xe2\x82\xac", 24.0 + (t % 40), &w26, &wpx);
                    const ipx_glyph *gl = nullptr; int n = 0;
                    if (ipx_font_draw_string(font, "Wj\xc3\xa9.", 12.0 + (t % 90), 10, 60, 640, 360, &gl, &n, nullptr) == IPX_OK) ipx_font_release_thread();
                    (void)ipx_font_kern(font, 'A', 'V', 32.0, &w26);
                    ipx_font_destroy(font);
                } else font_bad++;
                free(heap);
            } else {
                size_t sos = 0;
                for (size_t i = 0; i + 1 < v.size(); i++) if (v[i] == 0xff && v[i + 1] == 0xda) { sos = i; break; }
                // header region for the marker parser; every other case anywhere in the file, so that the host scan decoder
                // (progressive / multi-scan files) sees broken entropy-coded data, lost scans and misplaced markers as well
                if (t) mutate(v, 2, (t & 1) ? v.size() : std::min(v.size(), sos + 16));
                uint8_t *heap = (uint8_t *)malloc(v.size() ? v.size() : 1);
                memcpy(heap, v.data(), v.size());
                ipx::JpegDecInfo info;
                static ipx::JpegDecTables tab;
                const int rc = ipx::jpeg_parse(heap, v.size(), &info, &tab);
                if (rc == IPX_OK) {
                    jpeg_ok++;
                    if (info.w <= 0 || info.h <= 0 || (!info.host_scans && info.scan_off + info.scan_len > v.size())) { fprintf(stderr, "inconsistent parse result\n"); abort(); }
                    if (info.host_scans) {
                        // exact-size slices, as the runtime hands them out (one past the end is an ASan report)
                        const size_t mxx = (info.w + 8 * info.h0 - 1) / (8 * info.h0), myy = (info.h + 8 * info.v0 - 1) / (8 * info.v0);
                        const size_t nblk = mxx * myy * (info.ncomp == 1 ? 1 : info.h0 * info.v0 + 2);
                        if (nblk > (size_t)1 << 22) { host_bad++; free(heap); continue; }      // (a mutated size: the runtime's batch geometry check comes first)
                        int16_t *coefs = (int16_t *)malloc(nblk * 64 * sizeof(int16_t)), *dcs = (int16_t *)malloc(nblk * sizeof(int16_t));
                        uint16_t qnat[3][64];
                        bool prog = false;
                        ipx::JpegDecInfo hi = info;
                        const int hr = ipx::jpeg_host_decode(heap, v.size(), &hi, coefs, dcs, nblk, qnat, &prog);
                        if (hr == IPX_OK) {
                            host_ok++;
                            if (hi.w != info.w || hi.h != info.h) { fprintf(stderr, "host decoder disagrees with the parser\n"); abort(); }
                        } else host_bad++;
                        free(coefs); free(dcs);
                    }
                } else jpeg_bad++;
                free(heap);
            }
        }
    }
    long plans = 0;
    for (int t = 0; !jpeg_seeds.empty() && t < std::max(30, cases / 10); t++) {
        const int n = t % 3 == 0 ? 1 : (t % 3 == 1 ? 5 : 70);
        std::vector<std::vector<uint8_t>> batch(n);
        for (auto &v : batch) {
            v = jpeg_seeds[rnd() % jpeg_seeds.size()];
            if (rnd() % 3 == 0) mutate(v, 2, v.size());
        }
        static const int subs[] = {0, 0, 128, 256, 512, 1024};
        const ipx::JpegPlanOptions opt{t % 5 == 4 ? 160 : 0, t % 5 == 4 ? 120 : 0, t % 7 != 6, subs[t % 6], 1024, t % 3 != 2};
        check_plan(batch, opt);
        plans++;
    }
    printf("jpeg headers: %ld parsed, %ld refused; host scan decodes: %ld done, %ld refused; batch plans: %ld checked, %ld pieces (%ld of them padding), %ld parallel images; fonts: %ld loaded, %ld refused; no sanitizer report\n",
           jpeg_ok, jpeg_bad, host_ok, host_bad, plans, plan_pieces, plan_padding, plan_par, font_ok, font_bad);
    return 0;
}
