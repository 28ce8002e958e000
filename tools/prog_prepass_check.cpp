// prog_prepass_check.cpp -- a stand-alone driver of the marker pre-pass of the GPU scan walk (jpeg_prog_prepass), for a sanitizer
// build on the CPU: tools/prog_prepass_asan.py writes clean and damaged progressive files, builds this program together with
// ipx_jpeg_dec_host.cpp and ipx_jpeg_dec_prog.cpp under -fsanitize=address,undefined and runs it on them.  For every file: the header
// parser, the pre-pass and the host scan decoder run; a clean pre-pass must describe scans that lie inside the file, end where the
// reader ends (at an 0xff that 0x00 does not follow, or at the file's end), hold no such byte before, and name table definitions
// that exist.  No device is touched.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../imageprocessor_amd/csrc/ipx_internal.h"

namespace ipx {   // the error plumbing of ipx_host.cpp, which this program does not link
void set_error(const char *, ...) {}
int status_of_exception() noexcept { return IPX_ERR_INVALID; }
}

static std::vector<uint8_t> slurp(const char *path)
{
    std::vector<uint8_t> v;
    FILE *f = fopen(path, "rb");
    if (!f) return v;
    uint8_t buf[65536];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

int main(int argc, char **argv)
{
    int clean = 0, kept = 0, refused = 0, bad = 0;
    for (int a = 1; a < argc; a++) {
        const std::vector<uint8_t> file = slurp(argv[a]);
        // an exact-size heap copy: a read one byte past the file is a sanitizer report
        uint8_t *d = (uint8_t *)malloc(file.size() ? file.size() : 1);
        for (size_t k = 0; k < file.size(); k++) d[k] = file[k];
        const size_t len = file.size();
        ipx::JpegDecInfo info;
        ipx::JpegDecTables tab;
        const int st = ipx::jpeg_parse(d, len, &info, &tab);
        if (st != IPX_OK) { refused++; free(d); continue; }
        ipx::JpegProgPlan plan;
        const bool ok = info.host_scans && ipx::jpeg_prog_prepass(d, len, info, &plan, tab.qnat);
        if (ok) {
            clean++;
            if (plan.defs.size() > 3 * plan.scans.size()) { bad++; fprintf(stderr, "%s: %zu table definitions for %zu scans\n", argv[a], plan.defs.size(), plan.scans.size()); }
            if (plan.scans.empty() || plan.scans.size() > (size_t)ipx::IPX_JPEG_PROG_MAX_SCANS) { bad++; fprintf(stderr, "%s: %zu scans\n", argv[a], plan.scans.size()); }
            for (const ipx::JpegProgScan &s : plan.scans) {
                const size_t end = (size_t)s.off + s.len;
                bool fine = end <= len && s.ns >= 1 && s.ns <= 3 && s.ss <= s.se && s.se < 64;
                for (size_t k = s.off; fine && k < end; k++)
                    if (d[k] == 0xff) { fine = k + 1 < end && d[k + 1] == 0; k++; }
                if (fine && end < len) fine = d[end] == 0xff && (end + 1 >= len || d[end + 1] != 0);
                for (int i = 0; fine && i < s.ns; i++) {
                    if (s.ss == 0 && s.ah == 0) fine = s.dc_def[i] < plan.defs.size();
                    if (s.ss > 0) fine = s.ac_def[i] < plan.defs.size();
                    fine = fine && s.comp[i] < info.ncomp;
                }
                if (!fine) { bad++; fprintf(stderr, "%s: a scan the pre-pass describes wrongly (off %u len %u)\n", argv[a], s.off, s.len); }
            }
        } else kept++;
        if (info.host_scans) {      // the host route over the same bytes (it shares the marker loop and the SOS checks)
            const size_t mxx = (info.w + 8 * info.h0 - 1) / (8 * info.h0), myy = (info.h + 8 * info.v0 - 1) / (8 * info.v0);
            const size_t nblk = mxx * myy * (info.ncomp == 1 ? 1 : info.h0 * info.v0 + 2);
            std::vector<int16_t> coefs(nblk * 64), dcs(nblk);
            ipx::JpegDecInfo full;
            uint16_t q[3][64];
            bool prog = false;
            (void)ipx::jpeg_host_decode(d, len, &full, coefs.data(), dcs.data(), nblk, q, &prog);
        }
        free(d);
    }
    printf("prog_prepass_check: %d files: %d refused by the header parser, %d clean for the GPU walk, %d kept on the host route, %d wrong\n",
           argc - 1, refused, clean, kept, bad);
    return bad ? 1 : 0;
}
