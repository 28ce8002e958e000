// jpeg411_host_test.cpp -- a stand-alone driver of the host half of the 4:1:1 / 4:1:0 JPEG decoder (IPX_JPEG_411=1): jpeg_parse with the
// switch, and jpeg_host_decode on every file whatever its route (the scan decoder takes baseline files too), for a sanitizer build on
// the CPU.  tests/test_jpeg_411_host.py writes the files (tests/jpeg_411_corpus.py), builds this program with ipx_jpeg_dec_host.cpp and
// ipx_jpeg_dec_prog.cpp under -fsanitize=address,undefined and runs it on them.  For every file given:
//   - the file goes through the parser and the scan decoder, from an exact-size heap copy and into exact-size outputs (a read or write
//     one element past either is a sanitizer report); next to FILE a FILE.want may lie: the status expected, and for status 0 the luma
//     factors, the host_scans and progressive flags, the mask of components coded by non-interleaved scans only, and the coefficients as
//     the IDCT kernel reads them (int16: nblk * 64 in natural order with element 0 zero, then nblk DC terms) -- compared word for word
//   - seeded mutations of it -- truncations, flipped bits in the header bytes, changed bytes anywhere -- go the same way; their verdicts
//     are not judged, only that nothing is read or written out of bounds
//   - without the switch the parser must refuse every frame whose luma h factor is 4, as it always did
// No device is touched.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../imageprocessor_amd/csrc/ipx_internal.h"

namespace ipx {   // the error plumbing of ipx_host.cpp, which this program does not link
void set_error(const char *, ...) {}
int status_of_exception() noexcept { return IPX_ERR_INVALID; }
}

static std::vector<uint8_t> slurp(const std::string &path, bool *found = nullptr)
{
    std::vector<uint8_t> v;
    FILE *f = fopen(path.c_str(), "rb");
    if (found) *found = f != nullptr;
    if (!f) return v;
    uint8_t buf[65536];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

struct Outcome { int status = 0, h0 = 0, v0 = 0, host_scans = 0, progressive = 0, alone = 0; std::vector<int16_t> words; };

// parser and scan decoder over an exact-size copy of `file`
static Outcome decode(const std::vector<uint8_t> &file, bool s411)
{
    Outcome o;
    const size_t len = file.size();
    uint8_t *d = (uint8_t *)malloc(len ? len : 1);
    if (len) memcpy(d, file.data(), len);
    ipx::JpegDecInfo info;
    ipx::JpegDecTables tab;
    o.status = ipx::jpeg_parse(d, len, &info, &tab, false, s411);
    if (o.status == IPX_OK) {
        o.h0 = info.h0; o.v0 = info.v0; o.host_scans = info.host_scans;
        const size_t mxx = (info.w + 8 * info.h0 - 1) / (8 * info.h0), myy = (info.h + 8 * info.v0 - 1) / (8 * info.v0);
        const size_t nblk = mxx * myy * (info.ncomp == 1 ? 1 : info.h0 * info.v0 + 2);
        if (nblk > ((size_t)1 << 16)) o.status = IPX_ERR_UNSUPPORTED;   // (a mutated frame size: not this program's business)
        else {
            int16_t *out = (int16_t *)malloc(nblk * 65 * sizeof(int16_t));
            ipx::JpegDecInfo full;
            uint16_t q[3][64];
            bool prog = false;
            o.status = ipx::jpeg_host_decode(d, len, &full, out, out + nblk * 64, nblk, q, &prog, s411, &o.alone);
            o.progressive = prog;
            if (o.status == IPX_OK) o.words.assign(out, out + nblk * 65);
            free(out);
        }
    }
    free(d);
    return o;
}

int main(int argc, char **argv)
{
    int checked = 0, bad = 0;
    long mutated = 0;
    uint32_t seed = 0x9e3779b9u;
    auto rnd = [&](uint32_t n) { seed = seed * 1664525u + 1013904223u; return n ? (seed >> 8) % n : 0u; };
    for (int a = 1; a < argc; a++) {
        const std::vector<uint8_t> file = slurp(argv[a]);
        const Outcome got = decode(file, true);
        bool have = false;
        const std::vector<uint8_t> want = slurp(std::string(argv[a]) + ".want", &have);
        if (have) {
            // int32 status, h0, v0, host_scans, progressive, alone, then the words
            checked++;
            int32_t head[6] = {0, 0, 0, 0, 0, 0};
            if (want.size() < sizeof head) { bad++; fprintf(stderr, "%s: short .want\n", argv[a]); continue; }
            memcpy(head, want.data(), sizeof head);
            bool same = got.status == head[0];
            if (same && got.status == IPX_OK)
                same = got.h0 == head[1] && got.v0 == head[2] && got.host_scans == head[3] && got.progressive == head[4] && got.alone == head[5] &&
                       want.size() - sizeof head == got.words.size() * 2 && !memcmp(want.data() + sizeof head, got.words.data(), got.words.size() * 2);
            if (!same) {
                bad++;
                fprintf(stderr, "%s: status %d factors %dx%d host_scans %d progressive %d alone %d, %zu words; expected %d %dx%d %d %d %d, %zu words\n", argv[a],
                        got.status, got.h0, got.v0, got.host_scans, got.progressive, got.alone, got.words.size(), head[0], head[1], head[2], head[3], head[4],
                        head[5], (want.size() - sizeof head) / 2);
            }
        }
        // without the switch: a frame with h = 4 is refused by the parser, whatever else the file holds
        if (got.status == IPX_OK && got.h0 == 4 && decode(file, false).status != IPX_ERR_UNSUPPORTED) { bad++; fprintf(stderr, "%s: decoded without the switch\n", argv[a]); }
        for (int m = 0; m < 60 && !file.empty(); m++) {
            std::vector<uint8_t> f = file;
            switch (m % 3) {
            case 0: f.resize(rnd((uint32_t)f.size())); break;                                            // a truncation
            case 1: f[rnd((uint32_t)std::min<size_t>(f.size(), 700))] ^= (uint8_t)(1u << rnd(8)); break;  // a flipped bit in the headers
            default: f[rnd((uint32_t)f.size())] = (uint8_t)rnd(256); break;                               // a changed byte anywhere
            }
            (void)decode(f, true);
            mutated++;
        }
    }
    printf("jpeg411_host_test: %d files, %d with expectations, %ld mutations, %d wrong\n", argc - 1, checked, mutated, bad);
    return bad ? 1 : 0;
}
