// texts_batcher_host_test.cpp -- the micro-batcher's per-file text switch (csrc/ipx_batcher.cpp, IPX_BATCH_TEXTS=1 at the ABI) on the
// CPU alone: plain g++, no GPU, no HIP.  The "device" is a fake backend that copies what every job says about its texts at submit.
//
// What it shows:
//   switch on   files that differ only in their text (glyph count, rectangles, mask bytes, colour) share ONE job; the job has
//               ops.glyphs == NULL and texts set, and texts[i] holds file i's glyph bytes and colour, deep-copied (the submitter's
//               buffers are overwritten right after each submit) with tight rows; a file of another frame size goes out alone
//   switch off  the same files form one job each, with texts == NULL and the text in ops.glyphs, as always
//   257 glyphs  refused at submit with IPX_ERR_UNSUPPORTED, alone: the files around it still share their job
// tests/test_texts_host.py builds and runs it.
#define IPX_BATCHER_NO_ABI 1
#include "../imageprocessor_amd/csrc/ipx_batcher.cpp"

#include <cstdio>
#include <cstdlib>

namespace {

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

struct SeenGlyph { int mw, mh, mstride; ipx_rect dr; int mpx, mpy; std::vector<uint8_t> mask; };
struct SeenText { std::vector<SeenGlyph> glyphs; uint8_t col[4]; };
struct SeenJob {
    int kind, n, sw;
    bool has_texts, ops_glyphs;
    int ops_n_glyphs;
    std::vector<SeenText> texts;
    std::vector<uint8_t> first_bytes;      // byte 2 of every file: which test file it is
};
struct FakePool { std::vector<SeenJob> jobs; };

SeenGlyph see(const ipx_glyph &g)
{
    SeenGlyph s{g.mw, g.mh, g.mstride, g.dr, g.mpx, g.mpy, {}};
    for (int y = 0; y < g.mh; y++) s.mask.insert(s.mask.end(), g.mask + (size_t)y * g.mstride, g.mask + (size_t)y * g.mstride + g.mw);
    return s;
}

int fake_submit(void *self, const ipx_job *j, ipx_ticket *t)
{
    FakePool *p = (FakePool *)self;
    SeenJob s{j->kind, j->n, j->ops.sw, j->texts != nullptr, j->ops.glyphs != nullptr, j->ops.n_glyphs, {}, {}};
    for (int i = 0; i < j->n; i++) {
        s.first_bytes.push_back(j->files[i].data[2]);
        SeenText st{};
        if (j->texts) {
            for (int g = 0; g < j->texts[i].n_glyphs; g++) st.glyphs.push_back(see(j->texts[i].glyphs[g]));
            memcpy(st.col, j->texts[i].col, 4);
        } else {
            for (int g = 0; g < j->ops.n_glyphs; g++) st.glyphs.push_back(see(j->ops.glyphs[g]));
            memcpy(st.col, j->ops.col, 4);
        }
        s.texts.push_back(st);
    }
    p->jobs.push_back(s);
    *t = p->jobs.size();
    return IPX_OK;
}
int fake_wait(void *, ipx_ticket) { return IPX_OK; }
int fake_release(void *, ipx_ticket) { return IPX_OK; }

// test file k's text: k % 4 glyphs (text 0, 4: none), masks of (3 + k) x (2 + g) with rows `pad` bytes apart in the submitter's buffer
struct Submitter {
    std::vector<std::vector<uint8_t>> bufs;
    std::vector<ipx_glyph> glyphs;
    ipx_pool_ops ops;
    std::vector<uint8_t> file;
};
uint8_t mask_byte(int k, int g, int y, int x) { return (uint8_t)(k * 37 + g * 11 + y * 5 + x * 3 + 1); }

void make(Submitter &s, int k, int n_glyphs, int sw)
{
    const int pad = 5;
    s.bufs.clear(); s.glyphs.clear();
    for (int g = 0; g < n_glyphs; g++) {
        const int mw = 3 + k % 5, mh = 2 + g % 3;
        std::vector<uint8_t> b((size_t)(mw + pad) * mh, 0xEE);
        for (int y = 0; y < mh; y++)
            for (int x = 0; x < mw; x++) b[(size_t)y * (mw + pad) + x] = mask_byte(k, g, y, x);
        s.bufs.push_back(b);
    }
    for (int g = 0; g < n_glyphs; g++) {
        const int mw = 3 + k % 5, mh = 2 + g % 3;
        ipx_glyph gl;
        gl.mask = s.bufs[g].data(); gl.mw = mw; gl.mh = mh; gl.mstride = mw + pad;
        gl.dr = ipx_rect{10 * g + k, k, 10 * g + k + mw - 1, k + mh};
        gl.mpx = 1; gl.mpy = 0;
        s.glyphs.push_back(gl);
    }
    memset(&s.ops, 0, sizeof s.ops);
    s.ops.sw = sw; s.ops.sh = 50; s.ops.do_resize = 1; s.ops.resize_w = 10; s.ops.resize_h = 10; s.ops.do_watermark = 1;
    s.ops.glyphs = s.glyphs.empty() ? nullptr : s.glyphs.data();
    s.ops.n_glyphs = n_glyphs;
    s.ops.col[0] = (uint8_t)(200 + k); s.ops.col[1] = (uint8_t)k; s.ops.col[2] = 7; s.ops.col[3] = (uint8_t)(100 + k);
    s.file = {0xff, 0xd8, (uint8_t)k, 1, 2, 3};
}

// the submitter frees or reuses its memory right after submit
void scribble(Submitter &s)
{
    for (auto &b : s.bufs) std::fill(b.begin(), b.end(), 0x5A);
    for (auto &g : s.glyphs) { g.mw = 99; g.mh = 99; g.dr = ipx_rect{-1, -1, -1, -1}; g.mask = nullptr; }
    memset(s.ops.col, 0x33, 4);
}

void check_text(const SeenText &t, int k, int n_glyphs)
{
    REQUIRE((int)t.glyphs.size() == n_glyphs);
    REQUIRE(t.col[0] == (uint8_t)(200 + k) && t.col[1] == (uint8_t)k && t.col[2] == 7 && t.col[3] == (uint8_t)(100 + k));
    for (int g = 0; g < n_glyphs; g++) {
        const SeenGlyph &s = t.glyphs[g];
        const int mw = 3 + k % 5, mh = 2 + g % 3;
        REQUIRE(s.mw == mw && s.mh == mh && s.mstride == mw);         // the copy's rows are tight
        REQUIRE(s.dr.x0 == 10 * g + k && s.dr.y0 == k && s.dr.x1 == 10 * g + k + mw - 1 && s.dr.y1 == k + mh && s.mpx == 1 && s.mpy == 0);
        for (int y = 0; y < mh; y++)
            for (int x = 0; x < mw; x++) REQUIRE(s.mask[(size_t)y * mw + x] == mask_byte(k, g, y, x));
    }
}

// 8 files of one size with texts of their own, a 257-glyph text after the third, a file of another size after the fifth
void run(bool texts_on, FakePool &pool, std::vector<Submitter> &keep)
{
    using namespace ipx;
    BatchBackend be;
    be.self = &pool; be.submit = fake_submit; be.wait = fake_wait; be.release = fake_release;
    be.last_error = [] { return ""; };
    keep.resize(10);                                             // the FILE bytes stay valid until release, as the ABI asks
    Batcher b(be, 8, 10000000, 77, 0, texts_on);
    for (int k = 0; k < 8; k++) {
        Submitter &s = keep[k];
        make(s, k, k % 4, 100);
        uint64_t t = 0;
        std::string err;
        REQUIRE(b.submit(ipx_bytes{s.file.data(), s.file.size()}, s.ops, &t, &err) == IPX_OK);
        scribble(s);
        if (k == 2 && texts_on) {                                // too long a text: refused here, alone
            Submitter &big = keep[8];
            make(big, 0, 1, 100);
            std::vector<ipx_glyph> many(257, big.glyphs[0]);
            big.ops.glyphs = many.data(); big.ops.n_glyphs = 257;
            REQUIRE(b.submit(ipx_bytes{big.file.data(), big.file.size()}, big.ops, &t, &err) == IPX_ERR_UNSUPPORTED);
            REQUIRE(err.find("256") != std::string::npos);
        }
        if (k == 4) {
            Submitter &other = keep[9];
            make(other, 9, 2, 101);
            REQUIRE(b.submit(ipx_bytes{other.file.data(), other.file.size()}, other.ops, &t, &err) == IPX_OK);
            scribble(other);
        }
    }
    ipx_batcher_stats st;
    b.stats(&st);
    REQUIRE(st.files == 9);
}   // ~Batcher flushes what is pending

}  // namespace

int main()
{
    {
        FakePool pool;
        std::vector<Submitter> keep;
        run(true, pool, keep);
        // one job of the eight files (by size, when the eighth arrived), then the file of the other size (at destruction)
        REQUIRE(pool.jobs.size() == 2);
        const SeenJob &j = pool.jobs[0];
        REQUIRE(j.n == 8 && j.kind == IPX_JOB_JPEG && j.sw == 100 && j.has_texts && !j.ops_glyphs && j.ops_n_glyphs == 0);
        for (int i = 0; i < 8; i++) {
            REQUIRE(j.first_bytes[i] == i);
            check_text(j.texts[i], i, i % 4);
        }
        const SeenJob &o = pool.jobs[1];
        REQUIRE(o.n == 1 && o.sw == 101 && o.has_texts && !o.ops_glyphs && o.first_bytes[0] == 9);
        check_text(o.texts[0], 9, 2);
        printf("switch on: %d files with %d different texts in one job, texts deep-copied; another size alone; 257 glyphs refused alone\n", j.n, j.n);
    }
    {
        FakePool pool;
        std::vector<Submitter> keep;
        run(false, pool, keep);
        // texts 0 and 4 are both empty but differ in colour: nine different operator contents, nine jobs
        REQUIRE(pool.jobs.size() == 9);
        bool seen[10] = {false};
        for (const SeenJob &j : pool.jobs) {
            REQUIRE(j.n == 1 && !j.has_texts);
            const int k = j.first_bytes[0];
            REQUIRE(k >= 0 && k < 10 && !seen[k]);
            seen[k] = true;
            const int ng = k == 9 ? 2 : k % 4;
            REQUIRE(j.ops_n_glyphs == ng && j.ops_glyphs == (ng != 0));
            check_text(j.texts[0], k, ng);
        }
        printf("switch off: %zu jobs of one file each, texts == NULL\n", pool.jobs.size());
    }
    printf("texts batcher ok\n");
    return 0;
}
