// jpeg4_batcher_key_test.cpp -- the micro-batcher's grouping key (csrc/ipx_batcher.cpp: jpeg_shape) for four-component JPEGs, on the
// CPU alone against a fake backend (as batcher_formats_host_test.cpp): single files whose frame headers announce one, three or four
// components with luma sampling 1 x 1 or 2 x 2 are submitted from four threads, interleaved, with idle flushing off; every job the
// backend receives must hold files of ONE component count and ONE luma sampling -- a four-component file never shares a group with a
// three-component one (under IPX_JPEG_CMYK=1 the leg would take it out again; without the switch it would be handed back and, arriving
// first, would have its neighbours handed back).  Built by tests/test_jpeg_cmyk_batcher.py with -fsanitize=address,undefined.
#define IPX_BATCHER_NO_ABI 1
#include "../../imageprocessor_amd/csrc/ipx_batcher.cpp"

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <deque>

namespace {

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "line %d: %s\n", __LINE__, #c); abort(); } } while (0)

struct Shape { uint8_t ncomp, hv; };
const Shape kShapes[5] = {{1, 0x11}, {3, 0x11}, {3, 0x22}, {4, 0x11}, {4, 0x22}};

// SOI, an APP14 segment, SOF0 of 16 x 16 with the shape's components, then a serial number
std::vector<uint8_t> make_file(const Shape &s, int serial)
{
    std::vector<uint8_t> f = {0xff, 0xd8, 0xff, 0xee, 0x00, 0x0e, 'A', 'd', 'o', 'b', 'e', 0, 100, 0, 0, 0, 0, 2};
    const int len = 8 + 3 * s.ncomp;
    const uint8_t head[] = {0xff, 0xc0, (uint8_t)(len >> 8), (uint8_t)len, 8, 0, 16, 0, 16, s.ncomp};
    f.insert(f.end(), head, head + sizeof head);
    for (int c = 0; c < s.ncomp; c++) { f.push_back((uint8_t)(c + 1)); f.push_back(c == 0 || c == 3 ? s.hv : 0x11); f.push_back(0); }
    f.push_back((uint8_t)serial); f.push_back((uint8_t)(serial >> 8));
    return f;
}
Shape shape_of(const ipx_bytes &f)
{
    REQUIRE(f.len > 30 && f.data[18] == 0xff && f.data[19] == 0xc0);
    return Shape{f.data[27], f.data[29]};
}

struct FakePool {
    std::mutex mu;
    ipx_ticket next = 1;
    std::map<ipx_ticket, ipx_job> jobs;
    long long jobs_of_ncomp[5] = {0, 0, 0, 0, 0}, mixed = 0, largest = 0;
};
thread_local std::string g_err;

int fake_submit(void *self, const ipx_job *j, ipx_ticket *t)
{
    FakePool *p = (FakePool *)self;
    REQUIRE(j->kind == IPX_JOB_JPEG && j->n >= 1);
    const Shape first = shape_of(j->files[0]);
    bool mixed = false;
    for (int i = 1; i < j->n; i++) {
        const Shape s = shape_of(j->files[i]);
        mixed = mixed || s.ncomp != first.ncomp || s.hv != first.hv;
    }
    std::lock_guard<std::mutex> lk(p->mu);
    p->mixed += mixed;
    p->jobs_of_ncomp[first.ncomp]++;
    p->largest = std::max<long long>(p->largest, j->n);
    *t = p->next++;
    p->jobs[*t] = *j;
    return IPX_OK;
}
int fake_wait(void *self, ipx_ticket t)
{
    FakePool *p = (FakePool *)self;
    std::lock_guard<std::mutex> lk(p->mu);
    auto it = p->jobs.find(t);
    REQUIRE(it != p->jobs.end());
    for (int i = 0; i < it->second.n; i++) { it->second.status[i] = IPX_OK; it->second.resize_jpeg[i] = it->second.files[i]; }
    return IPX_OK;
}
int fake_release(void *self, ipx_ticket t)
{
    FakePool *p = (FakePool *)self;
    std::lock_guard<std::mutex> lk(p->mu);
    REQUIRE(p->jobs.erase(t) == 1);
    return IPX_OK;
}

}  // namespace

int main()
{
    using namespace ipx;
    FakePool pool;
    BatchBackend be;
    be.self = &pool; be.submit = fake_submit; be.wait = fake_wait; be.release = fake_release;
    be.last_error = [] { return g_err.c_str(); };
    const int nthreads = 4, per_thread = 100, max_batch = 16;
    std::vector<std::deque<std::vector<uint8_t>>> files(nthreads);
    std::atomic<long long> ok{0};
    {
        Batcher b(be, max_batch, 2000, 85, 0);        // size and timer only: groups fill up, so a shared key would show
        std::vector<std::thread> ts;
        for (int th = 0; th < nthreads; th++)
            ts.emplace_back([&, th] {
                std::vector<std::pair<uint64_t, size_t>> tickets;
                for (int i = 0; i < per_thread; i++) {
                    files[th].push_back(make_file(kShapes[(i + th) % 5], th * per_thread + i));
                    ipx_pool_ops ops;
                    memset(&ops, 0, sizeof ops);
                    ops.sw = 16; ops.sh = 16; ops.do_resize = 1; ops.resize_w = 8; ops.resize_h = 8;
                    uint64_t t = 0;
                    std::string err;
                    REQUIRE(b.submit(ipx_bytes{files[th].back().data(), files[th].back().size()}, ops, &t, &err) == IPX_OK);
                    tickets.push_back({t, files[th].size() - 1});
                }
                for (auto &tk : tickets) {
                    ipx_batch_result res;
                    memset(&res, 0, sizeof res);
                    std::string err;
                    REQUIRE(b.wait(tk.first, &res, &err) == IPX_OK && res.status == IPX_OK);
                    const std::vector<uint8_t> &src = files[th][tk.second];
                    REQUIRE(res.resize.len == src.size() && !memcmp(res.resize.data, src.data(), src.size()));     // its own file
                    REQUIRE(b.release(tk.first, &err) == IPX_OK);
                    ok++;
                }
            });
        for (auto &t : ts) t.join();
        ipx_batcher_stats st;
        b.stats(&st);
        printf("jpeg4 batcher key: %lld files in %lld batches (%lld by size), largest %lld; jobs of 1 / 3 / 4 components: %lld / %lld / %lld; mixed jobs: %lld\n",
               st.files, st.batches, st.flushed_by_size, st.largest_batch, pool.jobs_of_ncomp[1], pool.jobs_of_ncomp[3], pool.jobs_of_ncomp[4], pool.mixed);
        if (st.files != nthreads * per_thread || st.largest_batch > max_batch) return 2;
    }
    if (ok != nthreads * per_thread || !pool.jobs.empty()) return 3;
    if (pool.mixed || !pool.jobs_of_ncomp[1] || !pool.jobs_of_ncomp[3] || !pool.jobs_of_ncomp[4]) return 4;
    printf("jpeg4 batcher key ok\n");
    return 0;
}
