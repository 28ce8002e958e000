// batcher_formats_host_test.cpp -- the batcher's format routing (csrc/ipx_batcher.cpp) on the CPU alone, built with -fsanitize=thread
// (tools/sanitize/run_tsan_formats.sh), beside batcher_host_test.cpp, which keeps the queue / timer / ticket logic on JPEG-shaped
// keys.  The "device" is a fake backend that records the kind of every job; a job's work is done by whoever waits for it (a memcpy
// of every file into "outputs"), and one job in eleven is refused at submit.
//
// A test file is a signature, then a key byte (frame size and operator set), then the submitter and a serial number, then noise.
// The signatures: the 8 bytes of a PNG, "GIF87a", "GIF89a", FF D8, and two that only BEGIN like a PNG (89 50) or a GIF ("GIF8") and
// therefore have to go out as JPEG jobs, as image.Decode would not take them for a PNG or a GIF either.
//
// What it checks: every job holds files of one format, and its kind is the one their signatures name (IPX_JOB_PNG, IPX_JOB_GIF,
// IPX_JOB_JPEG for everything else); one frame size and one operator set per job; every ticket gets its own bytes back; max_batch is
// held; a refused job fails its own files only; destruction with work pending and tickets uncollected is clean; no data race (TSan).
#define IPX_BATCHER_NO_ABI 1
#include "../../imageprocessor_amd/csrc/ipx_batcher.cpp"

#include <atomic>
#include <cstdlib>
#include <cstdio>
#include <deque>
#include <random>

namespace {

struct Sig { const char *bytes; size_t len; int kind; };
const Sig kSigs[6] = {
    {"\x89PNG\r\n\x1a\n", 8, IPX_JOB_PNG}, {"GIF87a", 6, IPX_JOB_GIF}, {"GIF89a", 6, IPX_JOB_GIF}, {"\xff\xd8", 2, IPX_JOB_JPEG},
    {"\x89P", 2, IPX_JOB_JPEG},            // begins like a PNG
    {"GIF8", 4, IPX_JOB_JPEG},             // begins like a GIF
};
// the byte after a test file's signature is its key (0 .. 5), so a short signature never grows into a full one by chance
int sig_of(const ipx_bytes &f)
{
    for (int s = 0; s < 6; s++)
        if (f.len > kSigs[s].len && !memcmp(f.data, kSigs[s].bytes, kSigs[s].len)) return s;   // (full signatures come first)
    return -1;
}
uint8_t key_of(const ipx_bytes &f) { return f.data[kSigs[sig_of(f)].len]; }

struct FakeJob {
    ipx_job job;                       // shallow: the batcher keeps the arrays alive
    std::vector<std::vector<uint8_t>> out;
    bool done = false;
    std::mutex mu;
};
struct FakePool {
    std::mutex mu;
    std::map<ipx_ticket, std::shared_ptr<FakeJob>> jobs;
    ipx_ticket next = 1;
    std::atomic<long long> submitted{0}, largest{0}, released{0};
    std::atomic<long long> jobs_of_kind[10], files_of_kind[10];
    int max_batch = 0;
    FakePool() { for (int k = 0; k < 10; k++) { jobs_of_kind[k] = 0; files_of_kind[k] = 0; } }
};
thread_local std::string g_err;
std::atomic<long long> g_wrong{0};      // jobs of a kind their files do not name, or of mixed content (counted, reported at the end)
// (not assert: the checks hold whatever NDEBUG says)
#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "line %d: %s\n", __LINE__, #c); abort(); } } while (0)
#define CHECK(c) do { if (!(c)) { if (g_wrong++ < 10) fprintf(stderr, "line %d: %s\n", __LINE__, #c); } } while (0)

int fake_submit(void *self, const ipx_job *j, ipx_ticket *t)
{
    FakePool *p = (FakePool *)self;
    CHECK(j->n >= 1 && j->n <= p->max_batch);
    CHECK(j->kind == IPX_JOB_JPEG || j->kind == IPX_JOB_PNG || j->kind == IPX_JOB_GIF);
    for (int i = 0; i < j->n; i++) {
        const int s = sig_of(j->files[i]);
        REQUIRE(s >= 0);
        CHECK(kSigs[s].kind == j->kind);                        // one format per job, and the one the signature names
        CHECK(key_of(j->files[i]) == key_of(j->files[0]));      // one size and operator set per job
    }
    const uint8_t key = key_of(j->files[0]);
    CHECK(j->ops.sw == 100 + key % 3 && j->ops.do_thumbnail == key / 3);
    CHECK(j->quality == 77 && j->status && j->resize_jpeg && !j->wm_jpeg && (j->thumb_jpeg != nullptr) == (key / 3 != 0));
    std::lock_guard<std::mutex> lk(p->mu);
    const ipx_ticket id = p->next++;
    if (id % 11 == 0) { g_err = "fake: submit refused"; return IPX_ERR_NOMEM; }
    auto fj = std::make_shared<FakeJob>();
    fj->job = *j;
    p->jobs[id] = fj;
    p->submitted++;
    if (j->kind >= 0 && j->kind < 10) { p->jobs_of_kind[j->kind]++; p->files_of_kind[j->kind] += j->n; }
    long long l = p->largest.load();
    while (j->n > l && !p->largest.compare_exchange_weak(l, j->n)) { }
    *t = id;
    return IPX_OK;
}
int fake_wait(void *self, ipx_ticket t)
{
    FakePool *p = (FakePool *)self;
    std::shared_ptr<FakeJob> fj;
    {
        std::lock_guard<std::mutex> lk(p->mu);
        auto it = p->jobs.find(t);
        REQUIRE(it != p->jobs.end());
        fj = it->second;
    }
    std::lock_guard<std::mutex> lk(fj->mu);            // the first waiter "runs" the job
    if (!fj->done) {
        std::this_thread::sleep_for(std::chrono::microseconds(150 + (t * 37) % 500));
        fj->out.resize((size_t)fj->job.n);
        for (int i = 0; i < fj->job.n; i++) {
            const ipx_bytes &f = fj->job.files[i];
            fj->out[i].assign(f.data, f.data + f.len);
            fj->job.status[i] = IPX_OK;
            fj->job.resize_jpeg[i] = ipx_bytes{fj->out[i].data(), fj->out[i].size()};
            if (fj->job.thumb_jpeg) fj->job.thumb_jpeg[i] = ipx_bytes{fj->out[i].data(), 3};
        }
        fj->done = true;
    }
    return IPX_OK;
}
int fake_release(void *self, ipx_ticket t)
{
    FakePool *p = (FakePool *)self;
    std::lock_guard<std::mutex> lk(p->mu);
    auto it = p->jobs.find(t);
    REQUIRE(it != p->jobs.end());
    p->jobs.erase(it);
    p->released++;
    return IPX_OK;
}

}  // namespace

int main()
{
    using namespace ipx;
    std::unique_ptr<FakePool> pool_owner(new FakePool);
    FakePool &pool = *pool_owner;
    pool.max_batch = 16;
    BatchBackend be;
    be.self = &pool; be.submit = fake_submit; be.wait = fake_wait; be.release = fake_release;
    be.last_error = [] { return g_err.c_str(); };
    const int nthreads = 8, per_thread = 450;
    std::atomic<long long> ok_files{0}, refused{0};
    std::atomic<long long> sent_of_kind[10];
    for (auto &v : sent_of_kind) v = 0;
    std::vector<std::deque<std::vector<uint8_t>>> all_files(nthreads);   // outlive the batcher: some tickets are never collected
    {
        std::unique_ptr<Batcher> b_owner(new Batcher(be, pool.max_batch, 1500, 77, 3));
        Batcher &b = *b_owner;
        std::vector<std::thread> ts;
        for (int th = 0; th < nthreads; th++)
            ts.emplace_back([&, th] {
                std::mt19937 rng(4321 + th);
                std::deque<std::vector<uint8_t>> &files = all_files[th];
                std::vector<std::pair<uint64_t, size_t>> tickets;       // (ticket, index of its file)
                for (int i = 0; i < per_thread; i++) {
                    const Sig &sig = kSigs[rng() % 6];
                    const uint8_t key = (uint8_t)(rng() % 6);             // three sizes x two operator sets
                    std::vector<uint8_t> f(sig.len + 4 + rng() % 40);
                    for (auto &v : f) v = (uint8_t)rng();
                    memcpy(f.data(), sig.bytes, sig.len);
                    f[sig.len] = key; f[sig.len + 1] = (uint8_t)th; f[sig.len + 2] = (uint8_t)i; f[sig.len + 3] = (uint8_t)(i >> 8);
                    files.push_back(f);
                    sent_of_kind[sig.kind]++;
                    ipx_pool_ops ops;
                    memset(&ops, 0, sizeof ops);
                    ops.sw = 100 + key % 3; ops.sh = 50; ops.do_resize = 1; ops.resize_w = 10; ops.resize_h = 10;
                    ops.do_thumbnail = key / 3; ops.thumb_size = 20;
                    ipx_bytes fb{files.back().data(), files.back().size()};
                    uint64_t t = 0;
                    std::string err;
                    const int rc = b.submit(fb, ops, &t, &err);
                    REQUIRE(rc == IPX_OK);
                    tickets.push_back({t, files.size() - 1});
                    if (rng() % 5 == 0) std::this_thread::sleep_for(std::chrono::microseconds(rng() % 700));
                    // collect in a scrambled order, sometimes late, sometimes never (the destructor has to cope)
                    while (tickets.size() > 24 || (i == per_thread - 1 && tickets.size() > 7)) {
                        const size_t pick = rng() % tickets.size();
                        const uint64_t tk = tickets[pick].first;
                        const std::vector<uint8_t> &src = files[tickets[pick].second];
                        ipx_batch_result res;
                        memset(&res, 0, sizeof res);
                        std::string e2;
                        if (rng() % 13 != 0) {
                            const int r2 = b.wait(tk, &res, &e2);
                            if (r2 == IPX_ERR_NOMEM) { REQUIRE(e2 == "fake: submit refused"); refused++; }
                            else {
                                REQUIRE(r2 == IPX_OK && res.status == IPX_OK);
                                REQUIRE(res.resize.len == src.size() && !memcmp(res.resize.data, src.data(), src.size()));   // its own bytes
                                const bool thumb = key_of(ipx_bytes{src.data(), src.size()}) / 3 != 0;
                                REQUIRE(res.wm.data == nullptr && (res.thumb.data != nullptr) == thumb && (!thumb || (res.thumb.len == 3 && res.thumb.data[0] == src[0])));
                                ok_files++;
                            }
                        }
                        const int r3 = b.release(tk, &e2);
                        REQUIRE(r3 == IPX_OK);
                        tickets.erase(tickets.begin() + (long)pick);
                    }
                }
            });
        for (auto &t : ts) t.join();
        ipx_batcher_stats st;
        b.stats(&st);
        printf("formats: %lld files in %lld batches (%lld by size, %lld by timer, %lld when idle), largest %lld; verified %lld, refused %lld\n", st.files, st.batches,
               st.flushed_by_size, st.flushed_by_timer, st.flushed_when_idle, st.largest_batch, (long long)ok_files, (long long)refused);
        if (st.files != (long long)nthreads * per_thread || st.largest_batch > pool.max_batch ||
            st.batches != st.flushed_by_size + st.flushed_by_timer + st.flushed_when_idle) return 2;
    }   // ~Batcher: pending files flushed, uncollected tickets' jobs waited for and released
    {
        std::lock_guard<std::mutex> lk(pool.mu);
        if (!pool.jobs.empty()) { fprintf(stderr, "%zu jobs were never released\n", pool.jobs.size()); return 3; }
    }
    printf("formats: jobs jpeg %lld png %lld gif %lld; files sent jpeg %lld png %lld gif %lld\n", (long long)pool.jobs_of_kind[IPX_JOB_JPEG],
           (long long)pool.jobs_of_kind[IPX_JOB_PNG], (long long)pool.jobs_of_kind[IPX_JOB_GIF], (long long)sent_of_kind[IPX_JOB_JPEG],
           (long long)sent_of_kind[IPX_JOB_PNG], (long long)sent_of_kind[IPX_JOB_GIF]);
    if (g_wrong) { fprintf(stderr, "%lld checks failed in the backend: jobs of the wrong kind or of mixed content\n", (long long)g_wrong); return 6; }
    if (pool.largest > pool.max_batch) return 2;
    if (ok_files < 1000 || refused == 0) return 4;
    // every format was sent, and every format went out in jobs of its own kind (files of refused jobs are in no count)
    for (int k : {IPX_JOB_JPEG, IPX_JOB_PNG, IPX_JOB_GIF})
        if (sent_of_kind[k] == 0 || pool.jobs_of_kind[k] == 0 || pool.files_of_kind[k] > sent_of_kind[k]) return 5;
    {
        // one operator set, one size, the six signatures: three jobs (PNG; GIF87a with GIF89a; one JPEG job for FF D8, "89 50" and "GIF8")
        FakePool pool2;
        pool2.max_batch = 16;
        BatchBackend be2 = be;
        be2.self = &pool2;
        std::vector<std::vector<uint8_t>> fs;
        for (int i = 0; i < 12; i++) {
            const Sig &sig = kSigs[i % 6];
            std::vector<uint8_t> f(sig.bytes, sig.bytes + sig.len);
            for (int v : {0, 0, i, 0, 9, 9}) f.push_back((uint8_t)v);
            fs.push_back(f);
        }
        {
            Batcher b2(be2, pool2.max_batch, 50000, 77, 0);
            ipx_pool_ops ops;
            memset(&ops, 0, sizeof ops);
            ops.sw = 100; ops.sh = 50; ops.do_resize = 1; ops.resize_w = 10; ops.resize_h = 10;
            for (auto &f : fs) {
                uint64_t t = 0;
                std::string err;
                const int rc = b2.submit(ipx_bytes{f.data(), f.size()}, ops, &t, &err);
                REQUIRE(rc == IPX_OK);
            }
        }   // ~Batcher flushes the groups
        if (pool2.submitted != 3 || pool2.jobs_of_kind[IPX_JOB_PNG] != 1 || pool2.files_of_kind[IPX_JOB_PNG] != 2 || pool2.jobs_of_kind[IPX_JOB_GIF] != 1 ||
            pool2.files_of_kind[IPX_JOB_GIF] != 4 || pool2.jobs_of_kind[IPX_JOB_JPEG] != 1 || pool2.files_of_kind[IPX_JOB_JPEG] != 6 || g_wrong) {
            fprintf(stderr, "look-alikes: %lld jobs (png %lld, gif %lld, jpeg %lld)\n", (long long)pool2.submitted, (long long)pool2.jobs_of_kind[IPX_JOB_PNG],
                    (long long)pool2.jobs_of_kind[IPX_JOB_GIF], (long long)pool2.jobs_of_kind[IPX_JOB_JPEG]);
            return 7;
        }
    }
    printf("batcher formats ok: %lld jobs submitted, %lld released\n", (long long)pool.submitted, (long long)pool.released);
    return 0;
}
