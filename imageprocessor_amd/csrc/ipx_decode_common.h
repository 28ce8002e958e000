// ipx_decode_common.h -- the host scaffolding the three decode drivers share (jpeg_decode_files in ipx_jpeg_dec_runtime.hip,
// gif_decode_files in ipx_gif_dec.hip, png_decode_files in ipx_png_dec_runtime.hip).  What a driver schedules, and the
// JPEG driver's lane arena, stay with the driver.  Not part of the ABI.
#pragma once

#include <atomic>
#include <functional>
#include <memory>
#include <string>

#include "ipx_runtime_internal.h"
#include "ipx_threads.h"

// ---- the device blocks a decode entry hands to its caller: stream-ordered allocations of `stream` --------------------------------------
struct DevBlocks { std::vector<void *> dev; hipStream_t stream = nullptr; };
struct ipx_jpeg_planes : DevBlocks {};
struct ipx_gif_frames : DevBlocks {};
struct ipx_png_frames : DevBlocks {};

template <class T> inline void dev_blocks_free(ipx_ctx *ctx, T *o)
{
    if (!o) return;
    if (ctx) (void)hipSetDevice(ctx->device);
    // stream-ordered, like the allocation: hipMalloc / hipFree wait for EVERY stream of the device, and with several decodes in flight on
    // lanes of their own each such call waited for all the others' kernels (four concurrent parts: 0.9 s per decode instead of 0.03 s)
    for (void *p : o->dev) (void)hipFreeAsync(p, o->stream);
    delete o;
}

// An entry's blocks while it runs: freed on every way out but release(), which hands them to the caller.
template <class T> struct OwnedBlocks {
    ipx_ctx *ctx;
    std::unique_ptr<T> o;
    OwnedBlocks(ipx_ctx *c, hipStream_t s) : ctx(c), o(new T) { o->stream = s; }
    ~OwnedBlocks() { dev_blocks_free(ctx, o.release()); }
    template <class P> hipError_t alloc(P **p, size_t bytes)
    {
        const hipError_t e = hipMallocAsync((void **)p, bytes ? bytes : 1, o->stream);
        if (e == hipSuccess) o->dev.push_back(*p);
        return e;
    }
    T *release() { return o.release(); }
};

// ---- a mixed-size JPEG decode in its two halves (ipx_jpeg_dec_runtime.hip), for ipx_jpeg_decode_mixed and the mixed-size leg ------------
// Every file parsed once: status[i] the parser's verdict, *all what the decode needs of the files.
int jpeg_mixed_parse(const ipx_bytes *jpegs, int n, int *status, ipx::JpegBatchPlan *all);
// The m files idx[0 .. m) of that call whose status is IPX_OK, of any sizes and samplings: one run of the decode stages per sampling
// class, each class's files in idx's order, so files of one size and class that are neighbours in idx have planes one frame stride apart
// (256-byte aligned plane sizes).  frames and status by the caller's index; a file is decoded once (its parse is used up).  The planes
// are blocks of `own`; lane != NULL: scratch is bumped out of the lane's decode buffer.
int jpeg_mixed_decode(ipx_ctx *ctx, hipStream_t s, Lane *lane, const ipx_bytes *jpegs, ipx::JpegBatchPlan &all, const int *idx, int m,
                      OwnedBlocks<ipx_jpeg_planes> &own, ipx_jpeg_frame *frames, int *status);

// ---- the pinned blocks of one call (ipx_host_alloc): they go back once the stream is past the copies that read them --------------------
// Like StreamSync, declare it AFTER the host buffers the stream still reads or writes.
struct PinnedBlocks {
    ipx_ctx *ctx;
    hipStream_t s;
    std::vector<void *> p;
    PinnedBlocks(ipx_ctx *c, hipStream_t stream) : ctx(c), s(stream) {}
    PinnedBlocks(const PinnedBlocks &) = delete;
    ~PinnedBlocks()
    {
        (void)hipStreamSynchronize(s);
        if (p.empty()) return;
        const std::string text = ipx_last_error();      // (ipx_host_free clears it: a failing call keeps its text)
        for (void *q : p) (void)ipx_host_free(ctx, q);
        if (!text.empty()) set_error("%s", text.c_str());
    }
    uint8_t *get(size_t bytes)          // null: out of pinned memory, with ipx_host_alloc's text
    {
        uint8_t *q = (uint8_t *)ipx_host_alloc(ctx, bytes);
        if (q) p.push_back(q);
        return q;
    }
};

// ---- loops over the process-wide host pool (ipx_threads.h) -----------------------------------------------------------------------------
// fn(i) for i in [0, count) on at most `threads` threads.  An exception inside a worker (allocation) becomes the status returned, with
// `what` as the error text.
inline int parallel_guarded(int count, int threads, const std::function<void(int)> &fn, const char *what)
{
    std::atomic<int> failed{IPX_OK};
    HostPool::instance().parallel_for(count, threads, [&](int i) {
        const int rc = guarded_status([&] { fn(i); }, nullptr);
        if (rc) failed = rc;
    });
    if (failed) set_error("%s", what);
    return failed;
}
// light items (a file's markers, a memcpy): a thread per eight of them, up to 16; heavy items (a file's scans): a thread each, up to 16
inline int parallel_light(int count, const std::function<void(int)> &fn, const char *what) { return parallel_guarded(count, std::max(1, std::min(count / 8, 16)), fn, what); }
inline int parallel_heavy(int count, const std::function<void(int)> &fn, const char *what) { return parallel_guarded(count, 16, fn, what); }

inline bool any_ok(const int *status, int n) { return std::any_of(status, status + n, [](int s) { return s == IPX_OK; }); }

// Cuts `items` into consecutive groups whose need(item) sum to at most `budget` (an item beyond the budget gets a group of its own) and
// calls run(group) for each; the first status other than IPX_OK ends the walk.
template <class Need, class Run> inline int for_groups_under(const std::vector<int> &items, size_t budget, Need need, Run run)
{
    std::vector<int> group;
    size_t bytes = 0;
    for (int i : items) {
        const size_t b = need(i);
        if (!group.empty() && bytes + b > budget) {
            const int rc = run(group);
            if (rc) return rc;
            group.clear();
            bytes = 0;
        }
        group.push_back(i);
        bytes += b;
    }
    return group.empty() ? IPX_OK : run(group);
}
