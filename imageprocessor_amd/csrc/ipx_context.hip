// ipx_context.hip -- the context and what hangs off it directly: staging lanes, pinned and device memory, streams, events and the
// probe of the host link.  The operators and the plans live in ipx_image_ops.hip, ipx_text.hip, ipx_plan.hip and ipx_runtime.hip.
//
// Threading model (worker.go:88-96: WORKER_CONCURRENCY goroutines share one processor): a
// context is safe to call from any number of OS threads.  Host-pointer calls borrow one of
// `lanes` staging lanes (stream + device scratch), blocking only when all lanes are busy;
// device-pointer calls are plain asynchronous launches on the caller's stream.
#include <chrono>
#include <new>
#include <thread>

#include "ipx_runtime_internal.h"

extern "C" {

static void prepare_hip_env();
int ipx_device_count(void) try
{
    prepare_hip_env();
    clear_error();
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { (void)hipGetLastError(); set_error("hipGetDeviceCount: %s", hipGetErrorString(e)); return IPX_ERR_NODEVICE; }
    return n;
}
IPX_CATCH_STATUS

// ROCclr maps HIP streams onto a fixed number of hardware queues per device (GPU_MAX_HW_QUEUES, 4 by default) and reads the variable
// when the runtime initialises.  A context opens its own stream and five lane streams: with four queues the high-priority lane that
// serves single-frame calls shared a queue with a batch lane in about one context of ten, and its calls then waited for the batch
// (tools/seam_hunt.py).  So before the first HIP call of the process the variable is set -- unless the operator has set it -- to hold
// every stream of a default context on a queue of its own.
static void prepare_hip_env()
{
    static std::once_flag once;
    std::call_once(once, [] {
        if (!getenv("GPU_MAX_HW_QUEUES")) {
            char v[16];
            snprintf(v, sizeof v, "%d", std::max(8, env_int("IPX_LANES", 5) + 3));
            setenv("GPU_MAX_HW_QUEUES", v, 0);
        }
    });
}

int ipx_create(const ipx_config *cfg, ipx_ctx **out) try
{
    clear_error();
    if (!out) { set_error("ipx_create: null out"); return IPX_ERR_INVALID; }
    *out = nullptr;
    prepare_hip_env();
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        set_error("no HIP device visible: the pixel path has no CPU fallback");
        return IPX_ERR_NODEVICE;
    }
    int dev = cfg ? cfg->device : -1;
    if (dev < 0) dev = env_int("IPX_DEVICE", env_int("LOCAL_RANK", 0) % ndev);
    if (dev >= ndev) { set_error("device %d out of range (%d visible)", dev, ndev); return IPX_ERR_INVALID; }
    IPX_HIP(hipSetDevice(dev));
    hipDeviceProp_t prop;
    IPX_HIP(hipGetDeviceProperties(&prop, dev));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error("device %d is %s; libipx carries gfx950 code only", dev, prop.gcnArchName);
        return IPX_ERR_NODEVICE;
    }
    ipx_ctx *c = new (std::nothrow) ipx_ctx;
    if (!c) { set_error("out of memory"); return IPX_ERR_NOMEM; }
    c->device = dev;
    c->cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    int lanes = cfg && cfg->lanes > 0 ? cfg->lanes : env_int("IPX_LANES", 5);
    c->lane_bytes = cfg && cfg->lane_bytes ? cfg->lane_bytes : (size_t)64 << 20;
    c->host_cache_limit = (size_t)std::max(0, env_int("IPX_HOST_CACHE_MB", 8192)) << 20;
    c->lanes.resize(lanes);
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    // the last lane is the one a batch leaves free: single-frame calls land on it, ahead of the batch's queued work.  Its stream is
    // created first: streams take hardware queues in the order they are made
    hipError_t e = hipSuccess;
    if (c->lanes.size() >= 3) e = hipStreamCreateWithPriority(&c->lanes.back().stream, hipStreamNonBlocking, prio_hi);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    for (size_t i = 0; i < c->lanes.size(); i++) {
        Lane &l = c->lanes[i];
        if (e == hipSuccess && !l.stream) e = hipStreamCreateWithFlags(&l.stream, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipMalloc((void **)&l.flag, sizeof(int));
    }
    if (e == hipSuccess) {
        // stream-ordered scratch (the codecs' coefficient arrays, gigabytes per batch) comes from the device's default pool; with the
        // default release threshold of 0 every synchronisation hands the freed memory back to the driver and the next batch maps it
        // again.  Keep up to IPX_POOL_KEEP_GB (64) in the pool.
        hipMemPool_t pool = nullptr;
        if (hipDeviceGetDefaultMemPool(&pool, dev) == hipSuccess && pool) {
            uint64_t keep = (uint64_t)std::max(0, env_int("IPX_POOL_KEEP_GB", 64)) << 30;
            (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
        }
        (void)hipGetLastError();
    }
    if (e == hipSuccess) e = hipMalloc((void **)&c->flat_chroma, ipx_ctx::kFlatChromaBytes);
    if (e == hipSuccess) e = hipMemset(c->flat_chroma, 128, ipx_ctx::kFlatChromaBytes);
    if (e != hipSuccess) {
        set_error("context setup failed: %s", hipGetErrorString(e));
        ipx_destroy(c);
        return IPX_ERR_HIP;
    }
    *out = c;
    return IPX_OK;
}
IPX_CATCH_STATUS

void ipx_destroy(ipx_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    for (auto &l : c->lanes) {
        if (l.stream) { (void)hipStreamSynchronize(l.stream); (void)hipStreamDestroy(l.stream); }
        if (l.dev) (void)hipFree(l.dev);
        if (l.pin) (void)hipHostFree(l.pin);
        for (auto &ev : l.ev) if (ev) (void)hipEventDestroy(ev);
        if (l.dec) (void)hipFree(l.dec);
        if (l.flag) (void)hipFree(l.flag);
    }
    if (c->stream) { (void)hipStreamSynchronize(c->stream); (void)hipStreamDestroy(c->stream); }
    if (c->flat_chroma) (void)hipFree(c->flat_chroma);
    for (auto &e : c->ks_axes) (void)hipFree(e.second.first);
    for (auto &kv : c->plan_cache) ipx_plan_destroy(c, kv.second.second);     // (their glyph sets go with them)
    c->plan_cache.clear();
    for (auto &b : c->host_free_blocks) (void)hipHostFree(b.second);
    delete c;
}

// ---- memory ------------------------------------------------------------------------------------
void *ipx_host_alloc(ipx_ctx *ctx, size_t bytes)
{
    clear_error();
    if (!ctx || !bytes) { set_error("ipx_host_alloc: bad argument"); return nullptr; }
    const size_t want = (bytes + ((size_t)1 << 20) - 1) & ~(((size_t)1 << 20) - 1);   // 1 MiB classes
    {
        std::lock_guard<std::mutex> lk(ctx->host_mu);
        auto it = ctx->host_free_blocks.lower_bound(want);
        if (it != ctx->host_free_blocks.end() && it->first <= 2 * want + ((size_t)4 << 20)) {
            void *p = it->second;
            ctx->host_cached -= it->first;
            ctx->host_size[p] = it->first;
            ctx->host_free_blocks.erase(it);
            ctx->host_lru.erase(std::find(ctx->host_lru.begin(), ctx->host_lru.end(), p));
            return p;
        }
    }
    void *p = nullptr;
    if (getenv("IPX_DEBUG")) fprintf(stderr, "[ipx] pinning %zu MiB (cache holds %zu MiB in %zu blocks)\n", want >> 20, ctx->host_cached >> 20, ctx->host_free_blocks.size());
    // A fresh block is pinned on a thread bound to the CPUs next to the context's GPU (sysfs local_cpulist), so that its pages land on
    // that NUMA node: measured on the driver's two-socket box, copies from and to such blocks move 80 GB/s both directions summed against
    // 57 GB/s for blocks pinned wherever the calling thread happened to run (bench.py's pool leg against its context leg, round 3).
    // Rare: freed blocks are cached (below).  IPX_POOL_NUMA=0 switches the binding off.
    hipError_t e = hipSuccess;
    {
        std::thread t([&] {
            (void)hipSetDevice(ctx->device);
            bind_near_device(ctx->device);
            e = hipHostMalloc(&p, want, hipHostMallocDefault);
            if (e == hipSuccess && env_int("IPX_HOST_TOUCH", 1)) memset(p, 0, want);     // first touch, where the pages are to live
        });
        t.join();
    }
    if (e != hipSuccess) { (void)hipGetLastError(); set_error("hipHostMalloc(%zu): %s", want, hipGetErrorString(e)); return nullptr; }
    std::lock_guard<std::mutex> lk(ctx->host_mu);
    ctx->host_size[p] = want;
    return p;
}

int ipx_host_free(ipx_ctx *ctx, void *p) try
{
    IPX_ENTER(ctx);
    if (!p) return IPX_OK;
    std::vector<void *> victims;     // unpinned outside the lock
    bool cached = false;
    {
        std::lock_guard<std::mutex> lk(ctx->host_mu);
        auto it = ctx->host_size.find(p);
        if (it != ctx->host_size.end()) {
            const size_t sz = it->second;
            ctx->host_size.erase(it);
            if (sz <= ctx->host_cache_limit) {
                // keep the block; make room by dropping the blocks that have gone unused the longest (a cache full of sizes nobody
                // asks for any more would otherwise make every later call pin fresh memory, ~0.2 ms per MB)
                while (ctx->host_cached + sz > ctx->host_cache_limit && !ctx->host_lru.empty()) {
                    void *old = ctx->host_lru.front();
                    ctx->host_lru.pop_front();
                    for (auto fb = ctx->host_free_blocks.begin(); fb != ctx->host_free_blocks.end(); ++fb)
                        if (fb->second == old) { ctx->host_cached -= fb->first; ctx->host_free_blocks.erase(fb); break; }
                    victims.push_back(old);
                }
                ctx->host_free_blocks.emplace(sz, p);
                ctx->host_lru.push_back(p);
                ctx->host_cached += sz;
                cached = true;
            }
        }
    }
    hipError_t e = hipSuccess;
    for (void *v : victims) { hipError_t e2 = hipHostFree(v); if (e == hipSuccess) e = e2; }
    if (!cached) { hipError_t e2 = hipHostFree(p); if (e == hipSuccess) e = e2; }
    IPX_HIP(e);
    return IPX_OK;
}
IPX_CATCH_STATUS

void *ipx_dev_alloc(ipx_ctx *ctx, size_t bytes)
{
    clear_error();
    if (!ctx || !bytes) { set_error("ipx_dev_alloc: bad argument"); return nullptr; }
    (void)hipSetDevice(ctx->device);
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) { (void)hipGetLastError(); set_error("hipMalloc(%zu): %s", bytes, hipGetErrorString(e)); return nullptr; }
    return p;
}

int ipx_dev_free(ipx_ctx *ctx, void *p) try
{
    IPX_ENTER(ctx);
    if (p) IPX_HIP(hipFree(p));
    return IPX_OK;
}
IPX_CATCH_STATUS

int ipx_memcpy_h2d(ipx_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes) try
{
    IPX_ENTER(ctx);
    if (bytes) IPX_HIP(hipMemcpy(dst_dev, src_host, bytes, hipMemcpyHostToDevice));
    return IPX_OK;
}
IPX_CATCH_STATUS

int ipx_memcpy_d2h(ipx_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes) try
{
    IPX_ENTER(ctx);
    if (bytes) IPX_HIP(hipMemcpy(dst_host, src_dev, bytes, hipMemcpyDeviceToHost));
    return IPX_OK;
}
IPX_CATCH_STATUS

int ipx_memcpy_d2d(ipx_ctx *ctx, void *dst_dev, const void *src_dev, size_t bytes) try
{
    IPX_ENTER(ctx);
    // A device-to-device hipMemcpy returns before the copy has run, and the null stream it runs on does not order against the
    // context's non-blocking streams: a launch queued right after it could read the destination half copied (a 1024-slot test batch
    // tiled with this call did, once).  Queue it on the context's stream and wait: done on return, like the two host copies.
    if (bytes) {
        IPX_HIP(hipMemcpyAsync(dst_dev, src_dev, bytes, hipMemcpyDeviceToDevice, ctx->stream));
        IPX_HIP(hipStreamSynchronize(ctx->stream));
    }
    return IPX_OK;
}
IPX_CATCH_STATUS

int ipx_stream_copy(ipx_ctx *ctx, void *stream, void *dst_dev, const void *src_dev, size_t bytes) try
{
    IPX_ENTER(ctx);
    if (((uintptr_t)dst_dev | (uintptr_t)src_dev | bytes) & 15) { set_error("ipx_stream_copy: pointers and size must be multiples of 16"); return IPX_ERR_INVALID; }
    if (bytes) IPX_HIP(launch_stream_copy(dst_dev, src_dev, bytes, stream ? (hipStream_t)stream : ctx->stream));
    return IPX_OK;
}
IPX_CATCH_STATUS

// What the host link gives pinned copies on this box, in this process: one direction alone, and both at once with the byte mix of a
// call (bench.py holds the PCIe-inclusive legs against it).  Not part of the path.
}  // extern "C"
namespace {
__global__ void link_store_kernel(uint4 *__restrict__ dst, const uint4 *__restrict__ src, size_t n16)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i];
}
}  // namespace
extern "C" {

int ipx_link_probe(ipx_ctx *ctx, size_t up_bytes, size_t down_bytes, int reps, double out_gbps[4]) try
{
    IPX_ENTER(ctx);
    if (!out_gbps || !up_bytes || !down_bytes || (down_bytes & 15) || reps < 1) { set_error("ipx_link_probe: bad argument"); return IPX_ERR_INVALID; }
    uint8_t *hu = (uint8_t *)ipx_host_alloc(ctx, up_bytes), *hd = (uint8_t *)ipx_host_alloc(ctx, down_bytes);
    uint8_t *du = nullptr, *dd = nullptr;
    hipStream_t s1 = nullptr, s2 = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hu && hd ? hipSuccess : hipErrorOutOfMemory;
    if (e == hipSuccess) e = hipMalloc((void **)&du, up_bytes);
    if (e == hipSuccess) e = hipMalloc((void **)&dd, down_bytes);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&s1, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&s2, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    if (e == hipSuccess) { memset(hu, 1, up_bytes); e = hipMemset(dd, 2, down_bytes); }
    uint8_t *hd_dev = nullptr;       // the device's view of the pinned block (ipx_host_alloc maps what it pins)
    if (e == hipSuccess && hipHostGetDevicePointer((void **)&hd_dev, hd, 0) != hipSuccess) { (void)hipGetLastError(); hd_dev = nullptr; }
    const size_t piece = (size_t)std::max(1, env_int("IPX_PROBE_CHUNK_MB", 32)) << 20;
    // down_by_kernel: the download as a kernel's stores into the pinned block (how run_host_packed delivers outputs) instead of a copy
    auto timed = [&](bool up, bool down, bool down_by_kernel, double *gb_up, double *gb_down) {
        double best = 1e30;
        for (int r = 0; r < reps + 1 && e == hipSuccess; r++) {           // (the first repetition warms the path)
            const auto t0 = std::chrono::steady_clock::now();
            if (down && down_by_kernel) {
                hipLaunchKernelGGL(link_store_kernel, dim3(512), dim3(256), 0, s2, (uint4 *)hd_dev, (const uint4 *)dd, down_bytes / 16);
                e = hipGetLastError();
            }
            // copies go in pieces, enqueued alternately: the runtime picks a copy engine per stream when the stream's first copy is
            // enqueued, the lowest one idle at that moment, and two large copies enqueued together land on the same engine
            for (size_t o = 0; e == hipSuccess && (o < up_bytes || o < down_bytes); o += piece) {
                if (up && o < up_bytes) e = hipMemcpyAsync(du + o, hu + o, std::min(piece, up_bytes - o), hipMemcpyHostToDevice, s1);
                if (down && !down_by_kernel && o < down_bytes && e == hipSuccess) e = hipMemcpyAsync(hd + o, dd + o, std::min(piece, down_bytes - o), hipMemcpyDeviceToHost, s2);
            }
            if (e == hipSuccess) e = hipStreamSynchronize(s1);
            if (e == hipSuccess) e = hipStreamSynchronize(s2);
            const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (r > 0) best = std::min(best, sec);
        }
        if (gb_up) *gb_up = up ? up_bytes / best / 1e9 : 0;
        if (gb_down) *gb_down = down ? down_bytes / best / 1e9 : 0;
    };
    if (e == hipSuccess) timed(true, false, false, &out_gbps[0], nullptr);
    if (e == hipSuccess) timed(false, true, false, nullptr, &out_gbps[1]);
    if (e == hipSuccess) timed(true, true, false, &out_gbps[2], &out_gbps[3]);
    if (e == hipSuccess && hd_dev) {        // the better of the two ways down, alone and beside the upload
        double u = 0, d = 0;
        timed(false, true, true, nullptr, &d);
        out_gbps[1] = std::max(out_gbps[1], d);
        if (e == hipSuccess) timed(true, true, true, &u, &d);
        if (e == hipSuccess && u + d > out_gbps[2] + out_gbps[3]) { out_gbps[2] = u; out_gbps[3] = d; }
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (s1) (void)hipStreamDestroy(s1);
    if (s2) (void)hipStreamDestroy(s2);
    if (du) (void)hipFree(du);
    if (dd) (void)hipFree(dd);
    if (hu) (void)ipx_host_free(ctx, hu);
    if (hd) (void)ipx_host_free(ctx, hd);
    if (e != hipSuccess) { set_error("ipx_link_probe: %s", hipGetErrorString(e)); return e == hipErrorOutOfMemory ? IPX_ERR_NOMEM : IPX_ERR_HIP; }
    return IPX_OK;
}
IPX_CATCH_STATUS

int ipx_device_sync(ipx_ctx *ctx) try
{
    IPX_ENTER(ctx);
    IPX_HIP(hipDeviceSynchronize());
    return IPX_OK;
}
IPX_CATCH_STATUS

int ipx_stream_sync(ipx_ctx *ctx, void *stream) try
{
    IPX_ENTER(ctx);
    IPX_HIP(hipStreamSynchronize(stream ? (hipStream_t)stream : ctx->stream));
    return IPX_OK;
}
IPX_CATCH_STATUS

void *ipx_stream_create(ipx_ctx *ctx)
{
    clear_error();
    if (!ctx) return nullptr;
    (void)hipSetDevice(ctx->device);
    hipStream_t st = nullptr;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); set_error("hipStreamCreate failed"); return nullptr; }
    return st;
}

int ipx_stream_destroy(ipx_ctx *ctx, void *stream) try
{
    IPX_ENTER(ctx);
    if (!stream) return IPX_OK;
    IPX_HIP(hipStreamSynchronize((hipStream_t)stream));
    IPX_HIP(hipStreamDestroy((hipStream_t)stream));
    return IPX_OK;
}
IPX_CATCH_STATUS

void *ipx_event_create(ipx_ctx *ctx)
{
    clear_error();
    if (!ctx) return nullptr;
    (void)hipSetDevice(ctx->device);
    hipEvent_t ev = nullptr;
    if (hipEventCreate(&ev) != hipSuccess) { (void)hipGetLastError(); set_error("hipEventCreate failed"); return nullptr; }
    return ev;
}

int ipx_event_record(ipx_ctx *ctx, void *event, void *stream) try
{
    IPX_ENTER(ctx);
    if (!event) { set_error("ipx_event_record: null event"); return IPX_ERR_INVALID; }
    IPX_HIP(hipEventRecord((hipEvent_t)event, stream ? (hipStream_t)stream : ctx->stream));
    return IPX_OK;
}
IPX_CATCH_STATUS

int ipx_event_elapsed_ms(ipx_ctx *ctx, void *start, void *stop, float *ms) try
{
    IPX_ENTER(ctx);
    if (!start || !stop || !ms) { set_error("ipx_event_elapsed_ms: bad argument"); return IPX_ERR_INVALID; }
    IPX_HIP(hipEventSynchronize((hipEvent_t)stop));
    IPX_HIP(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
    return IPX_OK;
}
IPX_CATCH_STATUS

void ipx_event_destroy(ipx_ctx *ctx, void *event)
{
    if (!ctx || !event) return;
    (void)hipSetDevice(ctx->device);
    (void)hipEventDestroy((hipEvent_t)event);
}

}  // extern "C"
