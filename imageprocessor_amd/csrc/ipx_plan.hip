// ipx_plan.hip -- plans: the geometry, axis tables and one-pass tilings of a set of operators on one frame size, built once and kept
// in HBM, and the context's cache of plans by content.  What runs a plan on a batch: ipx_runtime.hip.
#include <cstddef>
#include <new>

#include "ipx_runtime_internal.h"

extern "C" {

// ---- plans -------------------------------------------------------------------------------------------
int ipx_plan_create(ipx_ctx *ctx, const ipx_plan_params *p, ipx_plan **out) try
{
    IPX_ENTER(ctx);
    if (!p || !out) { set_error("ipx_plan_create: bad argument"); return IPX_ERR_INVALID; }
    *out = nullptr;
    if (p->sw <= 0 || p->sh <= 0) { set_error("ipx_plan_create: frame size %dx%d", p->sw, p->sh); return IPX_ERR_INVALID; }
    if (!frame_span_ok(p->sw, p->sh, (long long)p->sw * 4, 4)) {
        set_error("ipx_plan_create: a %dx%d frame is beyond the 2 GiB / 65535-pixel span the kernels address", p->sw, p->sh);
        return IPX_ERR_UNSUPPORTED;
    }
    ipx_plan *pl = new (std::nothrow) ipx_plan;
    if (!pl) { set_error("out of memory"); return IPX_ERR_NOMEM; }
    pl->p = *p;
    int rc = IPX_OK;
    const int sw = p->sw, sh = p->sh;
    if (p->do_resize) {
        int nw, nh;
        rc = ipx_resize_dims(sw, sh, p->resize_w, p->resize_h, p->keep_aspect, &nw, &nh);
        if (rc) { delete pl; return rc; }
        if (!frame_span_ok(nw, nh, (long long)nw * 4, 4)) {
            set_error("ipx_plan_create: a %dx%d resize output is beyond the 2 GiB / 65535-pixel span the kernels address", nw, nh);
            delete pl;
            return IPX_ERR_UNSUPPORTED;
        }
        pl->sc[0].on = true; pl->sc[0].dw = nw; pl->sc[0].dh = nh; pl->sc[0].sr = Rect{0, 0, sw, sh};
        pl->info.resize_w = nw; pl->info.resize_h = nh;
        pl->info.resize_bytes = (size_t)nw * nh * 4;
    }
    if (p->do_thumbnail) {
        int nw, nh;
        ipx_rect crop;
        rc = ipx_thumb_geometry(sw, sh, p->thumb_size, p->crop_to_fit, &crop, &nw, &nh);
        if (rc) { delete pl; return rc; }
        if (!frame_span_ok(nw, nh, (long long)nw * 4, 4)) {
            set_error("ipx_plan_create: a %dx%d thumbnail is beyond the 2 GiB / 65535-pixel span the kernels address", nw, nh);
            delete pl;
            return IPX_ERR_UNSUPPORTED;
        }
        pl->sc[1].on = true; pl->sc[1].dw = nw; pl->sc[1].dh = nh; pl->sc[1].sr = to_rect(crop);
        pl->info.thumb_w = nw; pl->info.thumb_h = nh; pl->info.thumb_crop = crop;
        pl->info.thumb_bytes = (size_t)nw * nh * 4;
    }
    if (p->do_watermark) {
        pl->info.wm_w = sw; pl->info.wm_h = sh;
        pl->info.wm_bytes = (size_t)sw * sh * 4;
        if (p->glyphs) {
            rc = glyphs_for_frame(p->glyphs, sw, sh, &pl->glyphs);
            if (rc) { delete pl; return rc; }
        }
    }
    pl->info.algorithmic_bytes = (size_t)sw * sh * 4 + pl->info.resize_bytes + pl->info.thumb_bytes + pl->info.wm_bytes;

    // newDistrib of both axes of every scaled output (an output with a zero dimension -- resize.go:70-72 has no guard -- is simply empty)
    std::vector<uint8_t> blob;
    auto put = [&](size_t bytes) {
        const size_t off = align16(blob.size());
        blob.resize(off + bytes);
        return off;
    };
    size_t axoff[2][2] = {{0, 0}, {0, 0}};
    bool have[2] = {false, false};
    for (int k = 0; k < 2; k++) {
        PlanScale &sk = pl->sc[k];
        if (!sk.on || sk.dw <= 0 || sk.dh <= 0) continue;
        if (!ks_build_axis(sk.dw, sk.sr.dx(), &sk.hx) || !ks_build_axis(sk.dh, sk.sr.dy(), &sk.hy)) {
            set_error("ipx_plan_create: cannot tabulate the axes of a %dx%d <- %dx%d scale", sk.dw, sk.dh, sk.sr.dx(), sk.sr.dy());
            delete pl;
            return IPX_ERR_INVALID;
        }
        have[k] = true;
        axoff[k][0] = put(ks_axis_bytes(sk.hx));
        axoff[k][1] = put(ks_axis_bytes(sk.hy));
    }
    // the one-pass kernel's tiling and tables (source pixels of 4 bytes in LDS)
    KsFusedIn fin[2];
    for (int k = 0; k < 2; k++) {
        const PlanScale &sk = pl->sc[k];
        fin[k].dw = sk.dw; fin[k].dh = sk.dh; fin[k].sr_x0 = sk.sr.x0; fin[k].sr_y0 = sk.sr.y0; fin[k].hx = &sk.hx; fin[k].hy = &sk.hy;
    }
    size_t fused_off[3] = {0, 0, 0};
    if (!env_int("IPX_NO_FUSE", 0)) {
        const int px_bytes[3] = {4, 8, 2};
        for (int f = 0; f < 3; f++) {
            std::vector<uint8_t> fblob;
            fin[1].top_taps = f == 1 && pl->p.crop_to_fit;       // (the YCbCr and NRGBA sources' crop thumbnails: IPX_SRC_YCBCR_CROP / IPX_SRC_NRGBA_CROP taps)
            if (ks_fused_plan(sw, sh, have[0] ? &fin[0] : nullptr, have[1] ? &fin[1] : nullptr, px_bytes[f], &fblob, &pl->fused[f])) {
                fused_off[f] = put(fblob.size());
                memcpy(blob.data() + fused_off[f], fblob.data(), fblob.size());
            }
        }
    }
    if (!blob.empty()) {
        hipError_t e = hipMalloc((void **)&pl->blob, blob.size());
        if (e != hipSuccess) {
            set_error("plan table allocation failed: %s", hipGetErrorString(e));
            ipx_plan_destroy(ctx, pl);
            return IPX_ERR_NOMEM;
        }
        for (int k = 0; k < 2; k++) {
            if (!have[k]) continue;
            ks_axis_pack(pl->sc[k].hx, blob.data() + axoff[k][0], pl->blob + axoff[k][0], &pl->sc[k].ax[0]);
            ks_axis_pack(pl->sc[k].hy, blob.data() + axoff[k][1], pl->blob + axoff[k][1], &pl->sc[k].ax[1]);
        }
        for (int f = 0; f < 3; f++)
            if (pl->fused[f].ok) ks_fused_rebase(&pl->fused[f], pl->blob + fused_off[f]);
        e = hipMemcpy(pl->blob, blob.data(), blob.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            set_error("plan table upload failed: %s", hipGetErrorString(e));
            ipx_plan_destroy(ctx, pl);
            return IPX_ERR_HIP;
        }
    }
    *out = pl;
    return IPX_OK;
}
IPX_CATCH_STATUS

void ipx_plan_destroy(ipx_ctx *ctx, ipx_plan *plan)
{
    if (!plan) return;
    if (ctx) (void)hipSetDevice(ctx->device);
    if (plan->blob) (void)hipFree(plan->blob);
    if (plan->owned_gs) ipx_glyphset_destroy(ctx, plan->owned_gs);
    delete plan;
}

// ---- plans by content --------------------------------------------------------------------------------------------------------
// The per-operator entries (ipx_*_process, ipx_processor_process) and the pool describe their operators per call; building a glyph set
// and a plan per call cost three hipMalloc / hipFree pairs, each of which waits for every stream of the device.  The context keeps
// plans (with their glyph sets) by content instead: operator parameters, colour, and every glyph's rectangle and mask bytes.
// The cache holds at most IPX_PLAN_CACHE_MAX (256) plans; a new content then takes the place of the plan that was handed out longest
// ago and that no call holds (a worker fed arbitrary upload sizes would otherwise fill the cache with sizes it never sees again, and
// sizes that become frequent later could not enter).
static size_t max_cached_plans() { return (size_t)std::max(1, env_int("IPX_PLAN_CACHE_MAX", 256)); }

static int ops_key(const ipx_pool_ops &in, std::string *key)
{
    if (in.n_glyphs < 0 || (in.n_glyphs && !in.glyphs)) { set_error("bad glyph list"); return IPX_ERR_INVALID; }
    key->assign((const char *)&in, offsetof(ipx_pool_ops, glyphs));
    key->append((const char *)in.col, 4);
    for (int i = 0; i < in.n_glyphs; i++) {
        const ipx_glyph &g = in.glyphs[i];
        if (g.mw < 0 || g.mh < 0 || (g.mw && g.mh && (!g.mask || g.mstride < g.mw))) { set_error("glyph %d has a bad mask", i); return IPX_ERR_INVALID; }
        key->append((const char *)&g.mw, sizeof(int32_t) * 2);
        key->append((const char *)&g.dr, sizeof g.dr);
        key->append((const char *)&g.mpx, sizeof(int32_t) * 2);
        for (int y = 0; y < g.mh; y++) key->append((const char *)g.mask + (size_t)y * g.mstride, (size_t)g.mw);
    }
    return IPX_OK;
}

int ipx_plan_acquire(ipx_ctx *ctx, const ipx_pool_ops *ops, ipx_plan **plan, int *cached) try
{
    IPX_ENTER(ctx);
    if (!ops || !plan || !cached) { set_error("ipx_plan_acquire: bad argument"); return IPX_ERR_INVALID; }
    *plan = nullptr; *cached = 0;
    std::string key;
    int rc = ops_key(*ops, &key);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(ctx->plan_mu);      // (a miss builds under the lock: two callers with the same new content build once)
    const bool use_cache = env_int("IPX_PLAN_CACHE", 1) != 0;     // 0: a plan per call, as before the cache existed (tools/bench_seam.py)
    auto it = ctx->plan_cache.find(key);
    if (use_cache && it != ctx->plan_cache.end()) {
        *plan = it->second.second; *cached = 1;
        (*plan)->cache_refs++; (*plan)->cache_stamp = ++ctx->plan_clock;
        return IPX_OK;
    }
    ipx_glyphset *gs = nullptr;
    if (ops->do_watermark && ops->n_glyphs > 0) {
        rc = ipx_glyphset_create(ctx, ops->glyphs, ops->n_glyphs, ops->col, &gs);
        if (rc) return rc;
    }
    ipx_plan_params pp;
    memset(&pp, 0, sizeof pp);
    pp.sw = ops->sw; pp.sh = ops->sh;
    pp.do_resize = ops->do_resize; pp.resize_w = ops->resize_w; pp.resize_h = ops->resize_h; pp.keep_aspect = ops->keep_aspect;
    pp.do_thumbnail = ops->do_thumbnail; pp.thumb_size = ops->thumb_size; pp.crop_to_fit = ops->crop_to_fit;
    pp.do_watermark = ops->do_watermark; pp.glyphs = gs;
    ipx_plan *pl = nullptr;
    rc = ipx_plan_create(ctx, &pp, &pl);
    if (rc) { if (gs) ipx_glyphset_destroy(ctx, gs); return rc; }
    pl->owned_gs = gs;
    if (use_cache && ctx->plan_cache.size() >= max_cached_plans()) {   // make room: the least recently used plan nobody holds
        auto victim = ctx->plan_cache.end();
        for (auto i2 = ctx->plan_cache.begin(); i2 != ctx->plan_cache.end(); ++i2)
            if (i2->second.second->cache_refs == 0 && (victim == ctx->plan_cache.end() || i2->second.second->cache_stamp < victim->second.second->cache_stamp))
                victim = i2;
        if (victim != ctx->plan_cache.end()) {
            ipx_plan_destroy(ctx, victim->second.second);               // (hipFree waits for the launches that still read its tables)
            ctx->plan_cache.erase(victim);
        }
    }
    if (use_cache && ctx->plan_cache.size() < max_cached_plans()) {
        pl->cache_refs = 1; pl->cache_stamp = ++ctx->plan_clock;
        ctx->plan_cache.emplace(std::move(key), std::make_pair(gs, pl));
        *cached = 1;
    }
    *plan = pl;
    return IPX_OK;
}
IPX_CATCH_STATUS

void ipx_plan_release(ipx_ctx *ctx, ipx_plan *plan, int cached)
{
    if (!plan) return;
    if (!cached) { ipx_plan_destroy(ctx, plan); return; }   // a plan the cache did not take (every cached plan was in use) lives for one call
    if (!ctx) return;
    std::lock_guard<std::mutex> lk(ctx->plan_mu);
    if (plan->cache_refs > 0) plan->cache_refs--;
}

int ipx_plan_query(const ipx_plan *plan, ipx_plan_info *info) try
{
    clear_error();
    if (!plan || !info) { set_error("ipx_plan_query: bad argument"); return IPX_ERR_INVALID; }
    *info = plan->info;
    return IPX_OK;
}
IPX_CATCH_STATUS

}  // extern "C"
