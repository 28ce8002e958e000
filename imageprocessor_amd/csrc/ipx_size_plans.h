// ipx_size_plans.h -- what the mixed-size legs share (ipx_run_png_png_mixed in ipx_png_legs.hip, ipx_run_jpeg_jpeg_mixed in
// ipx_jpeg_legs.hip): a plan per frame size of one call, from the context's cache.  Not part of the ABI.
#pragma once

#include <map>
#include <utility>
#include <vector>

#include "ipx_runtime_internal.h"

// the plans of one call, one per frame size; handed back on every way out
struct SizePlans {
    struct Held { ipx_plan *pl; int cached; };
    ipx_ctx *ctx;
    std::map<std::pair<int, int>, Held> held;
    explicit SizePlans(ipx_ctx *c) : ctx(c) {}
    SizePlans(const SizePlans &) = delete;
    ~SizePlans()
    {
        for (auto &kv : held)
            if (kv.second.pl) ipx_plan_release(ctx, kv.second.pl, kv.second.cached);
    }
};

// A plan per size: (*plan_of)[i] for every file whose status is IPX_OK, of its size w[i] x h[i], with ops' operators.  Files of a size
// no plan can be made for get ipx_plan_create's status, alone, and a null plan.  Every distinct size of the call holds its plan until
// `plans` goes: at most one per file (65535), of which the context's cache keeps IPX_PLAN_CACHE_MAX (256) and the rest live and die
// with the call -- a call with more sizes than that also turns the cache over once.
inline int size_plans_acquire(ipx_ctx *ctx, const ipx_pool_ops *ops, int n, const int *w, const int *h, int *status, SizePlans &plans,
                              std::vector<ipx_plan *> *plan_of)
{
    std::map<std::pair<int, int>, int> plan_rc;
    plan_of->assign(n, nullptr);
    for (int i = 0; i < n; i++) {
        if (status[i] != IPX_OK) continue;
        const std::pair<int, int> key(w[i], h[i]);
        auto it = plan_rc.find(key);
        if (it == plan_rc.end()) {
            ipx_pool_ops o = *ops;
            o.sw = key.first;
            o.sh = key.second;
            SizePlans::Held hd{nullptr, 0};
            const int prc = ipx_plan_acquire(ctx, &o, &hd.pl, &hd.cached);
            // a size the operators cannot be planned for is that size's verdict; anything else (memory, the device) fails the call
            if (prc != IPX_OK && prc != IPX_ERR_INVALID && prc != IPX_ERR_UNSUPPORTED) return prc;
            if (prc == IPX_OK) plans.held[key] = hd;
            it = plan_rc.emplace(key, prc).first;
        }
        if (it->second != IPX_OK) { status[i] = it->second; continue; }
        (*plan_of)[i] = plans.held[key].pl;
    }
    return IPX_OK;
}
