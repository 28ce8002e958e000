// ks_plan_check.cpp -- ks_fused_plan (csrc/ipx_ks_host.cpp) on the CPU: what it picks for a geometry, and whether the plan holds what
// ks_fused_kernel (csrc/ipx_ks_fused.hip) relies on.  Host C++ only; tests/test_ks_plan_host.py builds and runs it:
//   hipcc -x c++ -std=c++17 -ffp-contract=off -D__HIP_PLATFORM_AMD__ csrc/ipx_ks_host.cpp csrc/ipx_host.cpp tools/ks_plan_check.cpp
//
// Shapes come from stdin, one per line:  tag sw sh do_resize w h keep_aspect do_thumbnail size crop_to_fit
// and from a seeded sweep:               ks_plan_check --sweep N SEED
// For each shape the axes are built the way ipx_plan_create builds them and the planner runs for tiles of 4, 8 and 2 bytes per pixel.
// Output, one line per shape and tile size:
//   P tag px nacc strips dbuf fast.dbuf open_per_wave lanes | threads lds fast.lds | out0 ntap waves cpl wcols split | out1 ...
//   N tag px                 the planner declined (per-output kernels take the batch): legal, counted
//   X tag                    ipx_plan_create itself refuses the shape
//   V tag px what            a violated invariant
// then `T px nacc strips(1, 2, 3 = three and more) dbuf fast.dbuf open_per_wave lanes count` per class, and a summary line.
// Every check compares integers or bit patterns; each names what in the kernel it protects.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <tuple>
#include <vector>

#include "../imageprocessor_amd/csrc/ipx_ks.h"

using namespace ipx;

namespace ipx { float ks_float_eps(int nx, int ny); }

namespace {

struct Geo { std::string tag; int sw, sh, do_r, rw, rh, keep, do_t, tsize, crop; };
struct Scale { bool on = false, have = false; int dw = 0, dh = 0; ipx_rect sr{0, 0, 0, 0}; KsAxis hx, hy; };

long long n_viol = 0, n_plan = 0, n_noplan = 0, n_refused = 0, n_shapes = 0, n_nofloat = 0;
std::map<std::tuple<int, int, int, int, int, int, int>, long long> tally;

template <class T> uint64_t bits(T v)
{
    uint64_t b = 0;
    memcpy(&b, &v, sizeof v);
    return b;
}

struct Checker {
    const Geo &g;
    int px;
    const std::vector<uint8_t> &blob;
    int shown = 0;
    void fail(const char *fmt, ...) __attribute__((format(printf, 2, 3)))
    {
        n_viol++;
        if (++shown > 12) return;                      // one broken table repeats itself
        char msg[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(msg, sizeof msg, fmt, ap);
        va_end(ap);
        printf("V %s %d %s\n", g.tag.c_str(), px, msg);
    }
    // a table of `n` T's the plan points at: inside the blob?
    template <class T> const T *table(const void *off, size_t n, const char *what)
    {
        const size_t o = (size_t)(uintptr_t)off;
        if (o > blob.size() || n * sizeof(T) > blob.size() - o) { fail("%s: %zu entries at offset %zu leave the blob of %zu bytes", what, n, o, blob.size()); return nullptr; }
        if (o % 16) fail("%s: offset %zu is not 16-byte aligned", what, o);
        return (const T *)(blob.data() + o);
    }
};

struct Region { long long b, e; const char *what; };
void check_regions(Checker &C, const char *layout, std::vector<Region> r, long long total, long long limit)
{
    for (size_t i = 0; i < r.size(); i++) {
        if (r[i].b < 0 || r[i].e < r[i].b) C.fail("%s LDS: %s is [%lld, %lld)", layout, r[i].what, r[i].b, r[i].e);
        if (r[i].e > total) C.fail("%s LDS: %s ends at %lld, lds_bytes is %lld", layout, r[i].what, r[i].e, total);
        for (size_t j = i + 1; j < r.size(); j++)
            if (r[i].b < r[j].e && r[j].b < r[i].e && r[i].b < r[i].e && r[j].b < r[j].e)
                C.fail("%s LDS: %s [%lld, %lld) overlaps %s [%lld, %lld)", layout, r[i].what, r[i].b, r[i].e, r[j].what, r[j].b, r[j].e);
    }
    if (total > limit) C.fail("%s LDS: %lld bytes, more than %lld", layout, total, limit);
}

// one segmentation's row entries of one output (ks_column / ks_columns_fast walk them group by group; l. 567-569 stage them)
template <int NACC>
void check_rows(Checker &C, const KsFusedGeom &geo, const KsSeg *segs, int k, const Scale &s, const char *gname)
{
    typedef KsRowT<NACC> Row;
    const int B = kKsRows;
    const KsAxis &hy = s.hy;
    const int32_t *rowoff = C.table<int32_t>(geo.rowoff[k], geo.nseg, "rowoff");
    if (!rowoff) return;
    std::vector<int> emitted(s.dh, 0);
    long long expect_off = 0;
    for (int si = 0; si < geo.nseg; si++) {
        const KsSeg &sg = segs[si];
        const int rows = sg.r1 - sg.ys, n = (rows + B - 1) / B * B;
        if (rowoff[si] != expect_off) C.fail("%s out%d: rowoff[%d] = %d, the segments before it hold %lld entries", gname, k, si, rowoff[si], expect_off);
        expect_off += n;
        const Row *e = C.table<Row>((const void *)((uintptr_t)geo.rows[k] + (size_t)rowoff[si] * sizeof(Row)), n, "row entries");
        if (!e) return;
        struct Fed { int y; uint64_t w, wf; };
        std::vector<Fed> fed[NACC];
        for (int i = 0; i < n; i++) {
            const int y = sg.ys + i;
            for (int p = 0; p < NACC; p++) {
                const Row &r = e[i];
                if (i >= rows && (bits(r.w[p]) || r.emit[p] != -1 || bits(r.wf[p])))
                    C.fail("%s out%d seg %d: the padding entry of row %d feeds accumulator %d", gname, k, si, y, p);
                if (bits(r.w[p])) fed[p].push_back(Fed{y, bits(r.w[p]), bits(r.wf[p])});
                else if (bits(r.wf[p])) C.fail("%s out%d seg %d row %d: wf without w in accumulator %d", gname, k, si, y, p);
                const int d = r.emit[p];
                if (d < 0) {
                    if (d != -1) C.fail("%s out%d seg %d row %d: emit %d", gname, k, si, y, d);
                    continue;
                }
                if (d >= s.dh) { C.fail("%s out%d seg %d row %d: emits destination row %d of %d", gname, k, si, y, d, s.dh); fed[p].clear(); continue; }
                emitted[d]++;
                if (d % NACC != p) C.fail("%s out%d: destination row %d emitted from accumulator %d", gname, k, d, p);
                if (y < sg.r0 || y >= sg.r1) C.fail("%s out%d: destination row %d emitted at source row %d outside its segment [%d, %d)", gname, k, d, y, sg.r0, sg.r1);
                // the accumulator held exactly this destination row's (source row, weight) list, in order: nothing of another row
                // was added before this one was emitted, and nothing is missing because the segment began too late
                const int first = s.sr.y0 + hy.lo[d];
                if (first < sg.ys) C.fail("%s out%d: destination row %d starts at source row %d, its segment streams from %d", gname, k, d, first, sg.ys);
                bool same = (int)fed[p].size() == hy.cnt[d];
                for (int t = 0; same && t < hy.cnt[d]; t++) {
                    const double w = hy.w[(size_t)d * hy.ntap + t];
                    same = fed[p][t].y == first + t && fed[p][t].w == bits(w) && fed[p][t].wf == bits((float)(w * hy.itw[d]));
                }
                if (!same) C.fail("%s out%d: accumulator %d at the emit of destination row %d does not hold that row's %d taps from source row %d", gname, k, p, d, hy.cnt[d], first);
                if (bits(r.itw[p]) != bits(hy.itw[d]) || bits(r.ones[p]) != bits(hy.ones[d])) C.fail("%s out%d: itw / ones of destination row %d", gname, k, d);
                fed[p].clear();
            }
        }
        for (int p = 0; p < NACC; p++)
            if (!fed[p].empty()) C.fail("%s out%d seg %d: accumulator %d is fed from source row %d and never emitted", gname, k, si, p, fed[p][0].y);
    }
    for (int d = 0; d < s.dh; d++)
        if (emitted[d] != 1) { C.fail("%s out%d: destination row %d is emitted %d times", gname, k, d, emitted[d]); break; }
}

void check_plan(Checker &C, const Geo &g, const Scale sc[2], int px, int top_taps, const KsFusedPlan &P)
{
    const int B = kKsRows, sw = g.sw, sh = g.sh;
    const size_t row_bytes = P.nacc == 2 ? sizeof(KsRowT<2>) : sizeof(KsRowT<4>);
    if (P.rows != B) C.fail("rows %d", P.rows);
    if (P.nacc != 2 && P.nacc != 4) { C.fail("nacc %d", P.nacc); return; }
    const int ns = P.nstrips;
    if (ns < 1 || ns > 64) { C.fail("nstrips %d", ns); return; }
    const KsStrip *st = C.table<KsStrip>(P.strips, ns, "strips");
    if (!st) return;

    // ---- strips: l. 556-566 (staging: x = t0 + 4 * chunk, 16-byte LDS and watermark stores, owned columns [c0, c1)) ----
    int twmax = 0;
    for (int c = 0; c < ns; c++) {
        const KsStrip &s = st[c];
        if (s.c0 != (c ? st[c - 1].c1 : 0) || s.c1 <= s.c0 || (c == ns - 1 && s.c1 != sw)) C.fail("strip %d owns [%d, %d): no partition of [0, %d)", c, s.c0, s.c1, sw);
        if (s.c0 & 3) C.fail("strip %d: c0 %d is no multiple of 4", c, s.c0);
        if ((s.t0 & 3) || (s.tw & 3) || s.t0 < 0 || s.tw <= 0) C.fail("strip %d: tile [%d, +%d)", c, s.t0, s.tw);
        if (s.t0 > s.c0 || s.t0 + s.tw < s.c1) C.fail("strip %d: tile [%d, +%d) does not hold the owned columns [%d, %d)", c, s.t0, s.tw, s.c0, s.c1);
        twmax = std::max(twmax, s.tw);
    }
    if (P.pitch != twmax * px) C.fail("pitch %d, the widest tile is %d pixels of %d bytes", P.pitch, twmax, px);
    const long long chunks = (long long)B * (P.pitch / (4 * px));
    if (chunks > (long long)kKsMaxStage * P.nthreads) C.fail("%lld chunks per group for %d threads of %d each", chunks, P.nthreads, kKsMaxStage);
    if (P.nstg != (int)((chunks + P.nthreads - 1) / std::max(1, P.nthreads))) C.fail("nstg %d", P.nstg);
    if ((P.nthreads & 63) || P.nthreads < 256 || P.nthreads > kKsMaxThreads) C.fail("nthreads %d", P.nthreads);
    if (2 * B * (int)(row_bytes / 4) > P.nthreads) C.fail("%d threads cannot stage two outputs' row entries (l. 567)", P.nthreads);   // one dword each

    // ---- columns: l. 596-620 ----
    int waves_sum = 0;
    for (int k = 0; k < 2; k++) {
        const KsFusedPlan::Out &o = P.o[k];
        if (!sc[k].have) {
            if (o.wx || o.waves) C.fail("out%d is absent and has tables or waves", k);
            continue;
        }
        const KsAxis &hx = sc[k].hx;
        const int dw = sc[k].dw, x0 = sc[k].sr.x0;
        waves_sum += o.waves;
        if (o.ntap != hx.ntap) C.fail("out%d: ntap %d, the axis has %d", k, o.ntap, hx.ntap);
        if ((o.split != 1 && o.split != 2) || o.ntapf != (hx.ntap + o.split - 1) / o.split * o.split) C.fail("out%d: split %d ntapf %d for %d taps", k, o.split, o.ntapf, hx.ntap);
        if (o.split == 2 && hx.ntap < kKsSplitTaps) C.fail("out%d: two lanes per column at %d taps", k, hx.ntap);
        if (o.cpl > kKsMaxCpl || (o.cpl != 1 && (P.nacc == 4 || o.split == 2)) || (o.wcols > 0 && o.cpl < 1)) C.fail("out%d: cpl %d with nacc %d split %d", k, o.cpl, P.nacc, o.split);
        if ((long long)o.wcols * o.split > 64LL * o.waves * o.cpl) C.fail("out%d: %d columns x %d lanes on %d waves x %d columns per lane", k, o.wcols, o.split, o.waves, o.cpl);
        if (bits(o.feps) != bits(ks_float_eps(hx.ntap, sc[k].hy.ntap))) C.fail("out%d: feps", k);
        // (a lane without a column walks ntap taps from the tile's first pixel with weight 0: l. 617, `has` false)
        if ((long long)o.ntapf * px > P.pitch) C.fail("out%d: %d taps are wider than a tile row of %d bytes", k, o.ntapf, P.pitch);
        const int32_t *colb = C.table<int32_t>(o.colb, ns + 1, "colb");
        const int32_t *xlo = C.table<int32_t>(o.xlo, dw, "xlo");
        const double *itwf = C.table<double>(o.itwf, dw, "itwf");
        const size_t wc = (size_t)std::max(1, o.wcols);
        const double *wx = C.table<double>(o.wx, (size_t)ns * hx.ntap * wc, "wx");
        const float *wxf = C.table<float>(o.wxf, (size_t)ns * o.ntapf * wc, "wxf");
        if (!colb || !xlo || !itwf || !wx || !wxf) continue;
        if (memcmp(xlo, hx.lo.data(), (size_t)dw * 4)) C.fail("out%d: xlo is no copy of the axis", k);
        if (memcmp(itwf, hx.itwffff.data(), (size_t)dw * 8)) C.fail("out%d: itwf is no copy of the axis", k);
        if (colb[0] != 0 || colb[ns] != dw) C.fail("out%d: colb runs from %d to %d, the output has %d columns", k, colb[0], colb[ns], dw);
        bool mono = true;
        for (int c = 0; c < ns; c++) mono = mono && colb[c] <= colb[c + 1];
        if (!mono || colb[0] < 0 || colb[ns] > dw) { C.fail("out%d: colb does not rise", k); continue; }
        const double unit = px == 4 || (px == 8 && k == 1 && top_taps) ? 65535.0 * 257.0 : 65535.0;
        for (int c = 0; c < ns; c++) {
            const int n = colb[c + 1] - colb[c];
            if (n > o.wcols) C.fail("out%d strip %d: %d columns, wcols %d", k, c, n, o.wcols);
            const int t0 = st[c].t0, t1 = st[c].t0 + st[c].tw;
            for (int i = 0; i < n; i++) {
                const int dx = colb[c] + i, first = x0 + xlo[dx];
                // l. 617: the lane reads taps [first, first + ntap) of every tile row; the float pass ntapf of them
                if (first < t0 || first + hx.ntap > t1 || first + o.ntapf > t1)
                    C.fail("out%d strip %d column %d: taps [%d, +%d (float pass %d)) leave the tile [%d, %d)", k, c, dx, first, hx.ntap, o.ntapf, t0, t1);
                // its real taps are pixels of the frame (what lies beyond is never staged: l. 559)
                if (first + hx.cnt[dx] > sw) C.fail("out%d column %d: taps to %d in a frame of %d columns", k, dx, first + hx.cnt[dx], sw);
            }
            for (int t = 0; t < o.ntapf; t++)
                for (int i = 0; i < o.wcols; i++) {
                    const bool real = i < n && t < hx.ntap;
                    if (t < hx.ntap) {
                        const double want = real ? hx.w[(size_t)(colb[c] + i) * hx.ntap + t] : 0.0;
                        if (bits(wx[((size_t)c * hx.ntap + t) * o.wcols + i]) != bits(want)) { C.fail("out%d strip %d: wx[%d][%d]", k, c, t, i); goto next_strip; }
                    }
                    const float wantf = real ? (float)(hx.w[(size_t)(colb[c] + i) * hx.ntap + t] * hx.itwffff[colb[c] + i] * unit) : 0.f;
                    if (bits(wxf[((size_t)c * o.ntapf + t) * o.wcols + i]) != bits(wantf)) { C.fail("out%d strip %d: wxf[%d][%d]", k, c, t, i); goto next_strip; }
                }
        next_strip:;
        }
    }
    if (waves_sum > kKsMaxWaves || 64 * waves_sum > P.nthreads) C.fail("%d waves with roles in %d threads", waves_sum, P.nthreads);

    // ---- LDS: l. 585-618 (weight tables, row entries), l. 669 (lists), l. 686 / 713 (tile and row entries of buffer g & 1) ----
    {
        std::vector<Region> r;
        const long long tile = (long long)B * P.pitch;
        r.push_back(Region{0, (P.dbuf + 1) * tile, "the tile"});
        for (int k = 0; k < 2; k++)
            if (sc[k].have) {
                r.push_back(Region{P.lds_w[k], P.lds_w[k] + (long long)P.o[k].ntap * P.o[k].wcols * 8, k ? "out1's weights" : "out0's weights"});
                if (P.lds_w[k] & 7) C.fail("float64 LDS: weights of out%d at %d", k, P.lds_w[k]);
            }
        r.push_back(Region{P.lds_rows, P.lds_rows + (long long)(P.dbuf + 1) * 2 * B * (long long)row_bytes, "the row entries"});
        if (P.lds_rows & 7) C.fail("float64 LDS: row entries at %d", P.lds_rows);
        if (P.dbuf != 0 && P.dbuf != 1) C.fail("dbuf %d", P.dbuf);
        check_regions(C, "float64", r, P.lds_bytes, 150 << 10);
    }
    if (P.fast.lds_bytes > 0) {
        const KsFusedPlan::Lds &F = P.fast;
        std::vector<Region> r;
        const long long tile = (long long)B * P.pitch;
        r.push_back(Region{0, (F.dbuf + 1) * tile, "the tile"});
        for (int k = 0; k < 2; k++)
            if (sc[k].have) {
                r.push_back(Region{F.lds_w[k], F.lds_w[k] + (long long)P.o[k].ntapf * P.o[k].wcols * 4, k ? "out1's weights" : "out0's weights"});
                if (F.lds_w[k] & 3) C.fail("float LDS: weights of out%d at %d", k, F.lds_w[k]);
            }
        r.push_back(Region{F.lds_rows, F.lds_rows + (long long)(F.dbuf + 1) * 2 * B * (long long)row_bytes, "the row entries"});
        r.push_back(Region{F.lds_open, F.lds_open + (long long)(P.nthreads / 64) * F.open_per_wave * 8, "the lists"});
        if ((F.lds_rows & 7) || (F.lds_open & 7)) C.fail("float LDS: row entries at %d, lists at %d", F.lds_rows, F.lds_open);
        if (F.open_per_wave < 64) C.fail("open_per_wave %d: one ballot may add an entry per lane", F.open_per_wave);
        if (F.dbuf != 0 && F.dbuf != 1) C.fail("fast.dbuf %d", F.dbuf);
        check_regions(C, "float", r, F.lds_bytes, (160 << 10) - 512);
    } else n_nofloat++;

    // ---- segments and rows: l. 623-663 (groups of B rows from ys), l. 702 (rows [r0, r1) are stored to the watermark frame) ----
    for (int gi = 0; gi < 2; gi++) {
        const KsFusedGeom &geo = gi ? P.split : P.whole;
        const char *gname = gi ? "split" : "whole";
        if (geo.nseg < 1 || (!gi && geo.nseg != 1)) { C.fail("%s: %d segments", gname, geo.nseg); continue; }
        const KsSeg *segs = C.table<KsSeg>(geo.segs, geo.nseg, "segs");
        if (!segs) continue;
        bool ok = true;
        for (int i = 0; i < geo.nseg; i++) {
            const KsSeg &s = segs[i];
            if (s.r0 != (i ? segs[i - 1].r1 : 0) || s.r1 <= s.r0 || (i == geo.nseg - 1 && s.r1 != sh) || s.ys > s.r0 || s.ys < 0) {
                C.fail("%s seg %d: ys %d rows [%d, %d) of %d", gname, i, s.ys, s.r0, s.r1, sh);
                ok = false;
            }
        }
        if (!ok) continue;
        for (int k = 0; k < 2; k++) {
            if (!sc[k].have) continue;
            if (P.nacc == 2) check_rows<2>(C, geo, segs, k, sc[k], gname);
            else check_rows<4>(C, geo, segs, k, sc[k], gname);
        }
    }
}

void run_shape(const Geo &g)
{
    n_shapes++;
    Scale sc[2];
    const int sw = g.sw, sh = g.sh;
    bool refused = sw <= 0 || sh <= 0 || !frame_span_ok(sw, sh, (long long)sw * 4, 4);
    if (!refused && g.do_r) {
        int nw, nh;
        if (ipx_resize_dims(sw, sh, g.rw, g.rh, g.keep, &nw, &nh) || !frame_span_ok(nw, nh, (long long)nw * 4, 4)) refused = true;
        else { sc[0].on = true; sc[0].dw = nw; sc[0].dh = nh; sc[0].sr = ipx_rect{0, 0, sw, sh}; }
    }
    if (!refused && g.do_t) {
        int nw, nh;
        ipx_rect crop;
        if (ipx_thumb_geometry(sw, sh, g.tsize, g.crop, &crop, &nw, &nh) || !frame_span_ok(nw, nh, (long long)nw * 4, 4)) refused = true;
        else { sc[1].on = true; sc[1].dw = nw; sc[1].dh = nh; sc[1].sr = crop; }
    }
    for (int k = 0; k < 2 && !refused; k++) {
        Scale &s = sc[k];
        if (!s.on || s.dw <= 0 || s.dh <= 0) continue;
        if (!ks_build_axis(s.dw, s.sr.x1 - s.sr.x0, &s.hx) || !ks_build_axis(s.dh, s.sr.y1 - s.sr.y0, &s.hy)) refused = true;
        s.have = true;
    }
    if (refused) { n_refused++; printf("X %s\n", g.tag.c_str()); return; }
    KsFusedIn fin[2];
    for (int k = 0; k < 2; k++) { fin[k].dw = sc[k].dw; fin[k].dh = sc[k].dh; fin[k].sr_x0 = sc[k].sr.x0; fin[k].sr_y0 = sc[k].sr.y0; fin[k].hx = &sc[k].hx; fin[k].hy = &sc[k].hy; }
    for (int px : {4, 8, 2}) {
        std::vector<uint8_t> blob;
        KsFusedPlan P;
        const int top_taps = px == 8 && g.crop;
        fin[1].top_taps = top_taps;
        if (!ks_fused_plan(sw, sh, sc[0].have ? &fin[0] : nullptr, sc[1].have ? &fin[1] : nullptr, px, &blob, &P)) {
            n_noplan++;
            printf("N %s %d\n", g.tag.c_str(), px);
            continue;
        }
        n_plan++;
        Checker C{g, px, blob};
        if (!P.ok) C.fail("a plan that is not ok");
        check_plan(C, g, sc, px, top_taps, P);
        int lanes = 1;
        for (int k = 0; k < 2; k++) if (sc[k].have) lanes = std::max(lanes, P.o[k].split);
        tally[std::make_tuple(px, P.nacc, std::min(P.nstrips, 3), P.dbuf, P.fast.dbuf, P.fast.open_per_wave, lanes)]++;
        printf("P %s %d %d %d %d %d %d %d | %d %d %d |", g.tag.c_str(), px, P.nacc, P.nstrips, P.dbuf, P.fast.dbuf, P.fast.open_per_wave, lanes, P.nthreads, P.lds_bytes, P.fast.lds_bytes);
        for (int k = 0; k < 2; k++) printf(" out%d %d %d %d %d %d%s", k, P.o[k].ntap, P.o[k].waves, P.o[k].cpl, P.o[k].wcols, P.o[k].split, k ? "\n" : " |");
    }
}

// ---- the sweep: widths to 65532, crop rectangles, one operator or both, up- and downscales ----
void sweep(int n, unsigned seed)
{
    std::mt19937 rng(seed);                              // (the engine's output is fixed by the standard; no distribution object is used)
    auto below = [&](int m) { return (int)(rng() % (uint32_t)m); };
    auto between = [&](int a, int b) { return a + below(b - a + 1); };
    for (int i = 0; i < n; i++) {
        Geo g;
        switch (below(8)) {
        case 0: g.sw = between(1, 640); break;
        case 1: case 2: g.sw = between(640, 4096); break;
        case 3: case 4: g.sw = between(4096, 10000); break;
        case 5: g.sw = between(10000, 30000); break;
        case 6: g.sw = between(30000, 65532); break;
        default: g.sw = 65532 - 4 * below(8); break;
        }
        if (below(4)) g.sw = std::max(4, g.sw & ~3);     // the planar and deep types need a multiple of 4; RGBA frames do not
        // (the tiling follows the width; the rows cost the sweep its time)
        g.sh = below(10) == 0 ? between(600, 4500) : below(3) == 0 ? between(1, 12) : between(12, 600);
        if (g.sw > 20000) g.sh = std::min(g.sh, 300);
        const int ops = below(6);                        // 0: resize only, 1: thumbnail only, else both
        g.do_r = ops != 1; g.do_t = ops != 0;
        // output width from a fortieth of the source to twice it (beyond x4 on an axis the planner declines: counted)
        const int num = between(1, 80);
        g.rw = below(12) == 0 ? between(1, 5 * g.sw > 65535 ? 65535 : 5 * g.sw) : (int)std::min<long long>(65535, std::max<long long>(1, (long long)g.sw * num / 40));
        g.rh = below(3) == 0 ? g.sh : std::max(1, below(2) ? (int)((long long)g.sh * num / 40) : between(1, 2 * g.sh));
        g.keep = below(3) == 0;
        g.tsize = below(5) == 0 ? between(1, 16) : between(16, 400);
        g.crop = below(2);
        char tag[160];
        snprintf(tag, sizeof tag, "sweep:%d,%d,%d,%d,%d,%d,%d,%d,%d", g.sw, g.sh, g.do_r, g.rw, g.rh, g.keep, g.do_t, g.tsize, g.crop);
        g.tag = tag;
        run_shape(g);
    }
}

}  // namespace

int main(int argc, char **argv)
{
    for (const char *knob : {"IPX_KS_STRIPS", "IPX_KS_SPLIT_ROWS", "IPX_KS_TAPSPLIT", "IPX_KS_FAST_DBUF"})
        if (getenv(knob)) { fprintf(stderr, "ks_plan_check: %s is set; this tool checks what the planner picks by itself\n", knob); return 2; }
    int n_sweep = 0;
    unsigned seed = 1;
    bool read_stdin = true;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "--sweep") && i + 2 < argc) { n_sweep = atoi(argv[i + 1]); seed = (unsigned)strtoul(argv[i + 2], nullptr, 10); i += 2; }
        else if (!strcmp(argv[i], "--no-stdin")) read_stdin = false;
        else { fprintf(stderr, "usage: ks_plan_check [--no-stdin] [--sweep N SEED] < shapes\n"); return 2; }
    }
    char line[512], tag[256];
    while (read_stdin && fgets(line, sizeof line, stdin)) {
        Geo g;
        if (line[0] == '#' || line[0] == '\n') continue;
        if (sscanf(line, "%255s %d %d %d %d %d %d %d %d %d", tag, &g.sw, &g.sh, &g.do_r, &g.rw, &g.rh, &g.keep, &g.do_t, &g.tsize, &g.crop) != 10) {
            fprintf(stderr, "ks_plan_check: cannot read `%s`\n", line);
            return 2;
        }
        g.tag = tag;
        run_shape(g);
    }
    sweep(n_sweep, seed);
    for (const auto &t : tally)
        printf("T %d %d %d %d %d %d %d %lld\n", std::get<0>(t.first), std::get<1>(t.first), std::get<2>(t.first), std::get<3>(t.first), std::get<4>(t.first),
               std::get<5>(t.first), std::get<6>(t.first), t.second);
    printf("ks_plan_check: %lld shapes, %lld refused by the plan itself, %lld plans in %zu classes, %lld without a plan, %lld without a float layout, %lld violations\n",
           n_shapes, n_refused, n_plan, tally.size(), n_noplan, n_nofloat, n_viol);
    return n_viol ? 1 : 0;
}
