// ipx_jpeg_mixed_plan.h -- the per-image geometry records of a mixed-size JPEG decode (ipx_jpeg_decode_mixed, ipx_jpeg_dec_runtime.hip):
// the images of one sampling class, of any sizes, are decoded by one set of launches; what the uniform kernels take as launch arguments
// (w, h, mxx, myy, nblk, the strides, img * nblk) a mixed kernel reads from its image's record.  Plain C++ with no dependency on the
// runtime, shared by the kernels, the driver and tools/jpeg_mixed_plan_test.cpp, which holds the builder and the search to their rules
// as a program of its own.  DESIGN.md section 4.6.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "ipx_align.h"

#if defined(__HIPCC__)
#define IPX_MIX_HD __host__ __device__
#else
#define IPX_MIX_HD
#endif

namespace ipx {

// one image of a class, in HBM beside its JpegDecTables
struct JpegMixGeom {
    unsigned long long blk0;         // its first block in the class's coefficient and DC arrays (replaces img * nblk)
    unsigned long long yoff, coff;   // its planes within the class's Y block, and within each of the Cb and Cr blocks
    int32_t w, h, mxx, myy, nblk;
    int32_t ystride, cstride;        // image.NewYCbCr's: 8 * h0 * mxx and 8 * mxx
    uint32_t wg0;                    // its first workgroup in the class's one-dimensional IDCT launch
    int32_t wgs_per_row, rsv;
};
static_assert(sizeof(JpegMixGeom) == 64, "read as scalars, one record per image");

// a sampling class: one (h0, v0, components), which is one (bpm, ybl) pair -- the two stay launch arguments, so a class is one launch set
struct JpegMixClass {
    int h0, v0, gray;
    IPX_MIX_HD int ybl() const { return gray ? 1 : h0 * v0; }
    IPX_MIX_HD int bpm() const { return gray ? 1 : h0 * v0 + 2; }
    // MCUs of one MCU row that an IDCT workgroup takes (launch_jpeg_idct's rule)
    IPX_MIX_HD int mcus_per_wg() const { return bpm() == 1 ? 32 : bpm() == 10 ? 4 : 8; }
    bool operator==(const JpegMixClass &o) const { return h0 == o.h0 && v0 == o.v0 && gray == o.gray; }
};

struct JpegMixTotals {
    unsigned long long blocks = 0;      // of all images: the coefficient array holds blocks * 64 values, the DC array blocks
    unsigned long long wgs = 0;         // workgroups of the IDCT launch
    unsigned long long ybytes = 0, cbytes = 0;   // the Y block; each of the two chroma blocks (0 for Gray)
    int max_nblk = 0;
};

// The records of n images of class c, in the order given.  Every prefix sum is kept in 64 bits; false when the class cannot be one
// launch set: a negative size, or more IDCT workgroups than a grid's x dimension holds (2^31 - 1).
inline bool jpeg_mix_build(const JpegMixClass &c, const int *w, const int *h, int n, std::vector<JpegMixGeom> *out, JpegMixTotals *tot)
{
    out->assign((size_t)(n > 0 ? n : 0), JpegMixGeom{});
    *tot = JpegMixTotals{};
    const int per_wg = c.mcus_per_wg();
    for (int i = 0; i < n; i++) {
        if (w[i] <= 0 || h[i] <= 0) return false;
        JpegMixGeom &g = (*out)[(size_t)i];
        g.w = w[i]; g.h = h[i];
        g.mxx = (w[i] + 8 * c.h0 - 1) / (8 * c.h0); g.myy = (h[i] + 8 * c.v0 - 1) / (8 * c.v0);
        const unsigned long long nblk = (unsigned long long)g.mxx * (unsigned long long)g.myy * (unsigned long long)c.bpm();
        if (nblk > 0x7fffffffull) return false;
        g.nblk = (int32_t)nblk;
        g.ystride = 8 * c.h0 * g.mxx; g.cstride = 8 * g.mxx;
        g.wgs_per_row = (g.mxx + per_wg - 1) / per_wg;
        if (tot->wgs > 0xffffffffull) return false;
        g.blk0 = tot->blocks; g.yoff = tot->ybytes; g.coff = tot->cbytes; g.wg0 = (uint32_t)tot->wgs;
        tot->blocks += nblk;
        tot->wgs += (unsigned long long)g.wgs_per_row * (unsigned long long)g.myy;
        tot->ybytes += align256((size_t)g.ystride * 8 * c.v0 * g.myy);
        if (!c.gray) tot->cbytes += align256((size_t)g.cstride * 8 * g.myy);
        if (g.nblk > tot->max_nblk) tot->max_nblk = g.nblk;
    }
    return tot->wgs <= 0x7fffffffull;
}

// The image that owns workgroup wg of the IDCT launch: the last one whose first workgroup is not behind it (every image has at least
// one workgroup, so first workgroups are strictly increasing).  The kernel calls this with a value every lane shares: the probes are
// scalar loads.  wg must be below the launch's total.
IPX_MIX_HD inline int jpeg_mix_find(const JpegMixGeom *g, int n, uint32_t wg)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (g[mid].wg0 <= wg) lo = mid; else hi = mid - 1;
    }
    return lo;
}

}  // namespace ipx
