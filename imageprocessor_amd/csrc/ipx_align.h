// ipx_align.h -- the two rounding rules: frames, planes and scratch in HBM go up to the next multiple of 256 bytes (align256); a stream
// in an encoder's block, or a table in a blob, starts on a multiple of 16 (align16).  Plain C++ with no dependency on the runtime: the
// runtime (ipx_runtime_internal.h) and the per-image records of the mixed-size JPEG decode and encode (ipx_jpeg_mixed_plan.h,
// ipx_jpeg_enc_mixed_plan.h, which tools/jpeg_mixed_plan_test.cpp and tools/jpeg_enc_mixed_plan_test.cpp build as programs of their
// own) take them from here.
#pragma once

#include <cstddef>

namespace ipx {

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

}  // namespace ipx
