// ipx_align.h -- the one rounding rule of frames, planes and scratch in HBM: sizes go up to the next multiple of 256 bytes.  Plain C++
// with no dependency on the runtime: the runtime (ipx_runtime_internal.h) and the per-image records of a mixed-size JPEG decode
// (ipx_jpeg_mixed_plan.h, which tools/jpeg_mixed_plan_test.cpp builds as a program of its own) both take it from here.
#pragma once

#include <cstddef>

namespace ipx {

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace ipx
