// points_stream.h -- the memory pattern of the lens point kernels (points_lens.hip: OpenCV's rational model; points_fisheye.hip: the
// equidistant one), which is project_points_kernel's (geom_kernels.hip): 16 bytes per lane and step -- two float32 points or one float64
// point --, non-temporal loads, plain stores, a grid-stride loop, the odd last point, and one point per step for float32 buffers that are
// only 8-byte aligned.  The kernels' body is points_stream.inc; here are its vector types and the launch geometry.  What a unit adds is its
// model's arithmetic on one point, and its kernels.
#pragma once
#include "points_lens.h"

#include "bevwarp.h"

namespace bevwarp {
namespace {

typedef float plf32x4 __attribute__((ext_vector_type(4)));
typedef double plf64x2 __attribute__((ext_vector_type(2)));

// The launch of n > 0 points: vec16 -- two float32 points per lane and step where both buffers are 16-byte aligned (and the residual's
// pairs 8-byte aligned) -- and the grid: 8 workgroups per CU and a grid-stride loop above, for either type: unlike
// project_points_kernel<double> these kernels are bound by their float64 arithmetic, not by the stream.
inline int points_grid(const void* in, const void* out, const void* residual, int64_t n, bool f32, int& vec16) {
    vec16 = f32 && (((uintptr_t)in | (uintptr_t)out) & 15) == 0 && ((uintptr_t)residual & 7) == 0;
    const int64_t lanes = (f32 && vec16) ? (n + 1) / 2 : n;
    const int64_t want = (lanes + kPointsLensBlock - 1) / kPointsLensBlock;
    return (int)(want < kPointsLensMaxBlocks ? want : kPointsLensMaxBlocks);
}

}  // namespace
}  // namespace bevwarp
