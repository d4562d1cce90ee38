// warp_u8_linear_p16.hip -- the 8-bit bilinear instances of warp_rows_planes16 (warp_rows.h: float16 / bfloat16 channel planes); translation
// units of their own, so that they compile beside the units whose kernels they leave untouched.
#include "warp_rows.h"

namespace bevwarp {

void launch_u8_linear_p16(const WarpArgs& a, int channels, dim3 grid, hipStream_t stream) { launch_channels_planes16<uint8_t, kLinear>(a, channels, grid, stream); }
#ifdef BEVWARP_CLOCK
hipError_t launch_u8_linear_p16_clock(unsigned long long* out4, int reset) { return read_clock_of_this_unit(out4, reset); }
#endif

}  // namespace bevwarp
