// warp_stitch_gain_nv12_out.hip -- the gained instances of the stitch through warp maps into NV12 (bevwarp_stitch_maps_to_nv12 and
// bevwarp_stitch_maps_nv12_to_nv12 under BEVWARP_STITCH_GAIN): warp_stitch_maps_nv12_out.hip's text over Gained<>
// arguments, every tap put through its camera's gain before the interpolation.  A unit of its own: the plain unit's kernels and machine
// code stay what they were (profiles/stitch_gain_identity.txt).
#define BEVWARP_STITCH_GAIN_UNIT
#include "warp_stitch_maps_nv12_out.hip"
