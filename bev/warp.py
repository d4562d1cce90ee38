from bev_amd.warp import (BORDER_CONSTANT, BORDER_DEFAULT, BORDER_REFLECT, BORDER_REFLECT101, BORDER_REFLECT_101,  # noqa: F401
                          BORDER_REPLICATE, BORDER_TRANSPARENT, BORDER_WRAP, INTER_CUBIC, INTER_LINEAR, INTER_NEAREST, WARP_INVERSE_MAP, WarpMap, build_warp_map, convert_maps, fisheye_valid_theta, footprint,
                          invert_homography, lens_from_calib, lens_valid_r2, ray_matrix, remap, remap_nv12, remap_nv12_to_nv12, remap_nv12_to_planar, remap_stitch, remap_stitch_nv12, remap_stitch_nv12_to_nv12, remap_stitch_nv12_to_planar, remap_stitch_to_nv12, remap_stitch_to_planar, remap_to_nv12, remap_to_planar, resize_matrix, split_nv12, warp_nv12_to_nv12, warp_nv12_to_planar, warp_perspective,
                          warp_perspective_lens, warp_perspective_nv12, warp_perspective_resized, warp_perspective_to_nv12, warp_stitch, warp_to_planar, warpPerspective)
from bev_amd.resize import cv2_resize, resize  # noqa: F401,E402
