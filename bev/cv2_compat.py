from bev_amd.cv2_compat import *  # noqa: F401,F403
from bev_amd.cv2_compat import (COLOR_YUV2BGR_NV12, COLOR_YUV2RGB_NV12, convertMaps, cvtColor, remap,  # noqa: F401
                                BORDER_CONSTANT, BORDER_DEFAULT, BORDER_REFLECT, BORDER_REFLECT101, BORDER_REFLECT_101,
                                BORDER_REPLICATE, BORDER_TRANSPARENT, BORDER_WRAP, INTER_CUBIC, INTER_LINEAR, INTER_NEAREST, WARP_INVERSE_MAP,
                                findHomography, invert, perspectiveTransform, resize, warpPerspective)
