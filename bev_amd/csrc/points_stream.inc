// points_stream.inc -- the body of a lens point kernel `template <typename T, int DIR> (const T* in, T* out, T* residual, int64_t n,
// const PointsLensArgs a, int vec16)`, included by points_lens.hip and points_fisheye.hip: the stream of points_stream.h.
// BEVWARP_POINT: the unit's arithmetic on one point, `template <int DIR> void (a, px, py, ox, oy, e)`; e: the reprojection error
// (UNDISTORT; untouched by DISTORT).
// (`out` may be `in`: every lane reads its own points before it writes them, and no pointer is __restrict__.  residual is NULL under
// DISTORT, and may be under UNDISTORT.)
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool res = DIR == BEVWARP_LENS_UNDISTORT && residual != nullptr;
    if constexpr (sizeof(T) == 4) {
        if (!vec16) {  // buffers that are only 8-byte aligned (a view starting at an odd point), or a residual that is only 4-byte aligned
            for (int64_t i = t0; i < n; i += stride) {
                const float2 p = reinterpret_cast<const float2*>(in)[i];
                double ox, oy, e = 0.0;
                BEVWARP_POINT<DIR>(a, (double)p.x, (double)p.y, ox, oy, e);
                reinterpret_cast<float2*>(out)[i] = make_float2((float)ox, (float)oy);
                if (res) residual[i] = (float)e;
            }
            return;
        }
        const int64_t pairs = n >> 1;
        for (int64_t i = t0; i < pairs; i += stride) {
            const plf32x4 p = __builtin_nontemporal_load(reinterpret_cast<const plf32x4*>(in) + i);
            double ax, ay, bx, by, ea = 0.0, eb = 0.0;
            BEVWARP_POINT<DIR>(a, (double)p.x, (double)p.y, ax, ay, ea);
            BEVWARP_POINT<DIR>(a, (double)p.z, (double)p.w, bx, by, eb);
            const plf32x4 o = {(float)ax, (float)ay, (float)bx, (float)by};
            reinterpret_cast<plf32x4*>(out)[i] = o;
            if (res) reinterpret_cast<float2*>(residual)[i] = make_float2((float)ea, (float)eb);
        }
        if ((n & 1) && t0 == 0) {  // the odd last point
            double ox, oy, e = 0.0;
            BEVWARP_POINT<DIR>(a, (double)in[2 * (n - 1)], (double)in[2 * (n - 1) + 1], ox, oy, e);
            out[2 * (n - 1)] = (float)ox;
            out[2 * (n - 1) + 1] = (float)oy;
            if (res) residual[n - 1] = (float)e;
        }
    } else {
        for (int64_t i = t0; i < n; i += stride) {
            const plf64x2 p = __builtin_nontemporal_load(reinterpret_cast<const plf64x2*>(in) + i);
            double ox, oy, e = 0.0;
            BEVWARP_POINT<DIR>(a, p.x, p.y, ox, oy, e);
            const plf64x2 o = {ox, oy};
            reinterpret_cast<plf64x2*>(out)[i] = o;
            if (res) residual[i] = e;
        }
    }
