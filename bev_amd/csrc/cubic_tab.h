// cubic_tab.h -- the tables of the bicubic warp (BEVWARP_CUBIC), as plain C++17 for host and device: the 1-D coefficients, the
// float and the fixed-point 4 x 4 entry of a sub-pixel position (fy, fx), and the index remap's period for a tap window.
// OpenCV 3.x-4.x's interpolateCubic / initInterTab2D, restated from memory: parity with an installed cv2 is unpinned, like the
// rest of the warp.  Every function is constexpr, so that warp_cubic.hip emits its tables by constant evaluation, and
// tests/cubic_tab_driver.cpp compiles this file with g++ under the sanitizers.  See DESIGN.md section 4.10.  Not installed.
//
// All arithmetic is float32 with no contraction (an FMA would round once where the definition rounds twice): constant
// evaluation never contracts, and a translation unit that calls these at run time must be compiled with -ffp-contract=off.
#pragma once
#include <stdint.h>

#include "host_plan.h"

#if defined(__HIP__) || defined(__CUDACC__)
#define BEVWARP_HD __host__ __device__
#else
#define BEVWARP_HD
#endif

namespace bevwarp {
namespace cubic {

constexpr int kTabBits = 5, kTabSize = 1 << kTabBits;  // sub-pixel positions per axis (INTER_BITS of the maps)
constexpr int kTaps = 4;                               // per axis; the window starts one pixel before the map's integer position
constexpr int kOne = 32768;                            // fixed-point 1 (INTER_REMAP_COEF_SCALE)

struct Coeffs {
    float c[kTaps];
};
struct EntryF {
    float w[kTaps * kTaps];
};
struct EntryI {
    int16_t w[kTaps * kTaps];
};

// The coefficients of position i / 32, A = -0.75.
BEVWARP_HD constexpr Coeffs coeffs(int i) {
    const float A = -0.75f;
    const float x = (float)i * (1.f / 32);
    const float x1 = x + 1, xm = 1 - x;
    Coeffs r = {};
    r.c[0] = ((A * x1 - 5 * A) * x1 + 8 * A) * x1 - 4 * A;
    r.c[1] = ((A + 2) * x - (A + 3)) * x * x + 1;
    r.c[2] = ((A + 2) * xm - (A + 3)) * xm * xm + 1;
    r.c[3] = 1.f - r.c[0] - r.c[1] - r.c[2];
    return r;
}

// wf[k1 * 4 + k2] = cy[k1] * cx[k2]: k1 is the row.
BEVWARP_HD constexpr EntryF entry_f32(const Coeffs& cy, const Coeffs& cx) {
    EntryF e = {};
    for (int k1 = 0; k1 < kTaps; k1++)
        for (int k2 = 0; k2 < kTaps; k2++) e.w[k1 * kTaps + k2] = cy.c[k1] * cx.c[k2];
    return e;
}
BEVWARP_HD constexpr EntryF entry_f32(int fy, int fx) { return entry_f32(coeffs(fy), coeffs(fx)); }

// saturate_cast<short>(v): round half to even, clamp (|v| <= 2^24 here, so v - trunc(v) is exact)
BEVWARP_HD constexpr int round_sat16(float v) {
    int t = (int)v;
    const float r = v - (float)t;
    if (r > 0.5f || (r == 0.5f && (t & 1))) t++;
    if (r < -0.5f || (r == -0.5f && (t & 1))) t--;
    return t < -32768 ? -32768 : (t > 32767 ? 32767 : t);
}

// The fixed-point entry: every weight rounded on its own, then the sum brought to kOne at ONE tap of the lower right 2 x 2
// (k1, k2 in ksize / 2 .. ksize / 2 + 1, as OpenCV scans them -- not the central 2 x 2): a deficit goes to the largest of the
// four, a surplus comes off the smallest.
BEVWARP_HD constexpr EntryI entry_i16(int fy, int fx) {
    const EntryF f = entry_f32(fy, fx);
    int w[kTaps * kTaps] = {};
    int sum = 0;
    for (int k = 0; k < kTaps * kTaps; k++) {
        w[k] = round_sat16(f.w[k] * (float)kOne);
        sum += w[k];
    }
    if (sum != kOne) {
        const int diff = sum - kOne;
        int lo = (kTaps / 2) * kTaps + kTaps / 2, hi = lo;
        for (int k1 = kTaps / 2; k1 < kTaps / 2 + 2; k1++)
            for (int k2 = kTaps / 2; k2 < kTaps / 2 + 2; k2++) {
                const int k = k1 * kTaps + k2;
                if (w[k] < w[lo])
                    lo = k;
                else if (w[k] > w[hi])
                    hi = k;
            }
        if (diff < 0)
            w[hi] -= diff;
        else
            w[lo] -= diff;
    }
    EntryI e = {};
    for (int k = 0; k < kTaps * kTaps; k++) e.w[k] = (int16_t)w[k];
    return e;
}

// The tables as the kernel reads them: coefficients by position, and fixed-point entries in the order fy, fx, k1, k2.
struct CoeffTable {
    float c[kTabSize][kTaps];
};
struct FixedTable {
    int16_t w[kTabSize * kTabSize][kTaps * kTaps];
};
constexpr CoeffTable make_coeff_table() {
    CoeffTable t = {};
    for (int i = 0; i < kTabSize; i++) {
        const Coeffs c = coeffs(i);
        for (int k = 0; k < kTaps; k++) t.c[i][k] = c.c[k];
    }
    return t;
}
constexpr FixedTable make_fixed_table() {
    FixedTable t = {};
    for (int fy = 0; fy < kTabSize; fy++)
        for (int fx = 0; fx < kTabSize; fx++) {
            const EntryI e = entry_i16(fy, fx);
            for (int k = 0; k < kTaps * kTaps; k++) t.w[fy * kTabSize + fx][k] = e.w[k];
        }
    return t;
}

// The index remap of a window of taps, for an axis of n source pixels: plan::border_period's fields for indices in
// [-reach, reach].  The maps saturate to int16 BEFORE the window is laid out, so a window of `before` taps ahead of the
// map's position and `after` behind it reaches 32768 + before down and 32767 + after up: 32769 for these 4 taps (an 8-tap
// window would pass 32771).  border_period itself stays as the bilinear kernel's plans pin it.
constexpr int kReach = 32767 + kTaps / 2;
inline plan::BorderPeriod window_period(int mode, int n, int reach = kReach) {
    plan::BorderPeriod b = plan::border_period(mode, n);  // (the period alone is taken from it)
    b.off = ((uint32_t)reach + b.per - 1u) / b.per * b.per;
    b.mag = plan::div_magic((uint64_t)b.off + (uint32_t)reach + 1u, b.per);
    return b;
}

// cv::borderInterpolate(p, n, mode) in closed form for |p| <= reach, b = window_period(mode, n, reach): the border kernel's
// border_index (REPLICATE clamps; WRAP p mod n; REFLECT q = p mod 2n, q < n ? q : 2n - 1 - q; REFLECT_101 q = p mod (2n - 2),
// q < n ? q : 2n - 2 - q, and everything maps to 0 when n == 1), plus CONSTANT: -1 outside.  TRANSPARENT's written
// non-inliers take REFLECT_101's indices.
BEVWARP_HD constexpr int window_index(int mode, int p, int n, uint32_t per, uint32_t off, uint32_t mag) {
    if (mode == BEVWARP_BORDER_CONSTANT) return (unsigned)p < (unsigned)n ? p : -1;
    if (mode == BEVWARP_BORDER_REPLICATE) return p < 0 ? 0 : (p > n - 1 ? n - 1 : p);
    const uint32_t u = (uint32_t)(p + (int)off);
    const uint32_t d = mag ? (uint32_t)(((uint64_t)u * mag) >> 32) : u / per;  // (coords.h's fast_div)
    const int q = (int)(u - d * per);
    if (mode == BEVWARP_BORDER_WRAP) return q;
    if (mode == BEVWARP_BORDER_REFLECT) return q < n ? q : (int)per - 1 - q;
    return q < n ? q : (int)per - q;  // REFLECT_101 (and TRANSPARENT)
}

}  // namespace cubic
}  // namespace bevwarp
