// warp_stitch_maps_planes.hip -- several fixed cameras sampled through their warp maps into one BEV canvas that is written as normalised
// channel planes for a detector, in one launch (bevwarp_stitch_maps_planes, bevwarp_stitch_maps_nv12_planes):
// bevwarp_warp_nv12_planes' plane stage of bevwarp_stitch_maps' (bevwarp_stitch_maps_nv12's) 8-bit canvas under BORDER_CONSTANT, bit for
// bit, with the canvas never in memory.  It is stitch_maps_nv12_out_kernel's shape (warp_stitch_maps_nv12_out.hip): stitch_maps_body's
// camera loop and blends for 8-bit pixels of 3 channels, unchanged in meaning, every pixel starting as the border pixel and stored
// unconditionally, with plane_store.inc's store where the NV12 store stood.  No float64.
//
// One frame per item, the cameras are kernel arguments and the loop's camera number is wave-uniform, every sampled pixel is an inlier: all
// as warp_stitch_maps.hip describes.  The helpers are restated here rather than moved into a header: that unit's machine code stays what
// it was.
#include "warp_stitch_maps_planes.h"
#include "nv12_sample.h"

namespace bevwarp {
namespace {

// floor(n / d) for 0 <= n < 2^23 and 1 <= d < 2^16 with a quotient of at most 255 (warp_stitch.hip's, which has the argument)
__device__ __forceinline__ int div_byte_mean(int n, int d) {
    int q = (int)((float)n * __builtin_amdgcn_rcpf((float)d));
    const int r = n - q * d;
    q += (r >= d ? 1 : 0) - (r < 0 ? 1 : 0);
    return q;
}

// one source pixel of 3 bytes at a byte offset of the frame: exactly its bytes are read
__device__ __forceinline__ uint32_t load_at(const uint8_t* __restrict__ frame, uint32_t off) {
    const uint8_t* q = frame + off;
    return (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
}

// the two adjacent taps of a row of 3-byte pixels: 6 contiguous bytes, never a byte beyond them (warp_map.hip's load_pair_u8x3)
__device__ __forceinline__ void load_pair(const uint8_t* __restrict__ frame, uint32_t off, uint32_t& p0, uint32_t& p1) {
    uint32_t lo;
    uint16_t hi;
    __builtin_memcpy(&lo, frame + off, 4);
    __builtin_memcpy(&hi, frame + off + 4, 2);
    p0 = lo & 0xffffffu;
    p1 = __builtin_amdgcn_alignbit((uint32_t)hi, lo, 24);  // bytes 3, 4, 5
}

// An inlier of interleaved 3-byte pixels: a frame is below 2 GiB (the source limits), so 32 bits hold the offsets.
template <int INTERP>
__device__ __forceinline__ uint32_t sample_inlier(const uint8_t* __restrict__ frame, uint32_t rs, int sx, int sy, int fx, int fy) {
    const uint32_t o00 = (uint32_t)sy * rs + (uint32_t)sx * 3u;
    if constexpr (INTERP == kNearest) {
        return load_at(frame, o00);
    } else {
        uint32_t p00, p01, p10, p11;
        load_pair(frame, o00, p00, p01);
        load_pair(frame, o00 + rs, p10, p11);
        return blend_u8_packed<3>(p00, p01, p10, p11, (uint32_t)fx, (uint32_t)fy);
    }
}

// convert<RGB> (nv12_sample.h) with the middle channel behind a value barrier: warp_map_nv12.hip's convert_packed, which records why --
// fused into v_ashr_pk_u8_i32, two channels' shift and clamp gave wrong pixels on the MI355X in one instance of that unit.  The barrier
// costs no instruction.
template <int RGB>
__device__ __forceinline__ uint32_t convert_packed(uint32_t Y, const Chroma& c) {
    uint32_t r, g, b;
    convert_channels(Y, c, r, g, b);
    asm("" : "+v"(g));
    return RGB ? (r | (g << 8) | (b << 16)) : (b | (g << 8) | (r << 16));
}

// An inlier of NV12 frames in the order convert<RGB> gives: warp_stitch_maps.hip's sample_inlier_nv12.  A tap at pixel (c, r) reads
// Y[r][c] and the pair (r >> 1, c >> 1).  Bilinear: the two taps of a row are ONE 2-byte window of the Y row, and where a row of pairs holds two of them
// (src_w >= 4: `window`, uniform over the camera) their pairs lie in ONE 4-byte window starting at pair min(sx >> 1, src_w / 2 - 2); a
// source 2 px wide has one pair per row, which both taps share.  No byte outside the first src_w bytes of a plane row is read.
template <int INTERP, int RGB>
__device__ __forceinline__ uint32_t sample_inlier_nv12(const uint8_t* __restrict__ yf, const uint8_t* __restrict__ uvf, uint32_t y_rs, uint32_t uv_rs, int src_w,
                                                       bool window, int sx, int sy, int fx, int fy) {
    const uint32_t yo0 = (uint32_t)sy * y_rs + (uint32_t)sx, uo0 = (uint32_t)(sy >> 1) * uv_rs;
    const int p0 = sx >> 1;
    if constexpr (INTERP == kNearest) {
        const uint32_t q = *reinterpret_cast<const uint16_t*>(uvf + uo0 + 2u * (uint32_t)p0);
        return convert_packed<RGB>(yf[yo0], chroma_terms(q));
    } else {
        const uint32_t yo1 = yo0 + y_rs, uo1 = (uint32_t)((sy + 1) >> 1) * uv_rs;
        uint16_t w0, w1;
        __builtin_memcpy(&w0, yf + yo0, 2);  // (unaligned)
        __builtin_memcpy(&w1, yf + yo1, 2);
        uint32_t q00, q01, q10, q11;
        if (window) {
            const int p1 = (sx + 1) >> 1, ps = min(p0, (src_w >> 1) - 2);
            const uint32_t s0 = 16u * (uint32_t)(p0 - ps), s1 = 16u * (uint32_t)(p1 - ps);  // (p1 - ps is 0 or 1: p0 passes ps only at sx = src_w - 2)
            uint32_t v0, v1;
            __builtin_memcpy(&v0, uvf + uo0 + 2u * (uint32_t)ps, 4);  // (2-byte aligned)
            __builtin_memcpy(&v1, uvf + uo1 + 2u * (uint32_t)ps, 4);
            q00 = (v0 >> s0) & 0xffffu, q01 = (v0 >> s1) & 0xffffu, q10 = (v1 >> s0) & 0xffffu, q11 = (v1 >> s1) & 0xffffu;
        } else {
            q00 = q01 = *reinterpret_cast<const uint16_t*>(uvf + uo0);  // src_w == 2: sx is 0
            q10 = q11 = *reinterpret_cast<const uint16_t*>(uvf + uo1);
        }
        const uint32_t p00 = convert_packed<RGB>(w0 & 0xffu, chroma_terms(q00)), p01 = convert_packed<RGB>((uint32_t)w0 >> 8, chroma_terms(q01));
        const uint32_t p10 = convert_packed<RGB>(w1 & 0xffu, chroma_terms(q10)), p11 = convert_packed<RGB>((uint32_t)w1 >> 8, chroma_terms(q11));
        return blend_u8_packed<3>(p00, p01, p10, p11, (uint32_t)fx, (uint32_t)fy);
    }
}

// The lane's 4 entries of camera `cam`, map of frame b (a shared map: frame strides of 0), row y, first pixel xs: warp_stitch_maps.hip's
// load_camera_entries.  No entry past the row's end is read (such an entry is the sentinel: it covers nothing).
template <int INTERP>
__device__ __forceinline__ void load_camera_entries(const StitchMapCamera& cam, uint32_t b, int y, int xs, int dst_w, uint32_t (&e)[kBorderPPL], uint32_t (&fr)[kBorderPPL]) {
    constexpr int PPL = kBorderPPL;
    const bool wide = cam.map_vec_ok && xs + PPL <= dst_w;
    const uint8_t* xrow = cam.xy + (int64_t)b * cam.xy_fs + (int64_t)y * cam.xy_rs + (int64_t)xs * 4;
    if (wide) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(xrow);
        e[0] = v.x, e[1] = v.y, e[2] = v.z, e[3] = v.w;
    } else {
#pragma unroll
        for (int j = 0; j < PPL; j++) e[j] = (xs + j < dst_w) ? reinterpret_cast<const uint32_t*>(xrow)[j] : 0x80008000u;
    }
    if constexpr (INTERP == kLinear) {
        const uint8_t* frow = cam.frac + (int64_t)b * cam.frac_fs + (int64_t)y * cam.frac_rs + (int64_t)xs * 2;
        if (wide) {
            const u32x2 v = *reinterpret_cast<const u32x2*>(frow);
            fr[0] = v.x & 0xffffu, fr[1] = v.x >> 16, fr[2] = v.y & 0xffffu, fr[3] = v.y >> 16;
        } else {
#pragma unroll
            for (int j = 0; j < PPL; j++) fr[j] = (xs + j < dst_w) ? (uint32_t)reinterpret_cast<const uint16_t*>(frow)[j] : 0u;
        }
    }
}

// NV12: the cameras' frames are NV12, converted to B, G, R (RGB = 0) or R, G, B (1); otherwise plane k is the frames' channel k (RGB is 0).
template <int INTERP, int BLEND, bool NV12, int RGB, bool WIDE16>
__global__ __launch_bounds__(kWG) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd, 8))) void stitch_maps_planes_kernel(const StitchMapsPlanesArgs a) {
    constexpr int PPL = kBorderPPL;
    constexpr bool kFeather = BLEND == kStitchFeather;
    uint32_t b;
    int y, xs;  // frame, row, the lane's first pixel
    if (!lane_position(a, b, y, xs)) return;

    // per pixel, as in stitch_maps_body: OVER keeps the pixel and whether it is still undecided; FEATHER the weighted sums and the sum of
    // weights.  A pixel starts as the border pixel: what no camera covers stays that.
    uint32_t px[PPL];
    bool wr[PPL], todo[PPL];
    int acc[PPL][3], wsum[PPL];
#pragma unroll
    for (int j = 0; j < PPL; j++) {
        px[j] = a.bv_u8;
        todo[j] = xs + j < a.dst_w;  // pixels past the row's end are neither computed nor stored
        wr[j] = false;
        wsum[j] = 0;
#pragma unroll
        for (int c = 0; c < 3; c++) acc[j][c] = 0;
    }

    // OVER runs from the last camera to the first and stops when the lane's four pixels are decided; FEATHER runs in ascending order
    const int n = a.n_cams;
    for (int i = 0; i < n; i++) {
        if (!kFeather && !(todo[0] || todo[1] || todo[2] || todo[3])) break;
        const StitchMapCamera& cam = a.cams[kFeather ? i : n - 1 - i];
        uint32_t e[PPL], fr[PPL];
        load_camera_entries<INTERP>(cam, b, y, xs, a.dst_w, e, fr);
        const uint8_t* frame = cam.src + (int64_t)b * cam.src_fs;
        const uint8_t* uvf = NV12 ? cam.uv + (int64_t)b * cam.uv_fs : nullptr;
        const uint32_t rs = (uint32_t)cam.src_rs, uv_rs = (uint32_t)cam.uv_rs;  // (below 2^24: the source limits)
        const int sw = cam.src_w, sh = cam.src_h;
        const bool window = sw >= 4;
#pragma unroll
        for (int j = 0; j < PPL; j++) {
            if (!todo[j]) continue;
            const int sx = (int)(short)(e[j] & 0xffffu), sy = (int)e[j] >> 16;
            const int fx = INTERP == kLinear ? (int)(fr[j] & 31u) : 0, fy = INTERP == kLinear ? (int)((fr[j] >> 5) & 31u) : 0;  // (higher bits are ignored)
            // bevwarp_remap's TRANSPARENT inlier test against THIS camera's frame: every tap read below is a source pixel
            const bool in = INTERP == kLinear ? ((unsigned)sx < (unsigned)(sw - 1) && (unsigned)sy < (unsigned)(sh - 1))
                                              : ((unsigned)sx < (unsigned)sw && (unsigned)sy < (unsigned)sh);
            if (!in) continue;
            uint32_t p;
            if constexpr (NV12)
                p = sample_inlier_nv12<INTERP, RGB>(frame, uvf, rs, uv_rs, sw, window, sx, sy, fx, fy);
            else
                p = sample_inlier<INTERP>(frame, rs, sx, sy, fx, fy);
            wr[j] = true;
            if constexpr (!kFeather) {
                px[j] = p;
                todo[j] = false;
            } else {
                // whole source pixels to the nearest frame edge (>= 1 for an inlier), cut off at F
                const int w = min(min(min(sx + 1, sw - sx), min(sy + 1, sh - sy)), a.feather);
                wsum[j] += w;
#pragma unroll
                for (int c = 0; c < 3; c++) acc[j][c] += (int)((p >> (8 * c)) & 0xffu) * w;  // (the sums stay below 2^23)
            }
        }
    }

    if constexpr (kFeather) {
#pragma unroll
        for (int j = 0; j < PPL; j++) {
            if (wr[j]) {
                uint32_t out = 0;
#pragma unroll
                for (int c = 0; c < 3; c++) out |= (uint32_t)div_byte_mean(acc[j][c] + (wsum[j] >> 1), wsum[j]) << (8 * c);
                px[j] = out;
            }
        }
    }

    const uint32_t (&p)[PPL] = px;
#include "plane_store.inc"
}

template <int INTERP, int BLEND, bool NV12, int RGB>
void launch_format(const StitchMapsPlanesArgs& a, dim3 grid, hipStream_t stream) {
    const dim3 block(kWG);
    if (a.plane == kPlaneF32)
        hipLaunchKernelGGL((stitch_maps_planes_kernel<INTERP, BLEND, NV12, RGB, false>), grid, block, 0, stream, a);
    else
        hipLaunchKernelGGL((stitch_maps_planes_kernel<INTERP, BLEND, NV12, RGB, true>), grid, block, 0, stream, a);
}

template <int INTERP, int BLEND>
void launch_source(const StitchMapsPlanesArgs& a, int source, dim3 grid, hipStream_t stream) {
    if (source == 2)
        launch_format<INTERP, BLEND, true, 1>(a, grid, stream);
    else if (source == 1)
        launch_format<INTERP, BLEND, true, 0>(a, grid, stream);
    else
        launch_format<INTERP, BLEND, false, 0>(a, grid, stream);
}

template <int INTERP>
void launch_blend(const StitchMapsPlanesArgs& a, int blend, int source, dim3 grid, hipStream_t stream) {
    if (blend == kStitchFeather)
        launch_source<INTERP, kStitchFeather>(a, source, grid, stream);
    else
        launch_source<INTERP, kStitchOver>(a, source, grid, stream);
}

}  // namespace

hipError_t launch_stitch_maps_planes(const StitchMapsPlanesArgs& a, int nv12_src, int interp, int blend, int rgb_order, int64_t items, hipStream_t stream) {
    (void)hipGetLastError();  // a stale error left by the host framework is not this call's
    const dim3 grid((unsigned)items);
    const int source = nv12_src ? (rgb_order ? 2 : 1) : 0;  // 0 = interleaved frames, 1 = NV12 frames as B, G, R, 2 = NV12 frames as R, G, B
    (interp == kNearest ? launch_blend<kNearest> : launch_blend<kLinear>)(a, blend, source, grid, stream);
    return hipGetLastError();
}

}  // namespace bevwarp
