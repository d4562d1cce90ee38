// launch_record_driver.hip -- calls every public launcher of the flat-grid kernel units (and launch_warp, whose channel ladder is
// warp_rows.h's) with every combination of its runtime words and prints one line per call: launcher, tuple, return value, launches, and
// what launch_record_runtime.cpp wrote down of the launch -- the kernel's mangled name, grid, block, shared memory, stream, and a hash of
// the argument bytes.  tools/launch_record.py builds and runs it; it opens no device and dereferences no argument.
//
// Every word takes its admitted values and one below and one above them.  The fields of the argument struct that a launcher reads are
// words too: WarpArgs::planar and src_rs, the plane format of the plane units.  Everything else in the struct is zero but `dst`, which
// carries the call's number, so that the hash tells one call's arguments from another's.
#include <stdio.h>
#include <string.h>

#include <initializer_list>
#include <vector>

#include "warp_cubic.h"
#include "warp_kernels.h"
#include "warp_lens.h"
#include "warp_map.h"
#include "warp_map_nv12.h"
#include "warp_map_nv12_out.h"
#include "warp_map_planes.h"
#include "warp_nv12.h"
#include "warp_nv12_out.h"
#include "warp_stitch.h"
#include "warp_stitch_maps.h"
#include "warp_stitch_maps_nv12_out.h"
#include "warp_stitch_maps_planes.h"

extern "C" void launch_record_begin(size_t arg_bytes);
extern "C" int launch_record_end(const char** line);

using namespace bevwarp;

namespace {

struct Word {
    const char* name;
    int lo, hi;  // the admitted values
    int pad;     // 1: lo - 1 and hi + 1 are tried as well
};

int g_calls;

// call(a, v, items, stream) for every combination v of the words, the argument struct zeroed before each
template <class Args, class Call>
void sweep(const char* launcher, std::initializer_list<Word> list, Call call) {
    const std::vector<Word> words(list);
    std::vector<int> v;
    for (const Word& w : words) v.push_back(w.lo - w.pad);
    for (;;) {
        Args a;
        memset(&a, 0, sizeof(a));
        g_calls++;
        a.dst = reinterpret_cast<uint8_t*>(static_cast<uintptr_t>(g_calls) << 8);
        launch_record_begin(sizeof(Args));
        const hipError_t e = call(a, v.data(), (int64_t)(1000 + g_calls), reinterpret_cast<hipStream_t>(static_cast<uintptr_t>(0x5000 + g_calls % 7)));
        const char* line;
        const int launches = launch_record_end(&line);
        printf("%s", launcher);
        for (size_t k = 0; k < words.size(); k++) printf(" %s=%d", words[k].name, v[k]);
        printf(" -> returns %d, %d launch: %s\n", (int)e, launches, line);
        size_t k = words.size();
        while (k > 0 && v[k - 1] == words[k - 1].hi + words[k - 1].pad) k--, v[k] = words[k].lo - words[k].pad;
        if (k == 0) break;
        v[k - 1]++;
    }
}

const Word kDtype = {"dtype", 0, 1, 1}, kChannels = {"channels", 1, 4, 1}, kInterp = {"interp", kNearest, kLinear, 1};
const Word kBorder = {"mode", kBorderReplicate, kBorderTransparent, 1}, kBorderAll = {"mode", 0, kBorderTransparent, 1};
const Word kBorderWritten = {"mode", 0, kBorderReflect101, 1};  // the plane and NV12 stores write every pixel: no transparent instance
const Word kBlend = {"blend", kStitchOver, kStitchFeather, 1}, kBool = {"flag", 0, 1, 0}, kOrder = {"rgb_order", 0, 1, 1}, kNv12Src = {"nv12_src", 0, 1, 1};
const Word kPlane = {"plane", kPlaneF32, kPlaneBF16, 1}, kPlanar = {"planar", 0, kPlaneBF16, 1}, kRowStride = {"src_rs", 12, 13, 0};

}  // namespace

int main() {
    sweep<WarpArgs>("launch_warp", {kDtype, kChannels, kInterp, kPlanar, kRowStride}, [](WarpArgs& a, const int* v, int64_t items, hipStream_t s) {
        a.planar = v[3], a.src_rs = v[4];
        a.chunk = (int)items, a.tail_split = 3;  // (its grid is its own: 8 * (chunk + tail_split))
        return launch_warp(a, v[0], v[1], v[2], s);
    });
    sweep<BorderArgs>("launch_warp_border", {kDtype, kChannels, kInterp, kBorder},
                      [](BorderArgs& a, const int* v, int64_t items, hipStream_t s) { return launch_warp_border(a, v[0], v[1], v[2], v[3], items, s); });
    sweep<CubicArgs>("launch_warp_cubic", {kDtype, kChannels, kBorderAll},
                     [](CubicArgs& a, const int* v, int64_t items, hipStream_t s) { return launch_warp_cubic(a, v[0], v[1], v[2], items, s); });
    sweep<LensArgs>("launch_warp_lens", {kDtype, kChannels, kInterp, kBool},
                    [](LensArgs& a, const int* v, int64_t items, hipStream_t s) { return launch_warp_lens(a, v[0], v[1], v[2], v[3] != 0, items, s); });
    sweep<LensArgs>("launch_warp_fisheye", {kDtype, kChannels, kInterp, kBool},
                    [](LensArgs& a, const int* v, int64_t items, hipStream_t s) { return launch_warp_fisheye(a, v[0], v[1], v[2], v[3] != 0, items, s); });
    sweep<Nv12Args>("launch_warp_nv12", {kInterp, kOrder},
                    [](Nv12Args& a, const int* v, int64_t items, hipStream_t s) { return launch_warp_nv12(a, v[0], v[1], items, s); });
    sweep<Nv12PlanesArgs>("launch_warp_nv12_planes", {kInterp, kPlane}, [](Nv12PlanesArgs& a, const int* v, int64_t items, hipStream_t s) {
        a.plane = v[1];
        return launch_warp_nv12_planes(a, v[0], items, s);
    });
    sweep<Nv12OutArgs>("launch_warp_nv12_out", {kNv12Src, kInterp, kOrder},
                       [](Nv12OutArgs& a, const int* v, int64_t items, hipStream_t s) { return launch_warp_nv12_out(a, v[0], v[1], v[2], items, s); });
    sweep<StitchArgs>("launch_warp_stitch", {kDtype, kChannels, kInterp, kBlend},
                      [](StitchArgs& a, const int* v, int64_t items, hipStream_t s) { return launch_warp_stitch(a, v[0], v[1], v[2], v[3], items, s); });

    sweep<MapBuildArgs>("launch_build_map", {kInterp, kBool},
                        [](MapBuildArgs& a, const int* v, int64_t items, hipStream_t s) { return launch_build_map(a, v[0], v[1] != 0, items, s); });
    sweep<MapBuildArgs>("launch_build_map_fisheye", {kInterp},
                        [](MapBuildArgs& a, const int* v, int64_t items, hipStream_t s) { return launch_build_map_fisheye(a, v[0], items, s); });
    sweep<RemapArgs>("launch_remap", {kDtype, kChannels, kInterp, kBorderAll},
                     [](RemapArgs& a, const int* v, int64_t items, hipStream_t s) { return launch_remap(a, v[0], v[1], v[2], v[3], items, s); });
    sweep<RemapArgs>("launch_remap_cubic", {kDtype, kChannels, kBorderAll},
                     [](RemapArgs& a, const int* v, int64_t items, hipStream_t s) { return launch_remap_cubic(a, v[0], v[1], v[2], items, s); });
    sweep<RemapNv12Args>("launch_remap_nv12", {kInterp, kBorderAll, kOrder},
                         [](RemapNv12Args& a, const int* v, int64_t items, hipStream_t s) { return launch_remap_nv12(a, v[0], v[1], v[2], items, s); });
    sweep<RemapNv12PlanesArgs>("launch_remap_nv12_planes", {kInterp, kBorderWritten, kPlane}, [](RemapNv12PlanesArgs& a, const int* v, int64_t items, hipStream_t s) {
        a.plane = v[2];
        return launch_remap_nv12_planes(a, v[0], v[1], items, s);
    });
    sweep<RemapNv12OutArgs>("launch_remap_nv12_out", {kNv12Src, kInterp, kBorderWritten, kOrder}, [](RemapNv12OutArgs& a, const int* v, int64_t items, hipStream_t s) {
        return launch_remap_nv12_out(a, v[0], v[1], v[2], v[3], items, s);
    });
    sweep<RemapPlanesArgs>("launch_remap_planes", {kInterp, kBorderWritten, kPlane}, [](RemapPlanesArgs& a, const int* v, int64_t items, hipStream_t s) {
        a.plane = v[2];
        return launch_remap_planes(a, v[0], v[1], items, s);
    });

    sweep<StitchMapsArgs>("launch_stitch_maps", {kDtype, kChannels, kInterp, kBlend},
                          [](StitchMapsArgs& a, const int* v, int64_t items, hipStream_t s) { return launch_stitch_maps(a, v[0], v[1], v[2], v[3], items, s); });
    sweep<StitchMapsArgs>("launch_stitch_maps_nv12", {kInterp, kBlend, kOrder},
                          [](StitchMapsArgs& a, const int* v, int64_t items, hipStream_t s) { return launch_stitch_maps_nv12(a, v[0], v[1], v[2], items, s); });
    sweep<Gained<StitchMapsArgs>>("launch_stitch_gain", {kDtype, kChannels, kInterp, kBlend}, [](Gained<StitchMapsArgs>& a, const int* v, int64_t items, hipStream_t s) {
        return launch_stitch_gain(a, v[0], v[1], v[2], v[3], items, s);
    });
    sweep<Gained<StitchMapsArgs>>("launch_stitch_gain_nv12", {kInterp, kBlend, kOrder}, [](Gained<StitchMapsArgs>& a, const int* v, int64_t items, hipStream_t s) {
        return launch_stitch_gain_nv12(a, v[0], v[1], v[2], items, s);
    });
    sweep<StitchMapsNv12OutArgs>("launch_stitch_maps_nv12_out", {kNv12Src, kInterp, kBlend, kOrder}, [](StitchMapsNv12OutArgs& a, const int* v, int64_t items, hipStream_t s) {
        return launch_stitch_maps_nv12_out(a, v[0], v[1], v[2], v[3], items, s);
    });
    sweep<Gained<StitchMapsNv12OutArgs>>("launch_stitch_gain_nv12_out", {kNv12Src, kInterp, kBlend, kOrder},
                                         [](Gained<StitchMapsNv12OutArgs>& a, const int* v, int64_t items, hipStream_t s) {
                                             return launch_stitch_gain_nv12_out(a, v[0], v[1], v[2], v[3], items, s);
                                         });
    sweep<StitchMapsPlanesArgs>("launch_stitch_maps_planes", {kNv12Src, kInterp, kBlend, kOrder, kPlane}, [](StitchMapsPlanesArgs& a, const int* v, int64_t items, hipStream_t s) {
        a.plane = v[4];
        return launch_stitch_maps_planes(a, v[0], v[1], v[2], v[3], items, s);
    });
    sweep<Gained<StitchMapsPlanesArgs>>("launch_stitch_gain_planes", {kNv12Src, kInterp, kBlend, kOrder, kPlane},
                                        [](Gained<StitchMapsPlanesArgs>& a, const int* v, int64_t items, hipStream_t s) {
                                            a.plane = v[4];
                                            return launch_stitch_gain_planes(a, v[0], v[1], v[2], v[3], items, s);
                                        });
    fprintf(stderr, "%d calls\n", g_calls);
    return 0;
}
