// launch_pick.h -- how a kernel unit turns its runtime words (dtype, channels, interp, border mode, blend, channel order, plane format) into
// one template instance and launches it: each word goes through a picker, which calls a generic lambda with the value as a type, and the
// innermost lambda names the kernel.  The pickers are plain C++17 (tests/launch_pick_driver.cpp compiles them with no HIP); the launcher of
// a flat grid below them is HIP's.  See DESIGN.md section 4.9.
#pragma once
#include <cstdint>
#include <type_traits>

namespace bevwarp {
namespace pick {

// f(std::integral_constant<int, V>{}) for the listed V that v equals.  A value that is not listed takes the LAST listed alternative (the
// host checks admit listed values only); every unit's list order relies on it: interp ends in bilinear, border modes in TRANSPARENT --
// REFLECT_101 where a unit has no transparent instance --, blend in OVER.
template <int V, int... Rest, class F>
void value(int v, F&& f) {
    if constexpr (sizeof...(Rest) == 0)
        f(std::integral_constant<int, V>{});
    else if (v == V)
        f(std::integral_constant<int, V>{});
    else
        value<Rest...>(v, f);
}

// f(std::true_type{}) for any non-zero word, f(std::false_type{}) for zero
template <class F>
void flag(bool on, F&& f) {
    if (on)
        f(std::true_type{});
    else
        f(std::false_type{});
}

// the pixel type: f(pixel_type<uint8_t>{}) for dtype 0, f(pixel_type<float>{}) for anything else; the lambda reads it as
// `typename decltype(t)::type`
template <class T>
struct pixel_type {
    using type = T;
};
template <class F>
void pixel(int dtype, F&& f) {
    if (dtype == 0)
        f(pixel_type<uint8_t>{});
    else
        f(pixel_type<float>{});
}

template <class F>
void channels(int n, F&& f) {
    value<1, 2, 3, 4>(n, f);
}

}  // namespace pick
}  // namespace bevwarp

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

namespace bevwarp {

// One launch of a flat grid -- `items` workgroups of `block` lanes, no shared memory, one argument struct.  choose(launch) picks the
// instance and calls launch(kernel) once.  A stale error left by the host framework is cleared first: it is not this call's.
template <class Args, class Choose>
hipError_t launch_items(const Args& args, int64_t items, int block, hipStream_t stream, Choose&& choose) {
    (void)hipGetLastError();
    const dim3 grid((unsigned)items), lanes((unsigned)block);
    choose([&](void (*kernel)(Args)) { hipLaunchKernelGGL(kernel, grid, lanes, 0, stream, args); });
    return hipGetLastError();
}

}  // namespace bevwarp
#endif
