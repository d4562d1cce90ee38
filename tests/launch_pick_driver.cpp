// Runs the pickers of bev_amd/csrc/launch_pick.h on the CPU for tests/test_launch_pick_cpu.py (g++, address and undefined-behaviour
// sanitizers; no HIP: the header's launcher is left out of a plain C++ build).
//   stdin:  one line "picker word" per case; pickers: 0 value<0, 1> (interp), 1 value<1, 2, 3, 4, 5> (the border units' modes),
//           2 value<0, 1, 2, 3, 4> (the plane units' modes), 3 value<1, 0> (blend), 4 value<2, 1, 0> (source), 5 value<7> (a one-value
//           list), 6 channels, 7 flag, 8 pixel
//   stdout: "calls picked" per case -- how often the callable ran and with what (the sum over the calls); pixel: 0 = uint8_t, 1 = float,
//           -1 = anything else
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "launch_pick.h"

using namespace bevwarp;

int main() {
    int picker, word;
    while (scanf("%d %d", &picker, &word) == 2) {
        int calls = 0;
        long picked = 0;
        auto record = [&](auto v) {
            static_assert(std::is_same_v<typename decltype(v)::value_type, int> || std::is_same_v<typename decltype(v)::value_type, bool>, "a constant");
            constexpr int kValue = v();  // (usable as a template argument: what the units do with it)
            calls++, picked += kValue;
        };
        switch (picker) {
            case 0: pick::value<0, 1>(word, record); break;
            case 1: pick::value<1, 2, 3, 4, 5>(word, record); break;
            case 2: pick::value<0, 1, 2, 3, 4>(word, record); break;
            case 3: pick::value<1, 0>(word, record); break;
            case 4: pick::value<2, 1, 0>(word, record); break;
            case 5: pick::value<7>(word, record); break;
            case 6: pick::channels(word, record); break;
            case 7: pick::flag(word, record); break;
            case 8:
                pick::pixel(word, [&](auto t) {
                    using T = typename decltype(t)::type;
                    calls++, picked += std::is_same_v<T, uint8_t> ? 0 : std::is_same_v<T, float> ? 1 : -1;
                });
                break;
            default: return 2;
        }
        printf("%d %ld\n", calls, picked);
    }
    return 0;
}
