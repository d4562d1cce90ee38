// Runs bev_amd/csrc/cubic_tab.h on the CPU for tests/test_cubic_cpu.py (g++, address and undefined-behaviour sanitizers).
//   cubic_tab_driver TABLES REMAP
// TABLES: the 1024 float entries (16 float32 each, order fy, fx, k1, k2), then the 1024 fixed-point entries (16 int16 each).
// REMAP:  for every mode of 1..4, every n of the list below and every p of [-kReach, kReach]: window_index as int32.
// Both are also evaluated at compile time (static_assert below): what the kernel's tables hold is what is written here.
#include <stdio.h>

#include "cubic_tab.h"

using namespace bevwarp;

static_assert(cubic::entry_i16(0, 0).w[5] == 32767 && cubic::entry_i16(0, 0).w[10] == 1, "constant evaluation of the table");
static_assert(cubic::kReach == 32769, "the 4-tap window's reach");

static const int kN[] = {1, 2, 3, 4, 5, 37, 640, 32767};

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "wb");
    if (!f) return 3;
    for (int fy = 0; fy < cubic::kTabSize; fy++)
        for (int fx = 0; fx < cubic::kTabSize; fx++) {
            const cubic::EntryF e = cubic::entry_f32(fy, fx);
            if (fwrite(e.w, sizeof(float), 16, f) != 16) return 4;
        }
    for (int fy = 0; fy < cubic::kTabSize; fy++)
        for (int fx = 0; fx < cubic::kTabSize; fx++) {
            const cubic::EntryI e = cubic::entry_i16(fy, fx);
            if (fwrite(e.w, sizeof(int16_t), 16, f) != 16) return 4;
        }
    if (fclose(f)) return 4;
    // the tables as warp_cubic.hip emits them (built at run time here: the same functions)
    const cubic::FixedTable t = cubic::make_fixed_table();
    const cubic::CoeffTable c = cubic::make_coeff_table();
    for (int i = 0; i < 1024; i++) {
        const cubic::EntryI e = cubic::entry_i16(i >> 5, i & 31);
        const cubic::EntryF ef = cubic::entry_f32(i >> 5, i & 31);
        for (int k = 0; k < 16; k++)
            if (t.w[i][k] != e.w[k] || c.c[i >> 5][k >> 2] * c.c[i & 31][k & 3] != ef.w[k]) return 5;
    }
    f = fopen(argv[2], "wb");
    if (!f) return 3;
    for (int mode = BEVWARP_BORDER_REPLICATE; mode <= BEVWARP_BORDER_REFLECT_101; mode++)
        for (int n : kN) {
            const plan::BorderPeriod b = cubic::window_period(mode, n);
            for (int p = -cubic::kReach; p <= cubic::kReach; p++) {
                const int32_t q = cubic::window_index(mode, p, n, b.per, b.off, b.mag);
                if (fwrite(&q, sizeof(q), 1, f) != 1) return 4;
            }
        }
    if (fclose(f)) return 4;
    // CONSTANT gives -1 outside and the index inside
    for (int n : kN)
        for (int p = -cubic::kReach; p <= cubic::kReach; p++)
            if (cubic::window_index(BEVWARP_BORDER_CONSTANT, p, n, 1, 0, 0) != ((p >= 0 && p < n) ? p : -1)) return 6;
    return 0;
}
