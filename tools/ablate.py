#!/usr/bin/env python3
"""Ablation builds of the warp kernel (measurement aid; the product source carries no ablation code).

    python tools/ablate.py <name>=<spec>[+<spec>...] ...   ->  bev_amd/csrc/variants/<name>.so

Each spec patches a COPY of the kernel sources (bev_amd/csrc: warp_rows.h, rows_*.inc, coords.h, sample.h -- whichever file holds the
snippet).  Values stay live through `asm volatile` so that nothing upstream is dead code (guide, methodology rule 17).  The specs
(generated from the table below; tests/test_ablate_specs.py applies every one of them to the committed sources):
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bev_amd", "csrc")
FLAGS = "-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -Wno-unused-function -Wno-undefined-internal".split()


KERNEL_FILES = ("coords.h", "sample.h", "warp_rows.h", "rows_body.inc", "rows_coords.inc", "rows_sample.inc", "rows_store.inc", "rows_tiles.inc", "rows_run.inc", "warp_kernels.h")
UNITS = ("warp_kernels", "warp_u8_linear", "warp_u8_nearest", "warp_f32_linear", "warp_f32_nearest", "warp_composite",
         "warp_u8_linear_p16", "warp_u8_nearest_p16", "warp_f32_linear_p16", "warp_f32_nearest_p16")

# snippets of the product source that several specs replace
TAP_LOOP = "#pragma unroll\n        for (int j = 0; j < PPL; j++) {\n            const uint32_t off = S0[j];\n"  # head of issue_s' loop over a lane's pixels
WINDOW_LOADS = "                const uint32_t offa = off & ~3u;\n                __builtin_memcpy(&t0[j], b0 + offa, %s);\n                __builtin_memcpy(&t1[j], b1 + offa, %s);\n"
TILE_OUT = "    if (tile_out) {  // every pixel of the tile is the border value"
SLANT_RULE = "        if (!tile_affine) tile_slanted = fmaxf(edge_slant(0, 1), edge_slant(2, 3)) >"
WIDE_STORE = "    *p = v;\n}"
PAIR_RULE = "__ballot(stp >= 0.0 && stp <= 1.9375)"
WAVES_PER_SIMD = "constexpr int kWavesPerSimd = %d;"
WAVES_PER_EU = "amdgpu_waves_per_eu(%s)"
TAP_SETS = "constexpr int kAhead = INTERP == kNearest ? kFull : %d;"
WG_THREADS = "constexpr int kWG = %d;"


def coalesced_u8(both_rows):
    return (TAP_LOOP,
            "        if (f && kAligned) {\n"
            "            const uint32_t start = (uint32_t)__builtin_amdgcn_readfirstlane((int)S0[0]) & ~15u;\n"
            "            typedef uint32_t q4 __attribute__((ext_vector_type(4)));\n"
            "            q4 r0 = *reinterpret_cast<const q4*>(b0 + start + lane * 16), r1 = {0, 0, 0, 0}, r2 = {0, 0, 0, 0}, r3 = {0, 0, 0, 0};\n"
            "            if (lane < 32) r1 = *reinterpret_cast<const q4*>(b0 + start + 1024 + lane * 16);\n"
            "            if (" + both_rows + ") { r2 = *reinterpret_cast<const q4*>(b1 + start + lane * 16); if (lane < 32) r3 = *reinterpret_cast<const q4*>(b1 + start + 1024 + lane * 16); }\n"
            "            for (int j = 0; j < PPL; j++)\n"
            "                for (int k = 0; k < WINB / 4; k++) t0[j].w[k] = S0[j] * (k + 3) + r0[k] + r1[(k + j) & 3] + r2[k], t1[j].w[k] = S0[j] ^ (0x9e3779b9u * (k + 1)) ^ r0[3] ^ r3[j & 3];\n"
            "            return;\n        }\n" + TAP_LOOP)


def coalesced_f32(both_rows):
    return (TAP_LOOP,
            "        if (f && sizeof(T) == 4 && C == 3 && INTERP == kLinear) {\n"
            "            const uint32_t start = (uint32_t)__builtin_amdgcn_readfirstlane((int)S0[0]) & ~15u;\n"
            "            typedef uint32_t q4 __attribute__((ext_vector_type(4)));\n"
            "            q4 r[6];\n"
            "            for (int i = 0; i < 6; i++) r[i] = q4{0, 0, 0, 0};\n"
            "            r[0] = *reinterpret_cast<const q4*>(b0 + start + lane * 16);\n"
            "            r[1] = *reinterpret_cast<const q4*>(b0 + start + 1024 + lane * 16);\n"
            "            if (lane < 48) r[2] = *reinterpret_cast<const q4*>(b0 + start + 2048 + lane * 16);\n"
            "            if (" + both_rows + ") { r[3] = *reinterpret_cast<const q4*>(b1 + start + lane * 16); r[4] = *reinterpret_cast<const q4*>(b1 + start + 1024 + lane * 16); if (lane < 48) r[5] = *reinterpret_cast<const q4*>(b1 + start + 2048 + lane * 16); }\n"
            "            for (int j = 0; j < PPL; j++)\n"
            "                for (int k = 0; k < LOADB / 4; k++) t0[j].w[k] = r[k % 3][k & 3] ^ r[(k + j) % 3][(k + 1) & 3], t1[j].w[k] = r[3 + k % 3][k & 3] ^ r[0][(k + j) & 3];\n"
            "            return;\n        }\n" + TAP_LOOP)


def store_policy(pol):  # as inline assembly
    return (WIDE_STORE,
            "    if constexpr (__builtin_vectorelements(V) == 4)\n        asm volatile(\"global_store_dwordx4 %%0, %%1, off %s\" ::\"v\"(p), \"v\"(v) : \"memory\");\n"
            "    else if constexpr (__builtin_vectorelements(V) == 3)  // (a 3-element vector is padded to 16 bytes: count elements, not bytes)\n"
            "        asm volatile(\"global_store_dwordx3 %%0, %%1, off %s\" ::\"v\"(p), \"v\"(v) : \"memory\");\n    else\n        *p = v;\n}" % (pol, pol))


# (spec, what it does, [(snippet of the product source, its replacement), ...])
_TABLE = [
    ("nostore", "store_s keeps its operands alive and returns", [
        ("    auto store_s = [&](auto own, int xs, int y, const uint4 (&out)[NQ]) __attribute__((always_inline)) {  // xs = first pixel of the segment / block\n",
         "    auto store_s = [&](auto own, int xs, int y, const uint4 (&out)[NQ]) __attribute__((always_inline)) {\n"
         "        asm volatile(\"\" ::\"v\"(out[0].x), \"v\"(out[0].y), \"v\"(out[0].z), \"v\"(out[0].w));\n        if (y != 12345678) return;\n")]),
    ("noload", "issue_s fabricates taps from the offsets (no vector memory loads)", [
        (TAP_LOOP,
         "        for (int j = 0; j < PPL; j++)\n            for (int k = 0; k < WINB / 4; k++) t0[j].w[k] = S0[j] * (k + 3) + (uint32_t)(uintptr_t)b0, "
         "t1[j].w[k] = S0[j] ^ (0x9e3779b9u * (k + 1));\n        if (cls != 12345678) return;\n" + TAP_LOOP)]),
    ("noblend", "finish_s xors the taps instead of blending", [
        ("            blend_put(j, w0, w1, fx, fy);\n",
         "            wtr[64 * j + lane] = (w0[0] ^ w1[0] ^ w0[NEED - 1] ^ w1[NEED - 1]) + fx + fy;\n")]),
    ("stsmall", "stores go to a few KB per frame (no HBM write traffic)", [
        ("            uint8_t* d = dframe + (int64_t)(y + st_row) * a.dst_rs + (int64_t)st_x * C;\n",
         "            uint8_t* d = dframe + (int64_t)((y + st_row) & 7) * a.dst_rs + (int64_t)(st_x & 255) * C;\n")]),
    ("ldsmall", "taps come from the first 64 KB of the frame (cache hits)", [
        ("            const uint32_t off = S0[j];\n", "            const uint32_t off = S0[j] & 0xffffu;\n")]),
    ("ldx2", "timing only (wrong pixels): the aligned 12-byte tap windows fetched as 8 bytes: the texture path's cost per returned byte", [
        (WINDOW_LOADS % ("WINB", "WINB"), WINDOW_LOADS % (8, 8))]),
    ("ldx1", "timing only (wrong pixels): the same windows fetched as 4 bytes", [
        (WINDOW_LOADS % ("WINB", "WINB"), WINDOW_LOADS % (4, 4))]),
    ("cohload", "timing only: the 8 window gathers of a pass replaced by coalesced 16-byte loads of the source row span the pass starts at "
                "(1.5 KB of ONE row: what a wave that keeps the other tap row staged would fetch)", [coalesced_u8("0")]),
    ("cohload2", "cohload over both tap rows", [coalesced_u8("1")]),
    ("cohf32", "timing only, float RGB: the 16 tap gathers of a pass replaced by coalesced loads of 2.75 KB of ONE source row", [coalesced_f32("0")]),
    ("cohf32b", "cohf32 over both tap rows", [coalesced_f32("1")]),
    ("notie", "no tie-window test in the coordinate chain", [
        ("            tie = min(tie, min(lx[j] & F::kTieMask, ly[j] & F::kTieMask));\n", ""),
        ("            for (int j = 0; j < PPL; j++) tie = min(tie, min(S1[j] & F::kTieMask, S2[j] & F::kTieMask));\n", "            for (int j = 0; j < PPL; j++) tie |= S1[j] >> 31;\n")]),
    ("ntload", "float taps through non-temporal loads (streaming probe: nt loads + nt stores is the box's best mix)", [
        ("                __builtin_memcpy(&t0[j], b0 + off, LOADB);\n                if (INTERP == kLinear) __builtin_memcpy(&t1[j], b1 + off, LOADB);\n",
         "                for (int k = 0; k < LOADB / 4; k++) {\n"
         "                    t0[j].w[k] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(b0 + off) + k);\n"
         "                    if (INTERP == kLinear) t1[j].w[k] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(b1 + off) + k);\n"
         "                }\n")]),
    ("noedge", "EDGE passes cost what OUT passes cost (upper bound of what a cheaper guarded path can gain)", [
        ("            else if (cls == kEdge)\n                edge_s(S1, S2);\n", "            else if (cls == kEdge)\n                fill_s();\n")]),
    ("ownrow", "every tile forced to the unturned lane layout (row segments; edge tiles: blocks) whatever the slant: the slant rule's A/B", [
        (SLANT_RULE, "        if (false) tile_slanted = fmaxf(edge_slant(0, 1), edge_slant(2, 3)) >")]),
    ("ownblk", "every tile forced to the turned lane layout (patches) whatever the slant", [
        (SLANT_RULE, "        if (true) tile_slanted = true || fmaxf(edge_slant(0, 1), edge_slant(2, 3)) >")]),
    ("fillall", "every tile costs what an outside tile costs: the launch + prologue + store floor", [(TILE_OUT, "    if (true) {")]),
    ("edgefill", "tiles the frame's edge crosses cost what outside tiles cost", [(TILE_OUT, "    if (tile_out || !tile_in) {")]),
    ("infill", "interior tiles cost what outside tiles cost", [(TILE_OUT, "    if (tile_out || tile_in) {")]),
    ("nostagger", "dispatch order: every XCD starts at the first item of its run", [
        ("    uint32_t in_run = seq + (blockIdx.x & 7u) * (uint32_t)a.stagger;", "    uint32_t in_run = seq;")]),
    ("revrows", "dispatch order: a frame's tile rows from the bottom up", [
        ("    const uint32_t ty = fast_div(t, a.tx_magic, (uint32_t)a.tiles_x), tx = t - ty * (uint32_t)a.tiles_x;",
         "    const uint32_t ty_ = fast_div(t, a.tx_magic, (uint32_t)a.tiles_x), tx = t - ty_ * (uint32_t)a.tiles_x, ty = (uint32_t)(a.tiles_per_frame / a.tiles_x) - 1u - ty_;")]),
    ("lpt", "dispatch order: an XCD walks its frames tile row by tile row (row r of all its frames, then row r + 1 ...): the run ends with every frame's last rows", [
        ("    const uint32_t frame_idx = fast_div(item, a.tpf_magic, (uint32_t)a.tiles_per_frame);\n    const uint32_t t = item - frame_idx * (uint32_t)a.tiles_per_frame;\n",
         "    uint32_t frame_idx = fast_div(item, a.tpf_magic, (uint32_t)a.tiles_per_frame);\n    uint32_t t = item - frame_idx * (uint32_t)a.tiles_per_frame;\n"
         "    if ((uint32_t)a.chunk % (uint32_t)a.tiles_per_frame == 0u) {\n"
         "        const uint32_t fpx = (uint32_t)a.chunk / (uint32_t)a.tiles_per_frame, per_row = fpx * (uint32_t)a.tiles_x;\n"
         "        const uint32_t r = in_run / per_row, rem = in_run - r * per_row, f = rem / (uint32_t)a.tiles_x;\n"
         "        frame_idx = (blockIdx.x & 7u) * fpx + f;\n        t = r * (uint32_t)a.tiles_x + (rem - f * (uint32_t)a.tiles_x);\n    }\n")]),
    ("nosplit", "no half-height workgroups at the end of an XCD's run (the extra workgroups of the grid leave at once)", [
        ("    if (seq >= (uint32_t)(a.chunk - a.tail_split)) {", "    if (seq >= (uint32_t)a.chunk) return;\n    if (false) {")]),
    ("waves3", "three waves per SIMD (<= 168 VGPRs): room for a third tap set", [
        (WAVES_PER_SIMD % 4, WAVES_PER_SIMD % 3),
        (WAVES_PER_EU % "NSRC > 1 ? 3 : kWavesPerSimd, 8", WAVES_PER_EU % "3, 3")]),  # (max = 3 too: otherwise the allocator still aims at four waves)
    ("waves5", "every warp kernel compiled for five waves per SIMD (<= 96 VGPRs)", [(WAVES_PER_SIMD % 4, WAVES_PER_SIMD % 5)]),
    ("w4x", "exactly four waves per SIMD whatever the register count (with noclass, whose kernels shrink)", [
        (WAVES_PER_EU % "NSRC > 1 ? 3 : kWavesPerSimd, 8", WAVES_PER_EU % "4, 4")]),
    ("ahead1", "bilinear straight-line tiles with ONE tap set in flight", [(TAP_SETS % 2, TAP_SETS % 1)]),
    ("ahead3", "bilinear straight-line tiles with three tap sets in flight", [(TAP_SETS % 2, TAP_SETS % 3)]),
    ("ahead4", "bilinear straight-line tiles with four tap sets in flight", [(TAP_SETS % 2, TAP_SETS % 4)]),
    ("ntstore", "the wide destination stores non-temporal (rounds 2-3 measured them slower on every format)", [
        (WIDE_STORE, "    __builtin_nontemporal_store(v, p);\n}")]),
    ("stsc1", "the wide destination stores carry the sc1 cache policy (write-through)", [store_policy("sc1")]),
    ("stsc01", "the wide destination stores carry the sc0 sc1 cache policy", [store_policy("sc0 sc1")]),
    ("nopair", "no tile takes the pair loads (rows_tiles.inc: tile_pair)", [(PAIR_RULE, "__ballot(false)")]),
    ("allpair", "every row-affine interior tile takes them (timing / diagnosis only: wrong beyond 2 source pixels per pixel)", [(PAIR_RULE, "__ballot(true)")]),
    ("noclass", "timing only, all-interior row-affine footprints (abx --homography inset): no tile classification -- every tile is taken for an interior pair tile", [
        ("    // -- the passes of this wave over the tile, in order.\n",
         "    tile_in = true, tile_out = false, tile_slanted = false, tile_affine = true, tile_pair = true;\n    // -- the passes of this wave over the tile, in order.\n")]),
    ("wg1", "workgroups of one wave instead of four (the host sizes tiles by rows_per_pass(): 6 rows of 8-bit pixels, 4 of float): "
            "a finished wave's slot is refilled without waiting for three others", [(WG_THREADS % 256, WG_THREADS % 64)]),
    ("wg2", "workgroups of two waves (12 rows of 8-bit pixels, 8 of float)", [(WG_THREADS % 256, WG_THREADS % 128)]),
]
SPECS = {name: reps for name, _, reps in _TABLE}
__doc__ += "".join("    %-10s%s\n" % (name, what) for name, what, _ in _TABLE)


def patch(files, spec):
    """files: {name: text} of the kernel sources; each snippet of the spec is replaced (once) in the one file that holds it."""
    if spec not in SPECS:
        raise SystemExit("unknown spec " + spec)
    for old, new in SPECS[spec]:
        hits = [n for n, t in files.items() if old in t]
        assert len(hits) == 1, (spec, old[:60], hits)
        files[hits[0]] = files[hits[0]].replace(old, new, 1)
    return files


def main():
    # --clock: the diagnostic build (-DBEVWARP_CLOCK: per-workgroup stamps, tools/clock.py) of the patched sources; needs
    # `make -C bev_amd/csrc variants/clock.so` first (its bevwarp_api / geom_kernels objects are linked in)
    clock = "--clock" in sys.argv
    if clock:
        sys.argv.remove("--clock")
    base = {n: open(os.path.join(CSRC, n)).read() for n in KERNEL_FILES}
    os.makedirs(os.path.join(CSRC, "variants"), exist_ok=True)
    procs = []
    for arg in sys.argv[1:]:
        name, specs = arg.split("=", 1)
        files = dict(base)
        for spec in [s for s in specs.split("+") if s]:
            files = patch(files, spec)
        tmp = "/tmp/ablate_%s" % name
        os.makedirs(tmp, exist_ok=True)
        for n, t in files.items():
            open(os.path.join(tmp, n), "w").write(t)
        for u in UNITS:  # the translation units themselves are never patched; they include the patched headers from tmp
            open(os.path.join(tmp, u + ".hip"), "w").write(open(os.path.join(CSRC, u + ".hip")).read())
            cmd = ["/opt/rocm/bin/hipcc"] + FLAGS + (["-DBEVWARP_CLOCK"] if clock else []) + ["-I" + os.path.join(ROOT, "include"), "-I" + tmp, "-c", os.path.join(tmp, u + ".hip"), "-o", os.path.join(tmp, u + ".o")]
            procs.append((name, subprocess.Popen(cmd, stderr=subprocess.PIPE)))
    for name, p in procs:
        err = p.communicate()[1].decode()
        if p.returncode:
            raise SystemExit("%s: %s" % (name, err[-2000:]))
    for arg in sys.argv[1:]:
        name = arg.split("=", 1)[0]
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-shared", "-fPIC", "--offload-arch=gfx950", "-o", os.path.join(CSRC, "variants", name + ".so"),
                               os.path.join(CSRC, "variants/clock_bevwarp_api.o" if clock else "bevwarp_api.o"),
                               os.path.join(CSRC, "variants/clock_geom_kernels.o" if clock else "geom_kernels.o")] + ["/tmp/ablate_%s/%s.o" % (name, u) for u in UNITS])
        print("built", name)


if __name__ == "__main__":
    main()
