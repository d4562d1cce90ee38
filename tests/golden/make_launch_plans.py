#!/usr/bin/env python3
"""Writes tests/golden/launch_plans.json: the launch geometry (bev_amd/csrc/host_plan.h) of a few hundred calls.

    python tests/golden/make_launch_plans.py                    plans of the current host_plan.h, through tests/host_plan_driver.cpp:
                                                                for a pull request that changes a planning rule ON PURPOSE (it commits the
                                                                rule and the regenerated fixture together, and says so)
    python tests/golden/make_launch_plans.py --recorder LIB.so  plans a library prints itself: LIB.so is libbevwarp.so with a throw-away
                                                                patch that writes `PLAN {json}` to stderr just before every launch call.
                                                                The committed fixture was first recorded this way from commit 73baee2, the
                                                                last one that planned inside bevwarp_api.hip.

No GPU is needed: without a device the library sizes its launches for 256 CUs, the MI355X's own count, and the recorded calls pass
placeholder pointers that nothing dereferences (the launch itself then fails with a HIP error, after the plan was printed)."""
import ctypes
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "launch_plans.json")
U8, F32, NEAREST, LINEAR = 0, 1, 0, 1
FORMATS = [(U8, LINEAR), (U8, NEAREST), (F32, LINEAR), (F32, NEAREST)]
BIG = 1 << 20


def cases():
    """rows: [batch, src_h, src_w, dst_h, dst_w, channels, dtype, interp]; composite: [bg_h, bg_w, fg_h, fg_w, dst_h, dst_w, channels];
    border: [batch, src_h, src_w, dst_h, dst_w, channels, dtype, interp, mode]"""
    rows = []
    # smoke() and BASELINE.json configs[0]; the "small" branch; configs[1] (bench.py's headline and variants); configs[3]'s shard; configs[4]
    rows += [[1, 720, 1280, 512, 512, 3, d, i] for d, i in FORMATS] + [[1, 240, 426, 512, 512, 3, U8, LINEAR], [32, 480, 852, 1024, 1024, 3, U8, LINEAR]]
    rows += [[32, 1080, 1920, 1024, 1024, 3, d, i] for d, i in FORMATS] + [[32, 2160, 3840, 2048, 2048, 3, d, LINEAR] for d in (U8, F32)]
    rows += [[b, 1080, 1920, 1024, 1024, 3, U8, LINEAR] for b in (1, 4, 8, 16, 256)]
    dsts = [(8, 8), (1, 1), (300, 1), (77, 300), (64, 600), (512, 512), (1024, 1024), (1080, 1920), (2048, 2048), (4096, 4096), (BIG, 8), (8, BIG)]  # (dst_h, dst_w)
    for batch in (1, 2, 4, 12, 32, 64):
        for dtype, interp in FORMATS:
            for k, (dh, dw) in enumerate(dsts):
                rows.append([batch, 720, 1280, dh, dw, 1 + (k + batch) % 4, dtype, interp])
    # ERR_TOO_LARGE: from the item count (8 * chunk >= 2^31) and from a destination side above 2^20
    rows += [[2147483647, 8, 8, 64, 600, 3, U8, LINEAR], [2147483647, 8, 8, 16, 128, 1, F32, NEAREST], [1 << 30, 8, 8, 16, 512, 4, U8, NEAREST], [1 << 24, 8, 8, 4096, 4096, 1, F32, LINEAR]]
    rows += [[1, 8, 8, 8, BIG + 1, 1, U8, LINEAR], [2, 8, 8, BIG + 1, 8, 3, F32, LINEAR], [12, 8, 8, BIG + 1, BIG + 1, 1, U8, NEAREST], [1, 8, 8, 8, 2147483647, 1, U8, LINEAR]]
    out = [{"kind": "rows", "args": r} for r in rows]
    for dh, dw in [(8, 8), (1, 1), (77, 300), (512, 512), (600, 64), (1024, 1024), (1080, 1920), (2048, 2048), (4096, 4096), (BIG, 8), (8, BIG)]:
        for ch in (1, 3, 4):
            out.append({"kind": "composite", "args": [1080, 1920, 720, 1280, dh, dw, ch]})
    k = 0
    for batch in (1, 2, 12, 32):
        for dh, dw in [(8, 8), (300, 1), (77, 300), (512, 512), (1080, 1920), (4096, 4096), (BIG, 8), (8, BIG)]:
            for sh, sw in [(720, 1280), (1, 1), (32767, 5)]:
                dtype, interp = FORMATS[k % 4]
                out.append({"kind": "border", "args": [batch, sh, sw, dh, dw, 1 + k % 4, dtype, interp, 1 + k % 5]})
                k += 1
    out += [{"kind": "border", "args": a} for a in ([2147483647, 8, 8, 64, 600, 3, U8, LINEAR, 2], [1, 8, 8, 8, BIG + 1, 1, U8, LINEAR, 3], [3, 8, 8, BIG + 1, 8, 2, F32, NEAREST, 4])]
    return out


def call_library(lib, case):
    """The call of one case on placeholder pointers (tightly packed frames, the destination behind the source): its status."""
    a, one = case["args"], 16
    if case["kind"] == "composite":
        bh, bw, fh, fw, dh, dw, ch = a
        p, ptrs = 1 << 16, []
        for nbytes in (bh * bw * ch, fh * fw * ch, fh * fw * ch, dh * dw * ch):
            ptrs.append(p)
            p = (p + nbytes + 4095) // 4096 * 4096
        return lib.bevwarp_warp_composite(ptrs[0], bh, bw, bw * ch, ptrs[1], ptrs[2], fh, fw, fw * ch, fw * ch, ptrs[3], dh, dw, dw * ch, ch, one, one, 0, None)
    batch, sh, sw, dh, dw, ch, dtype, interp = a[:8]
    pix = ch * (1 if dtype == U8 else 4)
    src = 1 << 16
    dst = (src + batch * sh * sw * pix + 4095) // 4096 * 4096
    common = (src, dst, batch, sh, sw, dh, dw, ch, sh * sw * pix, sw * pix, dh * dw * pix, dw * pix, one, 1, dtype, interp)
    if case["kind"] == "border":
        return lib.bevwarp_warp_border(*common, a[8], None, None)
    return lib.bevwarp_warp(*common, None, None)


def record(lib_path):
    os.environ["BEVWARP_LIB"] = lib_path
    from bev_amd import _lib
    assert _lib.LIB_PATH == lib_path
    lib, out = _lib.load(), []
    for case in cases():
        with tempfile.TemporaryFile() as f:  # what the patched library writes to stderr during this one call
            sys.stderr.flush()
            saved = os.dup(2)
            os.dup2(f.fileno(), 2)
            try:
                st = call_library(lib, case)
            finally:
                ctypes.CDLL(None).fflush(None)
                os.dup2(saved, 2)
                os.close(saved)
            f.seek(0)
            plans = [json.loads(ln[5:]) for ln in f.read().decode().splitlines() if ln.startswith("PLAN ")]
        assert len(plans) == (1 if st in (0, -5) else 0), (case, st, plans)  # (-5: the launch itself, on a machine without a GPU)
        if plans:
            assert plans[0].pop("kind") == case["kind"]
            for flag in ("dst_vec_ok", "src_vec_ok"):  # (of the placeholder pointers, not of the plan)
                plans[0].pop(flag, None)
            out.append(dict(case, status=0, plan=plans[0]))
        else:
            out.append(dict(case, status=st, plan=None))
    return out


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--recorder":
        recorded = record(os.path.abspath(sys.argv[2]))
    else:
        from tests import hostplan, test_host_plan as t
        recorded = t.plans_from_driver(hostplan.build_driver(), cases())
    with open(OUT, "w") as f:
        f.write('{"cases": [\n' + ",\n".join(json.dumps(c) for c in recorded) + "\n]}\n")
    print("%d cases -> %s" % (len(recorded), OUT))


if __name__ == "__main__":
    main()
