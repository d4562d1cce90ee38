#!/usr/bin/env python3
"""Writes tests/golden/entry_calls.json: what the Python warp entry points (bev_amd/warp.py, bev_amd/resize.py) hand to the C ABI for a
few hundred calls, and what they raise for a few hundred more (tests/entry_calls.py holds the cases and says how arguments are written
down).  Needs a GPU -- the entry points insist on CUDA tensors and a current stream -- but launches no kernel of the library: the
loaded library is replaced by a stub that records.

    python tests/golden/make_entry_calls.py

The committed fixture was recorded from the last commit whose entry points spelt every step out by hand (45b9a43).  It pins
behaviour: a pull request regenerates it only where it changes what an entry point passes or raises ON PURPOSE, and says so."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "entry_calls.json")


def main():
    from tests import entry_calls
    recorded = entry_calls.record_all()
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    with open(out, "w") as f:
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in recorded.items()) + "\n}\n")
    print("%d cases, %d calls -> %s" % (len(recorded), sum(len(v) for v in recorded.values()), out))


if __name__ == "__main__":
    main()
