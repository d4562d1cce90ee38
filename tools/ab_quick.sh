#!/bin/bash
# A/B of any number of builds over the main variants (GPU box): bash tools/ab_quick.sh base=base.so new=new.so [other=other.so ...]
# Every abx.py run has its own time limit; the first one that fails ends the script.
[ $# -ge 2 ] || { echo "usage: $0 name=lib.so name=lib.so ..." >&2; exit 2; }
LIBS=("$@")
for cfg in "u8 linear keystone" "u8 linear brno" "u8 nearest keystone" "f32 linear keystone" "f32 linear brno" "u8 linear rot25z1.4"; do
  set -- $cfg
  echo "== $cfg"
  timeout -k 10 150 python tools/abx.py --rounds 40 --check --dtype $1 --interp $2 --homography $3 --libs "${LIBS[@]}" 2>/dev/null || exit 1
done
