#!/bin/bash
# tools/build_variant.sh NAME [extra hipcc flags...] -- builds build/libcofhe_hip_NAME.so (tuning variants of the
# product library; bench.py loads one with --lib) with __graft_entry__.build_library.  SRC=<dir> builds from another
# source tree (e.g. an export of an earlier commit: git archive HEAD cofhe_amd/csrc include | tar -x -C /tmp/base_src;
# SRC=/tmp/base_src); a tree from before the C ABI moved to abi.hip is built with that tree's own build().
# Switches of the device headers: -DCOFHE_M12_FULL (qf.hpp: M1 and M2 from the full products only, the arithmetic of before
# the low-half route: tools/build_variant.sh m12_full -DCOFHE_M12_FULL); -DCOFHE_DOT_FULL (a' and b' from the double-width
# dots only), -DCOFHE_C_FULL (c' from the double-width numerator only).  Each part of round 7 back to the code before it:
# -DCOFHE_M12_SINGLE_DIV (qf.hpp: the low-half route of M1 and M2 with one division per quotient instead of the paired one),
# -DCOFHE_DIVEXACT_HIGH (mp.hpp: mp_divexact keeps the high-limb bookkeeping for a one-plane numerator too),
# -DCOFHE_SQR_FULL (mp.hpp: mp_sqr_low multiplies every chunk pair twice, one chunk product per non-zero chunk).
# Round 8 back to the code before it: -DCOFHE_REM_QUOT (mp.hpp: r = y1 m mod a1 through mp_divrem with its quotient instead of
# mp_rem_norm: tools/build_variant.sh rem_quot -DCOFHE_REM_QUOT).
set -e
cd "$(dirname "$0")/.."
name=$1; shift
S=${SRC:-.}
python3 -c 'import sys; import __graft_entry__ as g; g.build_library(sys.argv[1], sys.argv[2], sys.argv[3], sys.argv[4:])' \
  $S/cofhe_amd/csrc build/obj_$name build/libcofhe_hip_$name.so "$@"
echo "built build/libcofhe_hip_$name.so"
