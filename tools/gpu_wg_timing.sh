# phase stamps of one 128x128 launch with build/wg_timing (cross-compiled by tools/build_tools.sh next to the library's objects,
# which do not travel to the GPU box: there is nothing to build it from here)
set -e
cd $GRAFT_REPO_ROOT
OUT=$GRAFT_REPO_ROOT/gpurun_out/wg_timing
mkdir -p $OUT
[ -x build/wg_timing ] || { echo "build/wg_timing is missing: run tools/build_tools.sh where the library was built"; exit 1; }
timeout -k 10 300 python tools/wg_timing.py gen $OUT
timeout -k 10 120 build/wg_timing $OUT/delta.bin $OUT/a.bin $OUT/b.bin > $OUT/wg.csv 2> $OUT/wg_timing.txt
grep -A14 "phase means" $OUT/wg_timing.txt
python tools/wg_timing.py report $OUT/wg.csv | tee $OUT/report.txt
rm -f $OUT/a.bin $OUT/b.bin
