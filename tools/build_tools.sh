#!/bin/bash
# tools/build_tools.sh -- cross-compiles the GPU-side measurement helpers into build/ (git-ignored, shipped by gpurun):
#   build/wg_timing      diagnostic build of k_compose_wg with phase / clock stamps (tools/wg_timing.hip)
#   build/traffic_calib  record-copy kernel that calibrates FETCH_SIZE / WRITE_SIZE (tools/traffic_calib.hip)
#   build/inst_bench     per-instruction issue costs (tools/inst_bench.hip)
set -e
cd "$(dirname "$0")/.."
mkdir -p build
H=/opt/rocm/bin/hipcc
$H --offload-arch=gfx950 -O3 -std=c++17 -o build/traffic_calib tools/traffic_calib.hip &
$H --offload-arch=gfx950 -O2 -std=c++17 -o build/inst_bench tools/inst_bench.hip &
# wg_timing.hip compiles the kernels of cofhe_hip.hip itself (with the stamps) and takes every other translation unit of the
# library from the objects of the last build (python __graft_entry__.py): abi.hip refers to the kernels of all of them
OBJ=${OBJ:-cofhe_amd/csrc/obj}
($H --offload-arch=gfx950 -O2 -std=c++17 -fPIC -Wno-unused-value $WG_TIMING_FLAGS -c tools/wg_timing.hip -o build/wg_timing.o &&
 $H --offload-arch=gfx950 -fPIC -o build/wg_timing build/wg_timing.o $(ls $OBJ/*.o | grep -v '/part[0-9]\.o$') -ldl) &
wait
ls -la build/wg_timing build/traffic_calib build/inst_bench
# the static instruction mix of the built objects x the measured issue costs (tools/gpu_counters.sh takes these when present:
# object files do not always travel to the GPU box)
INST_BENCH=${INST_BENCH:-profiles/r02_microbench/inst_bench_run3.txt}
python3 tools/issue_weights.py part0 k_compose_wg $INST_BENCH > build/issue_weights_compose.json
python3 tools/issue_weights.py part2 k_tree_level $INST_BENCH > build/issue_weights_matmul.json
