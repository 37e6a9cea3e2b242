#!/bin/bash
# AddressSanitizer + UBSan run of the lean lane-order pass of the tile builder (host code only: CPU, no GPU needed):
# icospheres, a jittered disk, a valence-32 vertex, bad indices; 1 and 4 threads.  usage: tools/asan_lane_order.sh
R=$(cd "$(dirname "$0")/.." && pwd)
C=$R/membrane_solver_amd/csrc
mkdir -p /tmp/ms_asan
/opt/rocm/bin/hipcc -x hip --offload-arch=gfx950 --cuda-host-only -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer \
  -std=c++17 -I$C -I$R/include $R/tools/micro/asan_lane_order.cpp $C/ms_tiles.cpp -o /tmp/ms_asan/asan_lane_order || exit 1
/tmp/ms_asan/asan_lane_order | tail -6
echo "exit ${PIPESTATUS[0]}"
