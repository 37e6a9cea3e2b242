#!/bin/bash
# AddressSanitizer + UBSan run of ms_leaflet_absent_flags_host (the flag update of ms_set_leaflet_absent: the absence bit
# through the vertex permutation; host code only: CPU, no GPU needed).  The library's host side (ms_api.cpp, ms_tiles.cpp)
# and tools/micro/asan_leaflet_absent.cpp are compiled with the sanitizers on the host pass and linked with the kernel
# objects of the ordinary build into a stand-alone program; nothing is loaded into Python.
# usage: tools/asan_leaflet_absent.sh
R=$(cd "$(dirname "$0")/.." && pwd)
C=$R/membrane_solver_amd/csrc
O=$(mktemp -d)
make -s -C $C -j16 || exit 1
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
  -std=c++17 -Wno-unused-result -I$C -I$R/include -x hip $R/tools/micro/asan_leaflet_absent.cpp $C/ms_api.cpp $C/ms_tiles.cpp -x none \
  $C/build/ms_kernels.o $C/build/ms_pins.o $C/build/ms_edge.o $C/build/ms_rim.o $C/build/ms_thetab.o $C/build/ms_rimmatch.o \
  $C/build/ms_thetab_bnd.o $C/build/ms_area.o $C/build/ms_enforce.o \
  -fsanitize=address,undefined -ldl -o $O/asan_leaflet_absent || exit 1
$O/asan_leaflet_absent
rc=$?
echo "exit $rc"
exit $rc
