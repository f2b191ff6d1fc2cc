#!/bin/bash
# Probe build of csrc/gemm_planes.hip with phase stamps in k_gemm_rows_k1 (-DP2M_K1_TRACE) and its run: see
# tools/probes/rows_k1_probe.py.   bash tools/k1_trace.sh build | run [B]
set -u
R=$(cd "$(dirname "$0")/.." && pwd)
CC=${HIPCC:-$(command -v hipcc || echo /opt/rocm/bin/hipcc)}
L=$R/pose2mesh_release_amd/lib
if [ "$1" = build ]; then
  mkdir -p $L/abl
  $CC --offload-arch=gfx950 -O3 -std=c++17 -fPIC -c -DP2M_PROBE_BUILD -DP2M_K1_TRACE -o $L/abl/gemm_K1TRACE.o $R/pose2mesh_release_amd/csrc/gemm_planes.hip || exit 1
  objs=$(ls $L/obj/*.o | grep -v "/gemm_planes.o")
  $CC --offload-arch=gfx950 -shared -fPIC -o $L/abl/libp2m_hip_K1TRACE.so $objs $L/abl/gemm_K1TRACE.o && rm -f $L/abl/gemm_K1TRACE.o
  ls -la $L/abl
else
  P2M_HIP_LIB=$L/abl/libp2m_hip_K1TRACE.so P2M_ROWS_K1=1 python $R/tools/probes/rows_k1_probe.py "${@:2}" 2>&1 | grep -v amdgpu
fi
