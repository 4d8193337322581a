#!/bin/bash
# AddressSanitizer + UBSan (trapping) run of the host side of the gate polynomials as a stand-alone program: host_fr.hip (the
# twin msm_amd_host_fr_gate_eval, the shared check msm_amd_fr_gate_check, the plan aid) and host_ntt.hip are compiled with the
# host instrumented (the device code is not) and linked with tools/gate_asan_check.cpp, which calls them on exactly sized heap
# buffers.  No GPU, no python.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
OUT=$ROOT/build_ab/gate_asan
SAN="-Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined -Xarch_host -fsanitize-trap=undefined -Xarch_host -fno-omit-frame-pointer"
mkdir -p "$OUT"
cd "$ROOT/metal-msm-gpu-acceleration_amd/csrc"
for f in host_fr host_ntt; do
  $HIPCC -O1 -g -std=c++17 -fPIC --offload-arch=${ARCH:-gfx950} -Wall -Wno-unused-function $SAN -c -o "$OUT/$f.o" $f.hip
done
HOST_SAN="-fsanitize=address -fsanitize=undefined -fsanitize-trap=undefined -fno-omit-frame-pointer"
$HIPCC -x c++ -O1 -g -std=c++17 $HOST_SAN -c -o "$OUT/main.o" "$ROOT/tools/gate_asan_check.cpp"
$HIPCC --offload-arch=${ARCH:-gfx950} $HOST_SAN -o "$OUT/gate_asan_check" "$OUT/main.o" "$OUT/host_fr.o" "$OUT/host_ntt.o" -lpthread
ASAN_OPTIONS=detect_leaks=1:halt_on_error=1 "$OUT/gate_asan_check"
