#!/bin/bash
# mkvar.sh <tag> <file.hip>... : lib_<tag> = current objects with the listed files from HEAD (compiled
# with the Makefile's own HIPFLAGS, against the working tree's headers)
set -e
cd "$(dirname "$0")/../event-camera-clustering-and-optical-flow-estimation_amd"
mkvar() { printf '_print_var:\n\t@echo $(%s)\n' "$1" | make -s --no-print-directory -f Makefile -f - _print_var; }
HIPCC=$(mkvar HIPCC); FLAGS="$(mkvar HIPFLAGS) -fvisibility=hidden -Icsrc -I../include"; ARCH=$(mkvar ARCH)
T=$1; shift
rm -rf build_exp/v_$T lib_$T; mkdir -p build_exp/v_$T/src lib_$T
cp build/*.o build_exp/v_$T/
for f in "$@"; do
  git show HEAD:event-camera-clustering-and-optical-flow-estimation_amd/csrc/$f > build_exp/v_$T/src/$f
  $HIPCC $FLAGS -c build_exp/v_$T/src/$f -o build_exp/v_$T/${f%.hip}.o &
done
wait
$HIPCC -shared --offload-arch=$ARCH -o lib_$T/libecc.so build_exp/v_$T/*.o -lpthread
echo built lib_$T
