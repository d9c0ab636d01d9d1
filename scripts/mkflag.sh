#!/bin/bash
# mkflag.sh <tag> <file.hip> <-Dflags...> : lib_<tag> = current objects with <file.hip> (working tree)
# recompiled with the extra flags (A/B of build switches).  The flags are the Makefile's own HIPFLAGS.
set -e
cd "$(dirname "$0")/../event-camera-clustering-and-optical-flow-estimation_amd"
mkvar() { printf '_print_var:\n\t@echo $(%s)\n' "$1" | make -s --no-print-directory -f Makefile -f - _print_var; }
HIPCC=$(mkvar HIPCC); FLAGS="$(mkvar HIPFLAGS) -fvisibility=hidden"; ARCH=$(mkvar ARCH)
T=$1; F=$2; shift 2
rm -rf build_exp/f_$T lib_$T; mkdir -p build_exp/f_$T lib_$T
cp build/*.o build_exp/f_$T/
$HIPCC $FLAGS "$@" -c csrc/$F -o build_exp/f_$T/${F%.hip}.o
$HIPCC -shared --offload-arch=$ARCH -o lib_$T/libecc.so build_exp/f_$T/*.o -lpthread
echo built lib_$T
