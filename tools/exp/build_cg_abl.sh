#!/bin/sh
# Ablation builds of the split tiles' production schedule in csrc/conv_gemm.hip (round 6): the product objects + conv_gemm.hip compiled with
# -DCG_ABL=<bits> (1 no activation split, 2 no DMA wait before the slice barrier, 4 no DMA in the K loop, 8 no epilogue, 16 no MFMAs; results
# are garbage, the TIME is the measurement).  Writes adafocus_amd/csrc/exp_build/libadafocus_hip_cg<bits>.so; run with ADAF_LIB=<that file>.
# Objects and flags are the Makefile's: its SRCS with conv_gemm.o replaced (built first if they are not there), its CXXFLAGS + -DCG_ABL.
# usage: build_cg_abl.sh 1 2 4 ...
set -e
cd "$(dirname "$0")/../../adafocus_amd/csrc"
make -j16
OBJS=$(sed -n 's/^SRCS *= *//p' Makefile | tr ' ' '\n' | grep -v '^conv_gemm\.hip$' | sed 's/\.hip$/.o/' | tr '\n' ' ')
FLAGS=$(sed -n 's/^CXXFLAGS *= *//p' Makefile | sed 's/\$(ARCH)/gfx950/')
[ -n "$OBJS" ] && [ -n "$FLAGS" ]
mkdir -p exp_build
for k in "$@"; do
  /opt/rocm/bin/hipcc $FLAGS -DCG_ABL=$k -c conv_gemm.hip -o exp_build/conv_gemm_abl$k.o &
done
wait
for k in "$@"; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $OBJS exp_build/conv_gemm_abl$k.o -o exp_build/libadafocus_hip_cg$k.so
done
ls -la exp_build/*cg*.so
