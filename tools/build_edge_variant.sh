#!/bin/bash
# Build a variant of the engine that differs from the product build in kernels_edge.hip (and, for -DDFM_EDGE_TRACE / _STAMP, in the two
# host files that hold those #ifs: api_complex.hip allocates the stamp buffer, api_forward.hip arms and reads it) only; the other
# objects are the product's (make -C dfmdock_amd/csrc first).  Output: tools/variants/NAME.so (git-ignored) + a resource line.
#   bash tools/build_edge_variant.sh trace "-DDFM_EDGE_TRACE"      (the diagnostic builds are listed in kernels_edge.hip, k_edge_f32m)
set -e
NAME=$1; EXTRA=$2
ROOT=$(cd $(dirname $0)/.. && pwd); SRC=$ROOT/dfmdock_amd/csrc; OBJ=/tmp/dfm_ev_$NAME; mkdir -p $OBJ $ROOT/tools/variants
COMMON="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -fno-slp-vectorize $EXTRA"
hipcc $COMMON -mllvm -amdgpu-atomic-optimizer-strategy=None -c $SRC/kernels_edge.hip -o $OBJ/kernels_edge.o
REPLACED="kernels_edge"
case "$EXTRA" in *TRACE*|*STAMP*)
    for f in api_complex api_forward; do hipcc $COMMON -c $SRC/$f.hip -o $OBJ/$f.o; REPLACED="$REPLACED $f"; done;;
esac
OBJS=""
for o in $SRC/*.o; do
    b=$(basename $o .o)
    case " $REPLACED " in *" $b "*) OBJS="$OBJS $OBJ/$b.o";; *) OBJS="$OBJS $o";; esac
done
hipcc --offload-arch=gfx950 -shared -fPIC -o $ROOT/tools/variants/$NAME.so $OBJS
python3 $ROOT/tools/kernel_resources.py $ROOT/tools/variants/$NAME.so k_edge_msgILi1ELi1ELi0 | sed "s/^/$NAME: /"
