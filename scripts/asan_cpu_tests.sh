#!/bin/bash
# AddressSanitizer over the host code (parser, graph stage on the host, size cap, device-context bookkeeping) with the CPU test
# suite: builds the .cpp files of lfr_amd/build.py's SOURCES with -fsanitize=address, links them with the regular device
# objects (csrc/_obj, run `python __graft_entry__.py` first) into /tmp/asan/liblfr_asan.so and runs `pytest -m "not gpu"` on it.
set -e
R=$(cd $(dirname $0)/.. && pwd); C=$R/local-feature-refinement_amd/csrc; O=/tmp/asan; mkdir -p $O
H=/opt/rocm/bin/hipcc
SRCS=$(cd $R/local-feature-refinement_amd && python3 -c "from lfr_amd.build import SOURCES; print(' '.join(SOURCES))")      # the one list of sources: lfr_amd/build.py
HOST=$(for f in $SRCS; do case $f in *.cpp) echo $f;; esac; done)
for f in $HOST; do
  $H --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -fsanitize=address -fno-omit-frame-pointer -I $R/include -I $C -c $C/$f -o $O/$f.o
done
$H --offload-arch=gfx950 -shared -fPIC -fsanitize=address -shared-libsan $(for f in $HOST; do echo $O/$f.o; done) $C/_obj/*.hip.o -o $O/liblfr_asan.so
ASAN=$(/opt/rocm/lib/llvm/bin/clang -print-file-name=libclang_rt.asan-x86_64.so)
cd $R && LD_PRELOAD=$ASAN ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 LFR_LIB_OVERRIDE=$O/liblfr_asan.so python -m pytest tests -x -q -m "not gpu" "$@"
