#!/bin/bash
# usage: scripts/mkvariant.sh NAME "<extra hipcc flags>"  -> local-feature-refinement_amd/lfr_amd/_variants/NAME.so (built here, travels with gpurun)
set -e
R=$(cd $(dirname $0)/.. && pwd); C=$R/local-feature-refinement_amd/csrc; O=$R/local-feature-refinement_amd/lfr_amd/_variants; mkdir -p $O
SRCS=$(cd $R/local-feature-refinement_amd && python3 -c "from lfr_amd.build import SOURCES; print(' '.join(SOURCES))")      # the one list of sources: lfr_amd/build.py
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -munsafe-fp-atomics -I $R/include -I $C $2 \
  $(for f in $SRCS; do echo $C/$f; done) -o $O/$1.so
echo built $O/$1.so
