#!/bin/bash
# Builds an experimental variant of the library with extra -D flags: tools/build_variant.sh NAME "-DMRT_X=1 ..."
# -> metal-raytracing_amd/variants/libmrt_hip_NAME.so (git-ignored; select it with MRT_LIB_PATH).
# The units are the Makefile's OBJS: there is one list.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd); C=$ROOT/metal-raytracing_amd/csrc; V=$ROOT/metal-raytracing_amd/variants/$1
mkdir -p $V
FL="-O3 -std=c++17 -fPIC -ffp-contract=off $2"
OBJS=$(sed -n 's/^OBJS *= *//p' $C/Makefile)
[ -n "$OBJS" ] || { echo "no OBJS in $C/Makefile" >&2; exit 1; }
for o in $OBJS; do
    f=${o%.o}
    if [ -f $C/$f.hip ]; then /opt/rocm/bin/hipcc --offload-arch=gfx950 $FL -c -o $V/$o $C/$f.hip & else /opt/rocm/bin/hipcc $FL -c -o $V/$o $C/$f.cpp & fi
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $LINK_EXTRA -o $ROOT/metal-raytracing_amd/variants/libmrt_hip_$1.so $(for o in $OBJS; do echo $V/$o; done) -ldl -lpthread
echo built $ROOT/metal-raytracing_amd/variants/libmrt_hip_$1.so
