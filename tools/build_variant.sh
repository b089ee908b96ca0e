#!/bin/bash
# tools/build_variant.sh <name> [extra hipcc flags]: the product source with extra -D flags -> tools/ubench/bin/libarah_<name>.so
NAME=$1; shift
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p $ROOT/tools/ubench/bin
cd $ROOT/arah_release_amd/csrc
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -Wno-unused-value -Xclang -target-feature -Xclang -packed-fp32-ops ${ARAH_SLP:--fno-slp-vectorize} "$@" -shared -fPIC arah_hip.hip -o $ROOT/tools/ubench/bin/libarah_$NAME.so 2>&1 | grep -v "not a recognized"
ls -la $ROOT/tools/ubench/bin/libarah_$NAME.so
