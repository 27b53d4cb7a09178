#!/bin/bash
# usage: bash tools/build_variant.sh <name> [extra hipcc flags...]   ->  build_ab/libgsrast_<name>.so
# A build of the library with extra -D switches for same-box A/B runs (tools/ab_libs.sh, GSRAST_LIB); never loaded by the product.
# The sources are every *.hip of SRC_DIR (default: this tree's csrc; another tree's csrc builds that tree), at most 16 compiles at a
# time; a compile that fails ends the build before the link.
set -eo pipefail
name=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
src=${SRC_DIR:-$root/taichi_3d_gaussian_splatting_amd/csrc}
obj=$root/build_ab/obj_$name
rm -rf "$obj"; mkdir -p "$obj"
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fno-slp-vectorize -Wall -Wno-unused-function"
export FLAGS src obj
# (xargs returns non-zero when any of its commands does)
ls "$src"/*.hip | xargs -P 16 -I{} bash -c 'f=$(basename "$1" .hip); /opt/rocm/bin/hipcc $FLAGS "${@:2}" -c "$src/$f.hip" -o "$obj/$f.o"' _ {} "$@"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$root/build_ab/libgsrast_$name.so" "$obj"/*.o
echo built "$root/build_ab/libgsrast_$name.so"
