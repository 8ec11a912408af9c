#!/bin/bash
# A/B build of the product library with another kernel source: seqs_amd/lib/ab/libframesum_<name>.so
# (measurement tool; tools/env_sweep.py lib=<name> runs the bench with it through FRAMESUM_LIB). Builds a
# copy of this tree's sources with the library's own Makefile, so its source list is the library's.
# usage: tools/build_ab.sh <name> <framesum_kernel.hip to use | git revision>
#   e.g. tools/build_ab.sh old a05f721     (that commit's kernel, this tree's host sources)
set -e
name=$1; src=$2
R=$(cd "$(dirname "$0")/.." && pwd)
d=$(mktemp -d)/a/b/csrc; mkdir -p "$d" "$d/../../include"
cp "$R"/seqs_amd/csrc/*.cpp "$R"/seqs_amd/csrc/*.h "$R"/seqs_amd/csrc/*.hip "$R"/seqs_amd/csrc/Makefile "$d"/
cp "$R"/include/*.h "$d/../../include/"
if [ -f "$src" ]; then cp "$src" "$d/framesum_kernel.hip"; else git -C "$R" show "$src:seqs_amd/csrc/framesum_kernel.hip" > "$d/framesum_kernel.hip"; fi
make -B -C "$d" lib OUT="$R/seqs_amd/lib/ab/libframesum_$name.so"
ls -la "$R/seqs_amd/lib/ab/libframesum_$name.so"
