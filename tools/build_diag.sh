#!/bin/bash
# Diagnostic library builds (measurement only; the one switch left is -DFS_STAMPS), from the library's
# own Makefile and source list:
#   tools/build_diag.sh <name> "<-D flags>"  ->  seqs_amd/lib/diag/libframesum_<name>.so
set -e
make -B -C "$(dirname "$0")/../seqs_amd/csrc" lib OUT="../lib/diag/libframesum_$1.so" EXTRA="$2"
