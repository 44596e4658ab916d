#!/bin/bash
# An A/B build of the library with extra kernel flags, beside the shipping one:  bash tools/build_variant.sh <name> "<flags>"
#   -> gpurun_ab/<name>/liblt_hip.so   (git-ignored, travels to the GPU box; select with LT_HIP_LIBRARY=gpurun_ab/<name>/liblt_hip.so)
# The file list, flags and rules are the Makefile's own: objects and library go to the variant's directory.
set -e -o pipefail
NAME=$1; FLAGS=$2
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$ROOT/gpurun_ab/$NAME
mkdir -p "$OUT"
make -s -j8 -C "$ROOT/light_transport_amd/csrc" OBJDIR="$OUT" OUT="$OUT/liblt_hip.so" EXTRA_KFLAGS="$FLAGS" 2>&1 | { grep -v "argument unused" || true; }
ls -la "$OUT/liblt_hip.so"
