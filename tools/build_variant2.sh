#!/bin/bash
# Experimental build with extra flags applied to SEVERAL kernel files: tools/build_variant2.sh NAME "FILE1 FILE2" [flags]
# -> tools/ab/libroomnet_hip_NAME.so (other objects are taken from build/obj: run csrc/build.sh first).
set -euo pipefail
ROOT="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
[ $# -ge 2 ] || { echo "usage: $0 NAME \"FILE ...\" [extra hipcc flags]" >&2; exit 2; }
NAME="$1"; FILES="$2"; shift 2
RN_VARIANT="$NAME" RN_FILES="$FILES" RN_VARIANT_FLAGS="-Wno-unused-variable -Wno-unused-but-set-variable $*" \
    exec "$ROOT/roomnet_amd/csrc/build.sh"
