#!/bin/bash
# Incremental rebuild: tools/build_inc.sh FILE [FILE ...] (names as in csrc/build.sh, without .hip; objects of the other files are reused from build/obj;
# run roomnet_amd/csrc/build.sh once first).  Relinks both libraries and reports the spills of the files it compiled.
set -euo pipefail
ROOT="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
[ $# -ge 1 ] || { echo "usage: $0 FILE [FILE ...]" >&2; exit 2; }
RN_FILES="$*" exec "$ROOT/roomnet_amd/csrc/build.sh"
