#!/bin/bash
# Experimental build of ONE kernel file: tools/build_variant.sh NAME FILE [extra hipcc flags]
# -> tools/ab/libroomnet_hip_NAME.so (other objects are taken from build/obj: run csrc/build.sh first).
# Select at run time with ROOMNET_HIP_LIB=<path>.  Diagnostic only; never shipped.
set -euo pipefail
exec "$(dirname "${BASH_SOURCE[0]}")/build_variant2.sh" "$@"
