#!/bin/bash
# Diagnostic build with in-kernel clock stamps (never shipped): tools/ab/libroomnet_hip_clock.so
# Every stage-kernel workgroup stamps s_memtime / s_memrealtime at entry and exit (RN_CLOCK in the kernels, rn_clock.h on the
# host).  Select the library with ROOMNET_HIP_LIB=<path>.  A forward pass prints the median clock per launch when
# RN_CLOCK_REPORT is set in the environment at the moment the pass is enqueued: run >= 2 s of back-to-back passes without it,
# set it (os.environ / setenv in the running process) for the last one.  (run csrc/build.sh first: other objects are reused)
set -euo pipefail
ROOT="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
# the files that carry RN_CLOCK blocks (the kernels) or include the host side
FILES="$(cd "$ROOT/roomnet_amd/csrc" && grep -l 'RN_CLOCK\|rn_clock\.h' *.hip | sed 's/\.hip$//' | tr '\n' ' ')"
exec "$ROOT/tools/build_variant2.sh" clock "$FILES" -DRN_CLOCK
