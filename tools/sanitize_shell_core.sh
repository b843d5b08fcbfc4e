#!/bin/bash
# The host compilation of csrc/nrtdsm/shell_core.hip.h + shell_build.h + shell_instance.hip.h (the text the device kernels run) under AddressSanitizer
# and UndefinedBehaviorSanitizer, as a stand-alone program (tools/shell_sanitize_main.cpp): no GPU, nothing loaded into Python.
#   bash tools/sanitize_shell_core.sh [output directory, default a fresh temporary one]
set -eu
cd "$(dirname "$0")/.."
OUT=${1:-$(mktemp -d)}
g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -ffp-contract=off -fno-fast-math -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined \
    -Igfxexp_amd/csrc -Iinclude tools/shell_sanitize_main.cpp -o "$OUT/shell_sanitize"
ASAN_OPTIONS=detect_leaks=1:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 "$OUT/shell_sanitize"
echo "sanitizers: no report"
