#!/bin/bash
# The host model of gfx_tfdm_update_heights (csrc/tfdm/tfdm_update.h over the TFDM core, tests/tfdm_update_host.cpp) under
# AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program (tools/tfdm_update_sanitize_main.cpp): no GPU, nothing
# loaded into Python.
#   bash tools/sanitize_tfdm_update.sh [output directory, default a fresh temporary one]
set -eu
cd "$(dirname "$0")/.."
OUT=${1:-$(mktemp -d)}
g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -ffp-contract=off -fno-fast-math -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined \
    -Igfxexp_amd/csrc -Iinclude tools/tfdm_update_sanitize_main.cpp -o "$OUT/tfdm_update_sanitize"
ASAN_OPTIONS=detect_leaks=1:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 "$OUT/tfdm_update_sanitize"
echo "sanitizers: no report"
