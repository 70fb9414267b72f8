#!/bin/bash
# AddressSanitizer + UndefinedBehaviorSanitizer over the host paths of the caller's-own-track ingest (upload and ingest growing across calls, the
# refusals, the poison hook, the extract calls on the ingested track, destroy with and without a track): tools/world_ingest_host_check.cpp, a
# stand-alone program, linked against the sanitizer build of the emulator library.  CPU only, a few minutes after the library is built.
#   scripts/asan_world_ingest.sh
cd "$(dirname "$0")/.." || exit 1
set -o pipefail
LIB=$(python -c "from realtime_yukarin_amd import build; print(build.build_emu(sanitize=True))" | tail -1) || exit 1
CXX=/opt/rocm/lib/llvm/bin/clang++
[ -x "$CXX" ] || CXX=$(command -v clang++) || exit 1
RT_DIR=$(dirname "$($CXX -print-file-name=libclang_rt.asan-x86_64.so)")
mkdir -p build
$CXX -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -shared-libasan -Iinclude tools/world_ingest_host_check.cpp \
  "$LIB" -Wl,-rpath,"$(dirname "$LIB")" -Wl,-rpath,"$RT_DIR" -pthread -o build/world_ingest_host_check || exit 1
ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 ./build/world_ingest_host_check 2>&1 | tee build/asan_world_ingest.log | tail -20
