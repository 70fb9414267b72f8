#!/bin/bash
# AddressSanitizer + UndefinedBehaviorSanitizer over the host paths of the row bank (create, appends of three streams until one stream's rings are
# full, retire of one stream and wrap, fetch and pick with pads / empty spans / spans across the ring end, growing tables, the refusals, poison,
# reset, destroy) and over the index arithmetic of its kernels on the emulator: tools/rowbank_host_check.cpp, a stand-alone program, linked
# against the sanitizer build of the emulator library.  CPU only, a few minutes after the library is built.
#   scripts/asan_rowbank.sh
cd "$(dirname "$0")/.." || exit 1
set -o pipefail
LIB=$(python -c "from realtime_yukarin_amd import build; print(build.build_emu(sanitize=True))" | tail -1) || exit 1
CXX=/opt/rocm/lib/llvm/bin/clang++
[ -x "$CXX" ] || CXX=$(command -v clang++) || exit 1
RT_DIR=$(dirname "$($CXX -print-file-name=libclang_rt.asan-x86_64.so)")
mkdir -p build
$CXX -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -shared-libasan -Iinclude tools/rowbank_host_check.cpp \
  "$LIB" -Wl,-rpath,"$(dirname "$LIB")" -Wl,-rpath,"$RT_DIR" -pthread -o build/rowbank_host_check || exit 1
ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 ./build/rowbank_host_check 2>&1 | tee build/asan_rowbank.log | tail -20
