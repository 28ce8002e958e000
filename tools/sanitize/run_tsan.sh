#!/bin/bash
# The host-side runtime logic that has no GPU in it -- the micro-batcher (csrc/ipx_batcher.cpp), the process-wide thread pool
# (csrc/ipx_threads.h) and the pool's queue / tickets / feeders (csrc/ipx_pool_core.h) -- under ThreadSanitizer on the CPU, against fake
# device work (tools/sanitize/batcher_host_test.cpp, tools/sanitize/pool_host_test.cpp).
set -e
cd "$(dirname "$0")/../.."
# a directory of its own per run: a fixed path under /tmp may belong to another user, or to a run going on beside this one
out=$(mktemp -d "${TMPDIR:-/tmp}/ipx_sanitize.XXXXXX")
trap 'rm -rf "$out"' EXIT
# ThreadSanitizer's shadow layout only admits the addresses of the usual ASLR range: under a kernel with more mmap randomisation
# it stops at start-up ("unexpected memory mapping").  The two test programs therefore run with address randomisation turned off
# for their own process (setarch -R) wherever a process may ask for that.
norand=
if setarch "$(uname -m)" -R true 2>/dev/null; then norand="setarch $(uname -m) -R"; fi
g++ -std=c++17 -O1 -g -fsanitize=thread -fno-omit-frame-pointer -pthread -o $out/batcher_tsan tools/sanitize/batcher_host_test.cpp
TSAN_OPTIONS=halt_on_error=1:second_deadlock_stack=1 $norand $out/batcher_tsan
g++ -std=c++17 -O1 -g -fsanitize=thread -fno-omit-frame-pointer -pthread -o $out/pool_tsan tools/sanitize/pool_host_test.cpp
TSAN_OPTIONS=halt_on_error=1:second_deadlock_stack=1 $norand $out/pool_tsan
echo "no sanitizer report"
