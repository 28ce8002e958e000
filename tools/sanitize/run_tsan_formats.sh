#!/bin/bash
# The micro-batcher's format routing (csrc/ipx_batcher.cpp: JPEG, PNG and GIF uploads, one format per job) under ThreadSanitizer on the
# CPU, against a fake backend that records every job's kind (tools/sanitize/batcher_formats_host_test.cpp).  Beside run_tsan.sh, which
# keeps the queue / timer / ticket logic.
set -e
cd "$(dirname "$0")/../.."
# a directory of its own per run: a fixed path under /tmp may belong to another user, or to a run going on beside this one
out=$(mktemp -d "${TMPDIR:-/tmp}/ipx_sanitize.XXXXXX")
trap 'rm -rf "$out"' EXIT
# ThreadSanitizer's shadow layout only admits the addresses of the usual ASLR range (run_tsan.sh has the why): the test program runs
# with address randomisation turned off for its own process wherever a process may ask for that.
norand=
if setarch "$(uname -m)" -R true 2>/dev/null; then norand="setarch $(uname -m) -R"; fi
g++ -std=c++17 -O1 -g -fsanitize=thread -fno-omit-frame-pointer -pthread -o $out/batcher_formats_tsan tools/sanitize/batcher_formats_host_test.cpp
TSAN_OPTIONS=halt_on_error=1:second_deadlock_stack=1 $norand $out/batcher_formats_tsan
echo "no sanitizer report"
