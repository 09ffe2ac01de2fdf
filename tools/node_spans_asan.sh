#!/bin/bash
# ASan/UBSan run of the device-input node ingest's host helper (CPU only): the check of the listed
# documents' indices before their spans are read from the host's frames (kwok_amd/csrc/node_spans.h).
set -e
cd "$(dirname "$0")/.."
OUT=${KWOK_ASAN_OUT:-/tmp/node_spans_asan}
mkdir -p "$OUT"
g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude -Ikwok_amd/csrc \
  tools/micro/node_spans_asan.cpp -o "$OUT/t"
"$OUT/t"
