#!/bin/bash
# ASan/UBSan run of the host List framer (CPU only): the named cases, the split's boundary
# sweeps, every prefix of a small body and 4000 byte-mutated bodies of tests/list_bodies.py.
set -e
cd "$(dirname "$0")/.."
OUT=${KWOK_ASAN_OUT:-/tmp/list_asan}
mkdir -p "$OUT"
python - "$OUT/bodies.bin" <<'PY'
import sys
sys.path.insert(0, "tests"); sys.path.insert(0, ".")
import list_bodies as lb
bodies = [b for b, _, _ in lb.cases().values()] + lb.sweep_bodies()
bodies += [lb.PREFIX_BODY[:k] for k in range(len(lb.PREFIX_BODY) + 1)] + lb.mutated_bodies(4000, 9)
with open(sys.argv[1], "wb") as f:
    for s in bodies:
        f.write(len(s).to_bytes(4, "little") + s)
PY
g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude -Ikwok_amd/csrc \
  tools/micro/list_asan.cpp kwok_amd/csrc/codec.cpp -o "$OUT/t" -lpthread
"$OUT/t" "$OUT/bodies.bin"
