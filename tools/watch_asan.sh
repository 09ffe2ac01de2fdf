#!/bin/bash
# ASan/UBSan run of the host watch-stream framer (CPU only): the named cases, the line-split
# sweeps and the fuzzed frames of tests/test_watch_frame_gpu.py, and 3000 byte-mutated streams.
set -e
cd "$(dirname "$0")/.."
OUT=${KWOK_ASAN_OUT:-/tmp/watch_asan}
mkdir -p "$OUT"
python - "$OUT/streams.bin" <<'PY'
import random, sys
sys.path.insert(0, "tests"); sys.path.insert(0, ".")
import watch_frames as wf
import test_watch_frame_gpu as T
streams = [s for s, _ in wf.cases().values()] + T.sweep_streams() + [T.fuzz_stream(2000, 9)]
rng = random.Random(5)
base = T.fuzz_stream(300, 10).split(b"\n")
for _ in range(3000):
    b = bytearray(b"\n".join(rng.sample(base, rng.randint(1, 4))) + b"\n")
    for _ in range(rng.randint(1, 6)):
        b[rng.randrange(len(b))] = rng.choice(b'{}[]",:\\0123456789tfnul \n\r\x00\xff')
    streams.append(bytes(b)[:rng.randrange(1, len(b) + 1)])
with open(sys.argv[1], "wb") as f:
    for s in streams:
        f.write(len(s).to_bytes(4, "little") + s)
PY
g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude -Ikwok_amd/csrc \
  tools/micro/watch_asan.cpp kwok_amd/csrc/codec.cpp -o "$OUT/t" -lpthread
"$OUT/t" "$OUT/streams.bin"
