// node_spans_asan.cpp - the host helper of the device-input node ingest (kwok_amd/csrc/node_spans.h:
// listed_in_range) under ASan / UBSan, without a GPU: the listed documents' indices against the kept list and the
// frames, at and past both ends, then used the way the engine uses them.  tools/node_spans_asan.sh.
#include <stdio.h>

#include <vector>

#include "node_spans.h"

static int fails = 0;
#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            fails++;                                                \
        }                                                           \
    } while (0)

int main() {
    using kwok::listed_in_range;
    const std::vector<uint32_t> kidx{0, 3, 4, 9};  // four kept records of ten frames
    CHECK(listed_in_range({}, kidx, 10));
    CHECK(listed_in_range({}, {}, 0));
    CHECK(listed_in_range({0, 1, 2, 3}, kidx, 10));
    CHECK(listed_in_range({3, 3, 0}, kidx, 10));            // repeats and any order
    CHECK(!listed_in_range({4}, kidx, 10));                 // one past the kept list
    CHECK(!listed_in_range({0, 0xFFFFFFFFu}, kidx, 10));
    CHECK(!listed_in_range({3}, kidx, 9));                  // its frame one past the frames
    CHECK(listed_in_range({2}, kidx, 5) && !listed_in_range({2}, kidx, 4));
    CHECK(!listed_in_range({0}, {}, 10) && !listed_in_range({0}, kidx, 0));
    // as the engine uses it: every access behind a true answer is inside both arrays (the sanitizer watches)
    std::vector<int> frames(10, 7);
    long sum = 0;
    for (uint32_t a = 0; a < 6; a++)
        for (uint32_t b = 0; b < 6; b++) {
            const std::vector<uint32_t> list{a, b};
            if (listed_in_range(list, kidx, frames.size()))
                for (uint32_t i : list) sum += frames[kidx[i]];
        }
    CHECK(sum == 7 * 2 * 16);
    printf(fails ? "node_spans_asan: %d FAILED\n" : "node_spans_asan: ok\n", fails);
    return fails ? 1 : 0;
}
