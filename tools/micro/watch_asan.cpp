// ASan/UBSan driver of the host watch-stream framer (kwok_frame_watch, codec.cpp):
// every stream of the input file (u32 length + bytes each) is framed from a heap
// copy of exactly its length, so a read past the stream is a report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "kwok_watch.h"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    size_t streams = 0, frames = 0, bad = 0;
    for (;;) {
        uint32_t n;
        if (fread(&n, 4, 1, f) != 1) break;
        char* s = (char*)malloc(n ? n : 1);
        if (n && fread(s, 1, n, f) != n) return 2;
        size_t lines = 0;
        for (uint32_t k = 0; k < n; k++) lines += s[k] == '\n';
        std::vector<kwok_watch_frame> fr(lines + 1);
        size_t nf = 0, used = 0;
        int rc = kwok_frame_watch(s, n, fr.data(), lines, &nf, &used);
        if (rc < 0 || nf != lines || used > n) {
            fprintf(stderr, "stream %zu: rc %d, %zu frames of %zu lines, consumed %zu of %u\n", streams, rc, nf, lines, used, n);
            return 1;
        }
        for (size_t i = 0; i < nf; i++) {  // every span lies inside the stream
            const kwok_watch_frame& x = fr[i];
            const kwok_str sp[5] = {{x.doc_off, x.doc_len}, x.uid, x.resource_version, x.name, x.namespace_};
            for (const kwok_str& q : sp)
                if ((size_t)q.off + q.len > used) {
                    fprintf(stderr, "stream %zu frame %zu: a span outside the consumed bytes\n", streams, i);
                    return 1;
                }
        }
        if (lines) {  // a frames array one too small: KWOK_EINVAL with the count
            size_t nf2 = 0, used2 = 0;
            if (kwok_frame_watch(s, n, fr.data(), lines - 1, &nf2, &used2) != KWOK_EINVAL || nf2 != lines) return 1;
        }
        streams++, frames += nf, bad += rc;
        free(s);
    }
    printf("watch_asan: %zu streams, %zu frames (%zu rejected): clean\n", streams, frames, bad);
    return 0;
}
