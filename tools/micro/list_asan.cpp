// ASan/UBSan driver of the host List framer (kwok_frame_list, codec.cpp) and of the
// two host pieces the device framer calls (frame_item, list_envelope): every body
// of the input file (u32 length + bytes each) is framed from a heap copy of exactly
// its length, so a read past the body is a report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "codec.h"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    size_t bodies = 0, items = 0, bad = 0;
    for (;;) {
        uint32_t n;
        if (fread(&n, 4, 1, f) != 1) break;
        char* s = (char*)malloc(n ? n : 1);
        if (n && fread(s, 1, n, f) != n) return 2;
        size_t cap = 0;
        for (uint32_t k = 0; k < n; k++) cap += s[k] == '{';
        std::vector<kwok_watch_frame> fr(cap + 1);
        size_t nf = 0;
        kwok_list_info info;
        const int rc = kwok_frame_list(s, n, fr.data(), cap, &nf, &info);
        if ((rc != KWOK_OK && rc != KWOK_EINVAL) || (rc && nf) || nf > cap) {
            fprintf(stderr, "body %zu: rc %d, %zu frames\n", bodies, rc, nf);
            return 1;
        }
        const kwok_str is[4] = {info.kind, info.resource_version, info.continue_, info.items};
        for (const kwok_str& q : is)
            if ((size_t)q.off + q.len > n) {
                fprintf(stderr, "body %zu: an info span outside the body\n", bodies);
                return 1;
            }
        for (size_t i = 0; i < nf; i++) {  // every span lies inside its item, the item inside the items array
            const kwok_watch_frame& x = fr[i];
            if (x.doc_off <= info.items.off || (size_t)x.doc_off + x.doc_len >= (size_t)info.items.off + info.items.len) return 1;
            const kwok_str sp[4] = {x.uid, x.resource_version, x.name, x.namespace_};
            for (const kwok_str& q : sp)
                if (q.len && (q.off < x.doc_off || (size_t)q.off + q.len > (size_t)x.doc_off + x.doc_len)) {
                    fprintf(stderr, "body %zu item %zu: a span outside the item\n", bodies, i);
                    return 1;
                }
            kwok_watch_frame y;  // the per-item entry over the same span gives the same frame
            if (!kwok::frame_item(s, x.doc_off, x.doc_off + x.doc_len, &y) || memcmp(&x, &y, sizeof x)) {
                fprintf(stderr, "body %zu item %zu: frame_item differs\n", bodies, i);
                return 1;
            }
        }
        if (rc == KWOK_OK && info.items.len) {  // the envelope around the items array: the same info, or not the device's
            kwok_list_info e2;
            memset(&e2, 0, sizeof e2);
            const int er = kwok::list_envelope(s, n, info.items.off, info.items.off + info.items.len - 1, &e2);
            if (er < 0 || (er == 0 && memcmp(&e2, &info, sizeof info))) {
                fprintf(stderr, "body %zu: list_envelope %d differs\n", bodies, er);
                return 1;
            }
        }
        if (n > 2) {  // any two offsets as brackets, any span as an item: no read outside the body
            kwok_list_info e3;
            kwok_watch_frame y;
            (void)kwok::list_envelope(s, n, n / 3, n - 1 - n / 4, &e3);
            (void)kwok::frame_item(s, n / 3, n - n / 4, &y);
        }
        if (nf) {  // a frames array one too small: KWOK_EINVAL with the count
            size_t nf2 = 0;
            if (kwok_frame_list(s, n, fr.data(), nf - 1, &nf2, &info) != KWOK_EINVAL || nf2 != nf) return 1;
        }
        bodies++, items += nf, bad += rc != KWOK_OK;
        free(s);
    }
    printf("list_asan: %zu bodies, %zu items (%zu bodies rejected): clean\n", bodies, items, bad);
    return 0;
}
