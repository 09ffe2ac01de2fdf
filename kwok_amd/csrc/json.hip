// json.hip - the watch-event codec's pod decode on the GPU (SURVEY.md §8(f)
// rank 2: "Watch-event -> SoA ingest codec ... later as a GPU JSON scanner").
//
// The host codec (codec.cpp, kwok_decode_pod) parses a Kubernetes Pod document
// into a DOM and derives the record kwok_ingest_pods takes: the routing flags of
// WatchPods / ListPods (pod_controller.go:252-269, 301-343: needLockPod's
// disregard selectors, deletionTimestamp, finalizers), the `{{ with .status }}`
// guard and computePatchData's strategic-merge no-op test (pod_controller.go:
// 404-439).  Here one thread scans one document in a single pass -
// no DOM: a streaming tokenizer (jparse) drives a handler (PodScan) that keeps
// only what the record needs, with the zero-value of every container tracked as
// the scan closes it (the omitempty semantics of the corev1 round trip).
//
// The scan decides exactly what the host codec decides, byte for byte, for the
// documents it accepts: the same kwok_pod_event (flags, phase, creation time,
// string spans into the arena), name, namespace and pod spec.  What it does not
// decide is listed for the host codec, never guessed (JSON_HOST):
//   * a JSON escape in a string that is compared or mapped (a key the scan
//     routes on, a label / annotation key, a selector-matched value, the status
//     phase, condition fields, container status fields): the host compares
//     decoded text.  Escapes in referenced strings are KWOK_EDOMAIN, as in the
//     host codec; escapes anywhere else change nothing.
// Documents outside the accepted JSON are KWOK_EDOMAIN, as malformed documents
// are for the host parser (same grammar: its lenient numbers, depth <= 64,
// surrogate pairs).
// A status that precedes the metadata or spec (its no-op test needs the creation
// time, the containers and readiness gates) is skipped by the first pass and
// scanned by a second one over its own bytes once the document has been read
// (Go's json.Marshal writes metadata, spec, status in that order; other writers
// need not).
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace kwok {

namespace {

// ---------------------------------------------------------------------------
// a document's bytes, read 16 at a time (the arena is 16-aligned and padded).
// A 64-byte window (a quarter of the refills) measured slower: a C5 batch of 10k
// node documents 0.68 -> 1.01 ms in k_json_nodes - the scan is bound by its
// per-byte instructions and the lanes' divergent paths, not by the refills
// ---------------------------------------------------------------------------
// positions are 32-bit: the JSON entry points take arenas below 4 GiB (engine.cpp), and
// half the scan's position arithmetic was 64-bit pairs
typedef uint32_t jpos;
struct JRd {
    const uint8_t* a;
    jpos pos, end;
    jpos wb;
    uint4 w;
    __device__ __forceinline__ uint32_t at(jpos p) {
        const jpos b = p & ~15u;
        if (b != wb) {
            wb = b;
            w = *reinterpret_cast<const uint4*>(a + b);
        }
        // (the byte picked from values, not by a select of the window's field addresses,
        // which the compiler would form from `o < 4 ? w.x : ...`: an indexed load keeps
        // the reader - and the scan state beside it - in scratch memory)
        const uint32_t o = (uint32_t)(p - b);
        const uint64_t q = o < 8 ? ((uint64_t)w.y << 32 | w.x) : ((uint64_t)w.w << 32 | w.z);
        return (uint32_t)(q >> (8 * (o & 7))) & 0xFFu;
    }
    __device__ __forceinline__ int peek() { return pos < end ? (int)at(pos) : -1; }
    // bytes from p up to the first one that ends a string's plain run (a quote, a
    // backslash or a control character), within p's 16-byte window: that byte's
    // offset from p, or the bytes to the window's end when the window holds none
    __device__ __forceinline__ uint32_t plain_run(jpos p);
};

// bit k set for each byte k of x that ends a string's plain run: a quote, a
// backslash or a control character (SWAR: a byte is zero iff its high bit stays
// clear below; the four high bits gathered by one multiply)
__device__ __forceinline__ uint32_t str_special4(uint32_t x) {
    auto zero = [](uint32_t y) { return ~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y | 0x7F7F7F7Fu); };
    const uint32_t m = zero(x ^ 0x22222222u) | zero(x ^ 0x5C5C5C5Cu) | zero(x & 0xE0E0E0E0u);
    return (((m >> 7) & 0x01010101u) * 0x01020408u) >> 24;
}
__device__ __forceinline__ uint32_t JRd::plain_run(jpos p) {
    (void)at(p);
    const uint32_t o = (uint32_t)(p - wb);
    const uint32_t m = (str_special4(w.x) | str_special4(w.y) << 4 | str_special4(w.z) << 8 | str_special4(w.w) << 12) &
                       (0xFFFFu << o);
    return (m ? (uint32_t)__builtin_ctz(m) : 16u) - o;
}

__device__ __forceinline__ bool bytes_eq(JRd& r, jpos off, uint32_t len, const uint8_t* s, uint32_t n) {
    if (len != n) return false;
    for (uint32_t k = 0; k < n; k++)
        if (r.at(off + k) != s[k]) return false;
    return true;
}
__device__ __forceinline__ bool span_eq(JRd& r, jpos a, jpos b, uint32_t len) {
    for (uint32_t k = 0; k < len; k++)
        if (r.at(a + k) != r.at(b + k)) return false;
    return true;
}
template <int N>
__device__ __forceinline__ bool lit_eq(JRd& r, jpos off, uint32_t len, const char (&s)[N]) {
    if (len != N - 1) return false;
    for (int k = 0; k < N - 1; k++)
        if (r.at(off + k) != (uint8_t)s[k]) return false;
    return true;
}

// ---------------------------------------------------------------------------
// the tokenizer: codec.cpp Parser's grammar, events to a handler
// ---------------------------------------------------------------------------
enum : uint8_t { J_STR, J_NUM, J_TRUE, J_FALSE, J_NULL };
struct JTok {
    jpos off;  // STR: inside the quotes; else the token
    uint32_t len;
    uint8_t kind;
    bool esc;      // STR held an escape (the span is not the value)
    bool nz;       // not a zero value (omitempty sense: codec.cpp zeroish)
};

__device__ __forceinline__ bool hexv(uint32_t c, uint32_t& v) {
    if (c >= '0' && c <= '9') v = (v << 4) | (c - '0');
    else if (c >= 'a' && c <= 'f') v = (v << 4) | (c - 'a' + 10);
    else if (c >= 'A' && c <= 'F') v = (v << 4) | (c - 'A' + 10);
    else return false;
    return true;
}
__device__ __forceinline__ bool hex4(JRd& r, uint32_t& v) {
    if (r.pos + 4 > r.end) return false;
    v = 0;
    for (int k = 0; k < 4; k++)
        if (!hexv(r.at(r.pos++), v)) return false;
    return true;
}
// a string token at r.pos (the opening quote)
__device__ __forceinline__ bool jstring(JRd& r, JTok& t) {
    r.pos++;
    t.kind = J_STR;
    t.off = r.pos;
    t.esc = false;
    for (;;) {
        if (r.pos >= r.end) return false;
        {  // the plain bytes of the 16-byte window in one step
            const uint32_t k = r.plain_run(r.pos);
            if (k >= r.end - r.pos) {
                r.pos = r.end;  // (the document ends inside the string)
                return false;
            }
            r.pos += k;
            if (r.pos - r.wb == 16) continue;  // (no special byte in the window)
        }
        const uint32_t c = r.at(r.pos);
        if (c == '"') break;
        if (c < 0x20) return false;
        if (c != '\\') {
            r.pos++;
            continue;
        }
        t.esc = true;
        if (++r.pos >= r.end) return false;
        const uint32_t e = r.at(r.pos++);
        if (e == 'u') {
            uint32_t c1;
            if (!hex4(r, c1)) return false;
            if (c1 >= 0xD800 && c1 < 0xDC00 && r.pos + 6 <= r.end && r.at(r.pos) == '\\' && r.at(r.pos + 1) == 'u') {
                r.pos += 2;
                uint32_t c2;
                if (!hex4(r, c2) || c2 < 0xDC00 || c2 >= 0xE000) return false;
            }
        } else if (!(e == '"' || e == '\\' || e == '/' || e == 'b' || e == 'f' || e == 'n' || e == 'r' || e == 't')) {
            return false;
        }
    }
    t.len = (uint32_t)(r.pos - t.off);
    t.nz = t.len > 0;  // an escape decodes to at least one byte
    r.pos++;
    return true;
}

// Handler interface: key(d, tok) - a key of the object at depth d; begin(d, arr,
// parent_arr) / end(d, arr, nz) - a container at depth d; scalar(d, tok,
// parent_arr).  Returns false on malformed JSON.  d0 > 0: one value at depth d0
// starting at r.pos (a member the handler deferred), parsed up to its end.
template <class H>
__device__ bool jparse(JRd& r, H& h, int d0 = 0) {
    uint64_t arr = 0, nzm = 0;  // depth 0..63: the container is an array / holds a non-zero value
    bool arr64 = false, nz64 = false;
    auto is_arr = [&](int d) { return d < 64 ? ((arr >> d) & 1) != 0 : arr64; };
    auto set_nz = [&](int d) {
        if (d < 64) nzm |= 1ull << d;
        else nz64 = true;
    };
    auto ws = [&]() {
        for (;;) {
            const int c = r.peek();
            if (c != ' ' && c != '\t' && c != '\n' && c != '\r') return;
            r.pos++;
        }
    };
    int d = d0 - 1;  // the innermost open container
    int state = 0;  // 0: a value; 1: after a value; 2: a key
    for (;;) {
        ws();
        const int c = r.peek();
        if (state == 0) {
            const int vd = d + 1;
            if (vd > 64) return false;
            const bool pa = d >= 0 && is_arr(d);
            if (pa) set_nz(d);  // an array with an element is not zero
            if (c == '{' || c == '[') {
                r.pos++;
                const bool a = c == '[';
                if (vd < 64) {
                    arr = a ? arr | (1ull << vd) : arr & ~(1ull << vd);
                    nzm &= ~(1ull << vd);
                } else {
                    arr64 = a, nz64 = false;
                }
                d = vd;
                h.begin(d, a, pa);
                ws();
                if (r.peek() == (a ? ']' : '}')) {
                    r.pos++;
                    h.end(d, a, false);
                    d--;
                    state = 1;
                } else {
                    state = a ? 0 : 2;
                }
                continue;
            }
            JTok t;
            if (c == '"') {
                if (!jstring(r, t)) return false;
            } else if (c == 't' || c == 'f' || c == 'n') {
                const char* w = c == 't' ? "true" : c == 'f' ? "false" : "null";
                const uint32_t n = c == 'f' ? 5 : 4;
                if (r.pos + n > r.end) return false;
                for (uint32_t k = 0; k < n; k++)
                    if (r.at(r.pos + k) != (uint8_t)w[k]) return false;
                t.off = r.pos, t.len = n, t.esc = false;
                t.kind = c == 't' ? J_TRUE : c == 'f' ? J_FALSE : J_NULL;
                t.nz = c == 't';
                r.pos += n;
            } else {  // codec.cpp num(): '-'? then any run of [0-9.eE+-]
                const jpos s = r.pos;
                if (c == '-') r.pos++;
                for (;;) {
                    const int x = r.peek();
                    if ((x >= '0' && x <= '9') || x == '.' || x == 'e' || x == 'E' || x == '+' || x == '-') r.pos++;
                    else break;
                }
                if (r.pos == s) return false;
                t.off = s, t.len = (uint32_t)(r.pos - s), t.kind = J_NUM, t.esc = false;
                t.nz = !(t.len == 1 && r.at(s) == '0');
            }
            if (t.nz && d >= 0) set_nz(d);
            h.scalar(vd, t, pa);
            state = 1;
            continue;
        }
        if (state == 1) {
            if (d < d0) return d0 ? true : c == -1;  // only whitespace after the document's value
            const bool a = is_arr(d);
            if (c == ',') {
                r.pos++;
                state = a ? 0 : 2;
            } else if (c == (a ? ']' : '}')) {
                r.pos++;
                const bool nz = d < 64 ? ((nzm >> d) & 1) != 0 : nz64;
                h.end(d, a, nz);
                d--;
                if (nz && d >= 0) set_nz(d);
            } else {
                return false;
            }
            continue;
        }
        // state 2: a key, ':'
        if (c != '"') return false;
        JTok k;
        if (!jstring(r, k)) return false;
        ws();
        if (r.peek() != ':') return false;
        r.pos++;
        h.key(d, k);
        state = 0;
    }
}

// RFC3339 "YYYY-MM-DDTHH:MM:SSZ" -> unix seconds (codec.cpp parse_time)
__device__ bool jtime(JRd& r, jpos off, uint32_t len, int64_t* out) {
    if (len != 20) return false;
    uint32_t b[20];
    for (int k = 0; k < 20; k++) b[k] = r.at(off + k);
    if (b[4] != '-' || b[7] != '-' || b[10] != 'T' || b[13] != ':' || b[16] != ':' || b[19] != 'Z') return false;
    auto dg = [&](int a, int n, int* v) {
        *v = 0;
        for (int k = a; k < a + n; k++) {
            if (b[k] < '0' || b[k] > '9') return false;
            *v = *v * 10 + (int)(b[k] - '0');
        }
        return true;
    };
    int Y, M, D, hh, mm, ss;
    if (!dg(0, 4, &Y) || !dg(5, 2, &M) || !dg(8, 2, &D) || !dg(11, 2, &hh) || !dg(14, 2, &mm) || !dg(17, 2, &ss))
        return false;
    if (M < 1 || M > 12 || D < 1 || D > 31 || hh > 23 || mm > 59 || ss > 59) return false;
    // a real calendar date: the month's length, February by the Gregorian leap rule
    // (codec.cpp parse_time: keep in step)
    const bool leap = Y % 4 == 0 && (Y % 100 != 0 || Y % 400 == 0);
    if (D > (M == 2 ? (leap ? 29 : 28) : (M == 4 || M == 6 || M == 9 || M == 11 ? 30 : 31))) return false;
    const int y = Y - (M <= 2);
    const int era = (y >= 0 ? y : y - 399) / 400;
    const int yoe = y - era * 400;
    const int doy = (153 * (M + (M > 2 ? -3 : 9)) + 2) / 5 + D - 1;
    const int doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
    const int64_t days = (int64_t)era * 146097 + doe - 719468;
    *out = days * 86400 + hh * 3600 + mm * 60 + ss;
    return true;
}

// ---------------------------------------------------------------------------
// the pod document (kwok_decode_pod)
// ---------------------------------------------------------------------------
// scan contexts: what a value at a position of the document means
enum : uint8_t {
    X_NONE = 0, X_ROOT, X_META, X_SPEC, X_STATUS,
    X_NAME, X_NS, X_CT, X_DT, X_FIN, X_ANN, X_LAB, X_ANNV, X_LABV,
    X_NODENAME, X_CONTS, X_INITS, X_GATES, X_CONT, X_INIT, X_GATE, X_CNAME, X_CIMAGE, X_INAME, X_IIMAGE, X_GTYPE,
    X_PHASE, X_HOSTIP, X_PODIP, X_STT, X_CONDS, X_COND, X_CTYPE, X_CSTAT, X_CLTT,
    X_CST, X_ICST, X_CSE, X_ICSE, X_SIMAGE, X_SNAME, X_READY, X_STATE, X_ISTATE, X_RUN, X_TERM,
    X_TS_ST, X_TS_REASON, X_ZV,
};
constexpr int XD = 8;  // contexts kept for depths 0..7 (deeper values are opaque: only their zero-ness counts)
constexpr uint32_t MAXC = KWOK_DOC_MAX_CONTAINERS, MAXG = KWOK_DOC_MAX_GATES;

struct Span {
    uint32_t off, len;
};

struct SelState {  // one selector over one label map: the last value per requirement key (labels.Set)
    uint32_t has, in;  // bit r: the key is present / its value is one of the requirement's values
};

struct PodScan {
    JRd* r;
    const JsonCfg* cfg;
    uint64_t cx = 0;      // context per depth (8 bits each)
    uint8_t next = X_NONE;  // the context of the value a key announced
    int err = 0;          // KWOK_EDOMAIN
    bool host = false;    // JSON_HOST
    bool root_obj = false;
    // first occurrences (codec.cpp JV::get returns the first key)
    uint32_t seen_root = 0, seen_meta = 0, seen_spec = 0, seen_status = 0;
    bool meta_done = false, spec_done = false, meta_obj = false, spec_obj = false;
    bool st_defer = false, pass2 = false;  // a status read before metadata / spec: scanned again at the end
    jpos st_pos = 0;                       // its '{'
    // metadata
    Span name{0, 0}, ns{0, 0};
    bool ct_ok = false;
    jpos ct_off = 0;
    int64_t creation = 0;
    uint8_t flags = 0, phase = 0;
    uint32_t n_ann = 0, n_lab = 0;
    SelState dis_ann{0, 0}, dis_lab{0, 0};
    uint32_t key_match = 0;  // the requirements whose key the current label entry has
    // spec
    Span node{0, 0};
    uint32_t n_cont = 0, n_init = 0, n_gates = 0;
    Span cname[MAXC], cimage[MAXC], iname[MAXC], iimage[MAXC], gate[MAXG];
    uint32_t elem_seen = 0;  // first name / image of the current container element
    // status
    bool has_status = false;
    Span hip{0, 0}, pip{0, 0};
    bool stt_ok = false;
    uint32_t cond_hit = 0, cond_ok = 0;  // per wanted condition type (3 + gates)
    uint32_t ce_seen = 0;                // the current condition element's type / status / ltt
    Span ctype{0, 0};
    bool ctype_set = false, cstat_ok = false, cltt_ok = false;
    bool cst_seen = false, icst_seen = false, cst_ok = true, icst_ok = true;
    int list = 0;                        // the open container-status list: 0 cst, 1 icst
    uint32_t lst_count = 0, k = 0;       // its elements; the current element
    uint32_t e_seen = 0, s_seen = 0, r_seen = 0;  // element / state / running (terminated) keys present

    __device__ uint8_t ctx(int d) const { return d < XD ? (uint8_t)(cx >> (8 * d)) : X_NONE; }
    __device__ void set_ctx(int d, uint8_t c) {
        if (d < XD) cx = (cx & ~(0xFFull << (8 * d))) | ((uint64_t)c << (8 * d));
    }
    __device__ void miss() { (list ? icst_ok : cst_ok) = false; }
    __device__ uint8_t first(uint32_t& seen, int bit, uint8_t c) {
        if (seen & (1u << bit)) return X_NONE;
        seen |= 1u << bit;
        return c;
    }
    // the value's context: the element context of an array parent, else what its key announced
    __device__ uint8_t value_ctx(int d, bool pa) {
        if (d == 0) return X_ROOT;
        if (!pa) return next;
        switch (ctx(d - 1)) {
            case X_CONTS: return X_CONT;
            case X_INITS: return X_INIT;
            case X_GATES: return X_GATE;
            case X_CONDS: return X_COND;
            case X_CST: return X_CSE;
            case X_ICST: return X_ICSE;
            case X_FIN: return X_NONE;
            default: return X_NONE;
        }
    }
    // a key the scan routes on must be compared as decoded text: escaped -> host
    __device__ bool k_is(const JTok& t, const char* s, uint32_t n) {
        if (t.len != n) return false;
        for (uint32_t q = 0; q < n; q++)
            if (r->at(t.off + q) != (uint8_t)s[q]) return false;
        return true;
    }
#define KIS(lit) k_is(t, lit, sizeof(lit) - 1)

    __device__ void key(int d, const JTok& t) {
        const uint8_t c = ctx(d);
        next = X_NONE;
        if (c == X_NONE || c == X_ZV) return;
        if (c == X_ANN || c == X_LAB) {  // a label / annotation entry
            (c == X_ANN ? n_ann : n_lab)++;
            next = c == X_ANN ? X_ANNV : X_LABV;
            key_match = 0;
            const JsonSel& S = c == X_ANN ? cfg->dis_ann : cfg->dis_lab;
            if (!S.set || !S.nreq) return;
            if (t.esc) {
                host = true;
                return;
            }
            for (uint32_t q = 0; q < S.nreq; q++)
                if (bytes_eq(*r, t.off, t.len, cfg->bytes + S.key_off[q], S.key_len[q])) key_match |= 1u << q;
            return;
        }
        if (t.esc) {  // a routed key whose decoded text the scan does not compare
            if (c == X_ROOT || c == X_META || c == X_SPEC || c == X_STATUS || c == X_CONT || c == X_INIT ||
                c == X_GATE || c == X_COND || c == X_CSE || c == X_ICSE || c == X_STATE || c == X_ISTATE ||
                c == X_RUN || c == X_TERM)
                host = true;
            return;
        }
        switch (c) {
            case X_ROOT:
                if (KIS("metadata")) next = first(seen_root, 0, X_META);
                else if (KIS("spec")) next = first(seen_root, 1, X_SPEC);
                else if (KIS("status")) next = first(seen_root, 2, X_STATUS);
                break;
            case X_META:
                if (KIS("name")) next = first(seen_meta, 0, X_NAME);
                else if (KIS("namespace")) next = first(seen_meta, 1, X_NS);
                else if (KIS("creationTimestamp")) next = first(seen_meta, 2, X_CT);
                else if (KIS("annotations")) next = first(seen_meta, 3, X_ANN);
                else if (KIS("labels")) next = first(seen_meta, 4, X_LAB);
                else if (KIS("deletionTimestamp")) next = first(seen_meta, 5, X_DT);
                else if (KIS("finalizers")) next = first(seen_meta, 6, X_FIN);
                break;
            case X_SPEC:
                if (KIS("nodeName")) next = first(seen_spec, 0, X_NODENAME);
                else if (KIS("containers")) next = first(seen_spec, 1, X_CONTS);
                else if (KIS("initContainers")) next = first(seen_spec, 2, X_INITS);
                else if (KIS("readinessGates")) next = first(seen_spec, 3, X_GATES);
                break;
            case X_CONT:
            case X_INIT:
                if (KIS("name")) next = first(elem_seen, 0, c == X_CONT ? X_CNAME : X_INAME);
                else if (KIS("image")) next = first(elem_seen, 1, c == X_CONT ? X_CIMAGE : X_IIMAGE);
                break;
            case X_GATE:
                if (KIS("conditionType")) next = first(elem_seen, 0, X_GTYPE);
                break;
            case X_STATUS:
                if (KIS("phase")) next = first(seen_status, 0, X_PHASE);
                else if (KIS("hostIP")) next = first(seen_status, 1, X_HOSTIP);
                else if (KIS("podIP")) next = first(seen_status, 2, X_PODIP);
                else if (KIS("conditions")) next = first(seen_status, 3, X_CONDS);
                else if (KIS("containerStatuses")) next = first(seen_status, 4, X_CST);
                else if (KIS("initContainerStatuses")) next = first(seen_status, 5, X_ICST);
                else if (KIS("startTime")) next = first(seen_status, 6, X_STT);
                break;
            case X_COND:
                if (KIS("type")) next = first(ce_seen, 0, X_CTYPE);
                else if (KIS("status")) next = first(ce_seen, 1, X_CSTAT);
                else if (KIS("lastTransitionTime")) next = first(ce_seen, 2, X_CLTT);
                break;
            // norm_equal(have, want): every occurrence of a key is compared; a key the
            // rendered status lacks must hold a zero value
            case X_CSE:
            case X_ICSE:
                if (KIS("image")) next = X_SIMAGE, e_seen |= 1;
                else if (KIS("name")) next = X_SNAME, e_seen |= 2;
                else if (KIS("ready")) next = X_READY, e_seen |= 4;
                else if (KIS("state")) next = c == X_CSE ? X_STATE : X_ISTATE, e_seen |= 8;
                else next = X_ZV;  // restartCount (rendered 0) and anything else
                break;
            case X_STATE:
                if (KIS("running")) next = X_RUN, s_seen |= 1;
                else next = X_ZV;
                break;
            case X_ISTATE:
                if (KIS("terminated")) next = X_TERM, s_seen |= 1;
                else next = X_ZV;
                break;
            case X_RUN:
                if (KIS("startedAt")) next = X_TS_ST, r_seen |= 1;
                else next = X_ZV;
                break;
            case X_TERM:
                if (KIS("finishedAt")) next = X_TS_ST, r_seen |= 2;
                else if (KIS("startedAt")) next = X_TS_ST, r_seen |= 1;
                else if (KIS("reason")) next = X_TS_REASON, r_seen |= 4;
                else next = X_ZV;  // exitCode (rendered 0) and anything else
                break;
            default:
                break;
        }
    }
#undef KIS

    // a referenced string (codec.cpp ref): null / absent -> empty; otherwise an unescaped string
    __device__ void ref(const JTok& t, Span& out) {
        if (t.kind == J_NULL) return;
        if (t.kind != J_STR || t.esc) {
            err = KWOK_EDOMAIN;
            return;
        }
        if (t.len) out = Span{(uint32_t)t.off, t.len};
    }
    // a compared string equal to the creation time (decoded text: escaped -> host)
    __device__ bool is_ct(const JTok& t) {
        if (t.kind != J_STR) return false;
        if (t.esc) {
            host = true;
            return false;
        }
        return ct_ok && t.len == 20 && span_eq(*r, t.off, ct_off, 20);
    }
    // a container-status field compared with the rendered string w (norm_equal)
    __device__ void cmp_str(const JTok& t, Span w) {
        if (!t.nz) {
            if (w.len) miss();
            return;
        }
        if (t.kind != J_STR) {
            miss();
            return;
        }
        if (t.esc) {
            host = true;
            return;
        }
        if (t.len != w.len || !span_eq(*r, t.off, w.off, w.len)) miss();
    }
    __device__ Span want_field(bool image) const {
        if (list == 0) return k < n_cont ? (image ? cimage[k] : cname[k]) : Span{0, 0};
        return k < n_init ? (image ? iimage[k] : iname[k]) : Span{0, 0};
    }

    __device__ void scalar(int d, const JTok& t, bool pa) {
        const uint8_t c = value_ctx(d, pa);
        if (d == 0) return;  // not an object: rejected at the end
        switch (c) {
            case X_META:
            case X_SPEC:
                err = KWOK_EDOMAIN;  // metadata / spec must be objects
                break;
            case X_STATUS:
                if (t.kind != J_NULL) err = KWOK_EDOMAIN;  // status: an object or null
                break;
            case X_NAME: ref(t, name); break;
            case X_NS: ref(t, ns); break;
            case X_NODENAME: ref(t, node); break;
            case X_HOSTIP: ref(t, hip); break;
            case X_PODIP: ref(t, pip); break;
            case X_CNAME: if (n_cont) ref(t, cname[n_cont - 1]); break;
            case X_CIMAGE: if (n_cont) ref(t, cimage[n_cont - 1]); break;
            case X_INAME: if (n_init) ref(t, iname[n_init - 1]); break;
            case X_IIMAGE: if (n_init) ref(t, iimage[n_init - 1]); break;
            case X_GTYPE: if (n_gates) ref(t, gate[n_gates - 1]); break;
            case X_CT:
                if (t.kind != J_STR) err = KWOK_EDOMAIN;
                else if (t.esc) host = true;
                else if (!jtime(*r, t.off, t.len, &creation)) err = KWOK_EDOMAIN;
                else ct_ok = true, ct_off = t.off;
                break;
            case X_DT:
                if (t.kind != J_NULL) flags |= KWOK_POD_DELETING;
                break;
            case X_ANN:
            case X_LAB:
                if (t.kind != J_NULL) err = KWOK_EDOMAIN;  // a label map: an object or null
                break;
            case X_ANNV:
            case X_LABV: {
                if (t.kind != J_STR) {
                    err = KWOK_EDOMAIN;  // label / annotation values are strings
                    break;
                }
                const bool ann = c == X_ANNV;
                const JsonSel& S = ann ? cfg->dis_ann : cfg->dis_lab;
                SelState& st = ann ? dis_ann : dis_lab;
                if (!key_match) break;
                if (t.esc) {
                    host = true;
                    break;
                }
                for (uint32_t q = 0; q < S.nreq; q++) {  // the last entry of a key wins (a Go map)
                    if (!((key_match >> q) & 1)) continue;
                    bool in = false;
                    for (uint32_t v = 0; v < S.val_n[q]; v++) {
                        const uint32_t vi = S.val_first[q] + v;
                        in |= bytes_eq(*r, t.off, t.len, cfg->bytes + S.val_off[vi], S.val_len[vi]);
                    }
                    st.has |= 1u << q;
                    st.in = in ? st.in | (1u << q) : st.in & ~(1u << q);
                }
                break;
            }
            case X_CONTS:
            case X_INITS:
                if (t.kind != J_NULL) err = KWOK_EDOMAIN;  // a list or null
                break;
            case X_CONT:
            case X_INIT:
            case X_GATE:
                err = KWOK_EDOMAIN;  // list elements are objects
                break;
            case X_PHASE:
                if (t.kind == J_STR) {
                    if (t.esc) {
                        host = true;
                        break;
                    }
                    if (!t.len) phase = KWOK_PHASE_NONE;
                    else if (lit_eq(*r, t.off, t.len, "Pending")) phase = KWOK_PHASE_PENDING;
                    else if (lit_eq(*r, t.off, t.len, "Running")) phase = KWOK_PHASE_RUNNING;
                    else if (lit_eq(*r, t.off, t.len, "Succeeded")) phase = KWOK_PHASE_SUCCEEDED;
                    else if (lit_eq(*r, t.off, t.len, "Failed")) phase = KWOK_PHASE_FAILED;
                    else if (lit_eq(*r, t.off, t.len, "Unknown")) phase = KWOK_PHASE_UNKNOWN;
                    else phase = KWOK_PHASE_OTHER;
                }
                break;
            case X_STT: stt_ok = is_ct(t); break;
            case X_CTYPE:
                if (t.kind == J_STR) {
                    if (t.esc) host = true;
                    else ctype = Span{(uint32_t)t.off, t.len}, ctype_set = true;
                }
                break;
            case X_CSTAT:
                if (t.kind == J_STR) {
                    if (t.esc) host = true;
                    else cstat_ok = lit_eq(*r, t.off, t.len, "True");
                }
                break;
            case X_CLTT: cltt_ok = is_ct(t); break;
            case X_CST:
            case X_ICST:  // not a list: equal to the rendered list only if both are zero
                list = c == X_ICST;
                (c == X_CST ? cst_seen : icst_seen) = true;
                if (t.nz || (c == X_CST ? n_cont : n_init)) miss();
                break;
            case X_CSE:
            case X_ICSE:  // a scalar element: the rendered element is an object
                list = c == X_ICSE;
                lst_count++;
                miss();
                break;
            case X_SIMAGE: cmp_str(t, want_field(true)); break;
            case X_SNAME: cmp_str(t, want_field(false)); break;
            case X_READY:
                if (t.kind != J_TRUE) miss();
                break;
            case X_STATE:
            case X_ISTATE:
            case X_RUN:
            case X_TERM:
                miss();  // the rendered value is an object
                break;
            case X_TS_ST:
                if (!is_ct(t)) miss();
                break;
            case X_TS_REASON:
                if (t.kind != J_STR) miss();
                else if (t.esc) host = true;
                else if (!lit_eq(*r, t.off, t.len, "Completed")) miss();
                break;
            case X_ZV:
                if (t.nz) miss();
                break;
            default:
                break;
        }
    }

    __device__ void begin(int d, bool a, bool pa) {
        const uint8_t c = value_ctx(d, pa);
        uint8_t mine = X_NONE;  // the context of this container's own members
        if (d == 0) {
            root_obj = !a;
            set_ctx(0, a ? X_NONE : X_ROOT);
            return;
        }
        switch (c) {
            case X_META: if (a) err = KWOK_EDOMAIN; else mine = X_META, meta_obj = true; break;
            case X_SPEC: if (a) err = KWOK_EDOMAIN; else mine = X_SPEC, spec_obj = true; break;
            case X_STATUS:
                if (a) {
                    err = KWOK_EDOMAIN;
                    break;
                }
                // its no-op test needs the creation time, containers and gates: before
                // them, skipped (X_NONE) and scanned by the second pass
                if (!pass2 && (!meta_done || !spec_done || !ct_ok)) {
                    st_defer = true;
                    st_pos = r->pos - 1;
                    break;
                }
                has_status = true;
                mine = X_STATUS;
                break;
            case X_NAME: case X_NS: case X_NODENAME: case X_HOSTIP: case X_PODIP:
            case X_CNAME: case X_CIMAGE: case X_INAME: case X_IIMAGE: case X_GTYPE:
            case X_CT: case X_ANNV: case X_LABV:
                err = KWOK_EDOMAIN;  // strings
                break;
            case X_DT: flags |= KWOK_POD_DELETING; break;
            case X_FIN: if (a) mine = X_FIN; break;
            case X_ANN: case X_LAB: if (a) err = KWOK_EDOMAIN; else mine = c; break;
            case X_CONTS: case X_INITS: if (!a) err = KWOK_EDOMAIN; else mine = c; break;
            case X_GATES: if (a) mine = X_GATES; break;  // not a list: ignored
            case X_CONT:
            case X_INIT: {
                if (a) {
                    err = KWOK_EDOMAIN;
                    break;
                }
                uint32_t& n = c == X_CONT ? n_cont : n_init;
                if (n >= MAXC) {
                    err = KWOK_EDOMAIN;  // too many containers
                    break;
                }
                (c == X_CONT ? cname : iname)[n] = Span{0, 0};
                (c == X_CONT ? cimage : iimage)[n] = Span{0, 0};
                n++;
                elem_seen = 0;
                mine = c;
                break;
            }
            case X_GATE:
                if (a) {
                    err = KWOK_EDOMAIN;
                    break;
                }
                if (n_gates >= MAXG) {
                    err = KWOK_EDOMAIN;
                    break;
                }
                gate[n_gates++] = Span{0, 0};
                elem_seen = 0;
                mine = X_GATE;
                break;
            case X_CONDS: if (a) mine = X_CONDS; break;
            case X_COND:
                if (!a) {
                    ce_seen = 0, ctype_set = cstat_ok = cltt_ok = false;
                    mine = X_COND;
                }
                break;
            case X_CST:
            case X_ICST:  // a list; any other container must be zero (and no container rendered)
                list = c == X_ICST;
                (c == X_CST ? cst_seen : icst_seen) = true;
                lst_count = 0;
                mine = c;
                break;
            case X_CSE:
            case X_ICSE:
                k = lst_count++;
                if (a) {
                    miss();  // the rendered element is an object
                } else {
                    e_seen = 0;
                    mine = c;
                }
                break;
            case X_STATE:
            case X_ISTATE:
                if (a) miss();
                else s_seen = 0, mine = c;
                break;
            case X_RUN:
            case X_TERM:
                if (a) miss();
                else r_seen = 0, mine = c;
                break;
            case X_SIMAGE:
            case X_SNAME:
            case X_READY:
            case X_TS_ST:
            case X_TS_REASON:
            case X_ZV:
                mine = c;  // a compared value that is a container: decided at its end, from its zero-ness
                break;
            default:
                break;
        }
        set_ctx(d, mine);
        if (d >= XD - 1 && mine != X_NONE && mine != X_ZV) host = true;  // (never at the depths a pod uses)
    }

    __device__ void end(int d, bool a, bool nz) {
        const uint8_t c = ctx(d);
        if (d == 1) {
            if (c == X_META) meta_done = true;
            if (c == X_SPEC) spec_done = true;
            if (c == X_STATUS && nz) flags |= KWOK_POD_STATUS_NONEMPTY;
        }
        switch (c) {
            case X_FIN:
                if (nz) flags |= KWOK_POD_HAS_FINALIZERS;  // a list with an element
                break;
            case X_COND:
                if (ctype_set) {
                    const uint32_t nw = 3 + n_gates;
                    for (uint32_t q = 0; q < nw; q++) {
                        if ((cond_hit >> q) & 1) continue;
                        bool m;
                        if (q == 0) m = lit_eq(*r, ctype.off, ctype.len, "Initialized");
                        else if (q == 1) m = lit_eq(*r, ctype.off, ctype.len, "Ready");
                        else if (q == 2) m = lit_eq(*r, ctype.off, ctype.len, "ContainersReady");
                        else m = gate[q - 3].len == ctype.len && span_eq(*r, gate[q - 3].off, ctype.off, ctype.len);
                        if (!m) continue;
                        cond_hit |= 1u << q;
                        if (cstat_ok && cltt_ok) cond_ok |= 1u << q;
                    }
                }
                break;
            case X_CST:
            case X_ICST:
                if (a ? lst_count != (c == X_CST ? n_cont : n_init) : (nz || (c == X_CST ? n_cont : n_init))) miss();
                break;
            case X_CSE:
            case X_ICSE: {
                const uint32_t n = c == X_CSE ? n_cont : n_init;
                if (k >= n) {
                    miss();
                    break;
                }
                uint32_t need = 4 | 8;  // ready, state
                if (want_field(true).len) need |= 1;
                if (want_field(false).len) need |= 2;
                if ((e_seen & need) != need) miss();
                break;
            }
            case X_STATE:
            case X_ISTATE:
                if (!(s_seen & 1)) miss();
                break;
            case X_RUN:
                if (!(r_seen & 1)) miss();
                break;
            case X_TERM:
                if ((r_seen & 7) != 7) miss();
                break;
            case X_SIMAGE:
            case X_SNAME:  // a container: equal to the rendered string only if both are zero
                if (nz || want_field(c == X_SIMAGE).len) miss();
                break;
            case X_READY:
            case X_TS_ST:
            case X_TS_REASON:
                miss();  // the rendered value is a non-zero scalar
                break;
            case X_ZV:
                if (nz) miss();
                break;
            default:
                break;
        }
    }

    __device__ bool matches(const JsonSel& S, const SelState& st) const {
        for (uint32_t q = 0; q < S.nreq; q++) {
            const bool has = (st.has >> q) & 1, in = (st.in >> q) & 1;
            switch (S.op[q]) {
                case JREQ_IN: if (!in) return false; break;
                case JREQ_NOTIN: if (in) return false; break;
                case JREQ_EXISTS: if (!has) return false; break;
                default: if (has) return false; break;
            }
        }
        return true;
    }
};

// FNV-1a 64 of the pod spec the engine interns (kwok_register_pod_spec): each
// container's name 0x1F image 0x1E, 0x1D, the init containers alike, 0x1D, each
// readiness gate 0x1E (engine.cpp json_spec_key is the same function)
// The walk over those bytes (engine.cpp json_spec_canon writes the same string)
template <class F>
__device__ __forceinline__ void spec_walk(JRd& r, const PodScan& p, F&& byte) {
    auto str = [&](Span s) {
        for (uint32_t q = 0; q < s.len; q++) byte(r.at(s.off + q));
    };
    for (uint32_t q = 0; q < p.n_cont; q++) str(p.cname[q]), byte(0x1F), str(p.cimage[q]), byte(0x1E);
    byte(0x1D);
    for (uint32_t q = 0; q < p.n_init; q++) str(p.iname[q]), byte(0x1F), str(p.iimage[q]), byte(0x1E);
    byte(0x1D);
    for (uint32_t q = 0; q < p.n_gates; q++) str(p.gate[q]), byte(0x1E);
}
// the key (FNV-1a 64) and a second, independent hash of the same bytes
__device__ void spec_keys(JRd& r, const PodScan& p, uint64_t& k1, uint64_t& k2) {
    uint64_t h = 0xCBF29CE484222325ull, g = 0x243F6A8885A308D3ull;
    spec_walk(r, p, [&](uint32_t b) {
        h = (h ^ b) * 0x100000001B3ull;
        g = (g + b + 1) * 0x9E3779B97F4A7C15ull;
        g ^= g >> 29;
    });
    k1 = h, k2 = g;
}
// the document's spec is exactly the registered one (a key hit is not proof)
__device__ bool spec_equal(JRd& r, const PodScan& p, const uint8_t* canon, uint2 ref) {
    uint32_t k = 0;
    bool eq = true;
    spec_walk(r, p, [&](uint32_t b) {
        eq = eq && k < ref.y && canon[ref.x + k] == (uint8_t)b;
        k++;
    });
    return eq && k == ref.y;
}

}  // namespace

// A batch of fewer documents than the chip has CUs x 4 waves goes one wave per block:
// each scanning wave reads 64 documents' 16-byte windows (64 lines per load), so
// waves spread over all CUs share no CU's SIMDs (a 10k-document node batch: 0.82 ms
// in 40 blocks of 4 waves, 0.68 ms in 157 blocks of one)
__host__ __device__ inline uint32_t json_block(uint32_t n) { return n < 256u * 64u * 4u ? 64u : 256u; }

// one thread per document
__global__ __launch_bounds__(256) void k_json_pods(JsonPodArgs A) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    const uint64_t off = A.doc_off[i];
    const uint32_t len = A.doc_len[i];
    kwok_pod_event ev;
    ev.op = KWOK_OP_UPSERT;
    ev.phase = 0;
    ev.flags = 0;
    ev.reserved0 = 0;
    ev.handle = -1;
    ev.spec_id = -1;
    ev.node_handle = -1;
    ev.creation_unix = 0;
    ev.node_name = ev.host_ip = ev.pod_ip = kwok_str{0, 0};
    JsonPodSide side{};
    int32_t status;
    PodScan p;
    if (off > A.arena_len || len > A.arena_len - off) {
        status = KWOK_EINVAL;  // (codec.cpp parse_doc: a span outside the arena)
    } else {
        JRd rd{A.arena, (jpos)off, (jpos)(off + len), ~0u, make_uint4(0, 0, 0, 0)};
        p.r = &rd;
        p.cfg = A.cfg;
        bool ok = !A.cfg->all_host && jparse(rd, p);
        if (ok && p.st_defer && !p.host && !p.err) {
            if (!p.meta_done || !p.spec_done || !p.ct_ok) {
                p.host = true;  // (the host decides a status it cannot test)
            } else {
                p.pass2 = true;
                p.next = X_STATUS;
                rd.pos = p.st_pos;
                ok = jparse(rd, p, 1);
            }
        }
        // (a document the scan routed past an escaped key may hold errors the host's
        // first-key lookup does not see: the host decides it, errors included)
        if (A.cfg->all_host) status = JSON_HOST;  // (selectors the device tables do not hold)
        else if (!ok || !p.root_obj) status = KWOK_EDOMAIN;
        else if (p.host) status = JSON_HOST;
        else if (p.err) status = p.err;
        else if (!p.meta_obj || !p.spec_obj || !p.ct_ok) status = KWOK_EDOMAIN;
        else status = KWOK_OK;
        if (status == KWOK_OK) {
            const JsonCfg& C = *A.cfg;
            uint8_t fl = p.flags;
            if ((C.dis_ann.set && p.n_ann && p.matches(C.dis_ann, p.dis_ann)) ||
                (C.dis_lab.set && p.n_lab && p.matches(C.dis_lab, p.dis_lab)))
                fl |= KWOK_POD_DISREGARD;
            if (p.has_status) {
                const uint32_t nw = 3 + p.n_gates, all = (nw >= 32 ? ~0u : (1u << nw) - 1u);
                const bool cst = p.cst_seen ? p.cst_ok : p.n_cont == 0;
                const bool icst = p.icst_seen ? p.icst_ok : p.n_init == 0;
                if (p.cond_hit == all && p.cond_ok == all && cst && icst && p.stt_ok) fl |= KWOK_POD_CONFORMS;
                ev.phase = p.phase;
                ev.host_ip = kwok_str{p.hip.off, p.hip.len};
                ev.pod_ip = kwok_str{p.pip.off, p.pip.len};
            }
            ev.flags = fl;
            ev.creation_unix = p.creation;
            ev.node_name = kwok_str{p.node.off, p.node.len};
            side.name_off = p.name.off, side.name_len = p.name.len;
            side.ns_off = p.ns.off, side.ns_len = p.ns.len;
            side.n_cont = (uint8_t)p.n_cont, side.n_init = (uint8_t)p.n_init, side.n_gates = (uint8_t)p.n_gates;
            spec_keys(rd, p, side.spec_key, side.spec_key2);
            side.spec_key &= A.key_mask;
        }
    }
    // the ingest form: the caller's op / handle, the registered spec (device table)
    if (A.op) {
        ev.op = A.op[i];
        ev.handle = A.handle[i];
        if (status == KWOK_OK && ev.op == KWOK_OP_UPSERT) {
            int32_t id = -1;
            uint32_t hs = 0;
            for (uint32_t q = 0, h = (uint32_t)side.spec_key & A.tab_mask; q <= A.tab_mask; q++, h = (h + 1) & A.tab_mask) {
                const uint64_t kk = A.tab_key[h];
                if (kk == side.spec_key) {
                    id = A.tab_id[h];
                    hs = h;
                    break;
                }
                if (!kk) break;
            }
            // a key hit whose strings differ from the registered spec's (FNV-1a is not
            // collision-resistant and specs come from users): the host decides it
            JRd rc{A.arena, (jpos)off, (jpos)(off + len), ~0u, make_uint4(0, 0, 0, 0)};
            if (id >= 0 && !spec_equal(rc, p, A.canon, A.tab_canon[hs])) status = JSON_SPEC_X;
            else if (id < 0) status = JSON_SPEC;
            else ev.spec_id = id;
        }
        const bool listed = status == JSON_HOST || status == JSON_SPEC || status == JSON_SPEC_X;
        if (status != KWOK_OK) ev.reserved0 = (uint8_t)(int8_t)(listed ? KWOK_EINVAL : status);
    }
    side.status = status;
    A.ev[i] = ev;
    A.side[i] = side;
    if (status == JSON_HOST || status == JSON_SPEC || status == JSON_SPEC_X) A.host_list[atomicAdd(A.n_host, 1u)] = A.base + i;
}

void launch_json_pods(const JsonPodArgs& A, hipStream_t st) {
    if (!A.n) return;
    const uint32_t bs = json_block(A.n);
    hipLaunchKernelGGL(k_json_pods, dim3((A.n + bs - 1) / bs), dim3(bs), 0, st, A);
}

// ---------------------------------------------------------------------------
// the node document (kwok_decode_node, codec.cpp): WatchNodes / ListNodes'
// routing facts (node_controller.go:206-223, 256-270) - needHeartbeat = the
// node selector (controller.go:81-98: all nodes, an annotation selector or a
// label selector), needLockNode = not disregarded (empty label maps never
// match) - and the A.5 inputs configureNode reads (node_controller.go:356-391):
// status.phase, the ten nodeInfo strings and the addresses / allocatable /
// capacity blobs.  Those blobs are re-serialised canonically by the host codec
// (`YAML . 1` echoes, node.status.tpl): a document holding a non-empty one is
// listed for the host (JSON_HOST), as is any string the scan would have to
// compare as decoded text (an escaped routed key, label key or compared value).
// kwok's own fleets create Nodes with an empty status: none of them is listed.
// With the status blob canonicaliser on (kwok_canon.h; k_json_nodes_canon and
// k_canon below) a non-empty blob lists the document for k_canon instead, which
// writes the canonical form on the device or hands the document to the host.
// ---------------------------------------------------------------------------
enum : uint8_t {
    N_NONE = 0, N_ROOT, N_META, N_STATUS, N_NAME, N_ANN, N_LAB, N_ANNV, N_LABV, N_PHASE, N_ADDR, N_ALLOC, N_CAP,
    N_INFO, N_INFOV,
};
// CANON (the status blob canonicaliser on, kwok_canon.h): a non-empty blob does not list the
// document for the host; the scan notes which blobs hold a member (ne) and the raw span of each
// value, and k_canon (below) decides the document.  Named fields, no indexed span: the scan state
// stays in registers.
template <bool CANON>
struct NodeScanT {
    JRd* r;
    const JsonCfg* cfg;
    uint32_t ne = 0;           // CANON: bit k - blob k (addresses, allocatable, capacity) holds a member
    Span b_addr{0, 0}, b_alloc{0, 0}, b_cap{0, 0};  // CANON: the blobs' raw value spans
    uint64_t cx = 0;
    uint8_t next = N_NONE;
    uint8_t info_k = 0;   // the nodeInfo key the next value belongs to
    int err = 0;          // KWOK_EDOMAIN
    bool host = false;    // JSON_HOST
    bool root_obj = false, meta_obj = false;
    bool skip_status = false;  // a Deleted event: its status is not read (node_controller.go:265-269: the name only)
    uint32_t seen_root = 0, seen_meta = 0, seen_status = 0, seen_info = 0;
    Span name{0, 0};
    uint32_t n_ann = 0, n_lab = 0;
    uint32_t km_man = 0, km_dis = 0;  // the current entry's key: requirements of the manage / disregard selector
    SelState man{0, 0}, dis_a{0, 0}, dis_l{0, 0};
    uint8_t phase = KWOK_PHASE_NONE;
    Span info[KWOK_NI_COUNT];

    __device__ uint8_t ctx(int d) const { return d < XD ? (uint8_t)(cx >> (8 * d)) : N_NONE; }
    __device__ void set_ctx(int d, uint8_t c) {
        if (d < XD) cx = (cx & ~(0xFFull << (8 * d))) | ((uint64_t)c << (8 * d));
    }
    __device__ uint8_t first(uint32_t& seen, int bit, uint8_t c) {
        if (seen & (1u << bit)) return N_NONE;
        seen |= 1u << bit;
        return c;
    }
    __device__ bool k_is(const JTok& t, const char* s, uint32_t n) {
        if (t.len != n) return false;
        for (uint32_t q = 0; q < n; q++)
            if (r->at(t.off + q) != (uint8_t)s[q]) return false;
        return true;
    }
    // the selector that decides `managed` over this label map (null: none does)
    __device__ const JsonSel* man_sel(bool ann) const {
        if (cfg->manage_all) return nullptr;
        if (cfg->man_ann.set) return ann ? &cfg->man_ann : nullptr;
        return ann ? nullptr : &cfg->man_lab;
    }
    __device__ uint32_t key_reqs(const JsonSel* S, const JTok& t) {
        uint32_t m = 0;
        if (!S || !S->set) return 0;
        for (uint32_t q = 0; q < S->nreq; q++)
            if (bytes_eq(*r, t.off, t.len, cfg->bytes + S->key_off[q], S->key_len[q])) m |= 1u << q;
        return m;
    }
    __device__ void sel_value(const JsonSel* S, SelState& st, uint32_t km, const JTok& t) {
        for (uint32_t q = 0; q < S->nreq; q++) {  // the last entry of a key wins (a Go map)
            if (!((km >> q) & 1)) continue;
            bool in = false;
            for (uint32_t v = 0; v < S->val_n[q]; v++) {
                const uint32_t vi = S->val_first[q] + v;
                in |= bytes_eq(*r, t.off, t.len, cfg->bytes + S->val_off[vi], S->val_len[vi]);
            }
            st.has |= 1u << q;
            st.in = in ? st.in | (1u << q) : st.in & ~(1u << q);
        }
    }
#define KIS(lit) k_is(t, lit, sizeof(lit) - 1)
    __device__ void key(int d, const JTok& t) {
        const uint8_t c = ctx(d);
        next = N_NONE;
        if (c == N_NONE) return;
        if (CANON && (c == N_ALLOC || c == N_CAP)) {  // a member, whatever its key: k_canon reads the blob
            ne |= c == N_ALLOC ? 2u : 4u;
            return;
        }
        if (c == N_ANN || c == N_LAB) {  // a label / annotation entry
            const bool ann = c == N_ANN;
            if (ann) n_ann++;  // (no reference picked by a condition: the scan's state stays in registers)
            else n_lab++;
            next = ann ? N_ANNV : N_LABV;
            const JsonSel* M = man_sel(ann);
            const JsonSel* D = ann ? &cfg->dis_ann : &cfg->dis_lab;
            const bool any = (M && M->set && M->nreq) || (D->set && D->nreq);
            km_man = km_dis = 0;
            if (!any) return;
            if (t.esc) {
                host = true;
                return;
            }
            km_man = key_reqs(M, t);
            km_dis = key_reqs(D, t);
            return;
        }
        if (t.esc) {  // a routed key whose decoded text the scan does not compare
            if (c == N_ROOT || c == N_META || c == N_STATUS || c == N_INFO) host = true;
            return;
        }
        switch (c) {
            case N_ROOT:
                if (KIS("metadata")) next = first(seen_root, 0, N_META);
                else if (KIS("status") && !skip_status) next = first(seen_root, 1, N_STATUS);
                break;
            case N_META:
                if (KIS("name")) next = first(seen_meta, 0, N_NAME);
                else if (KIS("annotations")) next = first(seen_meta, 1, N_ANN);
                else if (KIS("labels")) next = first(seen_meta, 2, N_LAB);
                break;
            case N_STATUS:
                if (KIS("phase")) next = first(seen_status, 0, N_PHASE);
                else if (KIS("addresses")) next = first(seen_status, 1, N_ADDR);
                else if (KIS("allocatable")) next = first(seen_status, 2, N_ALLOC);
                else if (KIS("capacity")) next = first(seen_status, 3, N_CAP);
                else if (KIS("nodeInfo")) next = first(seen_status, 4, N_INFO);
                break;
            case N_ALLOC:
            case N_CAP:
                host = true;  // a non-empty blob: its canonical form is the host codec's
                break;
            case N_INFO: {  // codec.cpp nik[], KWOK_NI_* order
#define NI(i, lit) else if (KIS(lit)) { next = first(seen_info, i, N_INFOV); info_k = i; }
                if (false) {}
                NI(0, "architecture") NI(1, "bootID") NI(2, "containerRuntimeVersion") NI(3, "kernelVersion")
                NI(4, "kubeProxyVersion") NI(5, "kubeletVersion") NI(6, "machineID") NI(7, "operatingSystem")
                NI(8, "osImage") NI(9, "systemUUID")
#undef NI
                break;
            }
            default:
                break;
        }
    }
#undef KIS
    __device__ uint8_t value_ctx(int d, bool pa) const { return d == 0 ? N_ROOT : pa ? N_NONE : next; }
    __device__ void ref(const JTok& t, Span& out) {  // codec.cpp ref
        if (t.kind == J_NULL) return;
        if (t.kind != J_STR || t.esc) {
            err = KWOK_EDOMAIN;
            return;
        }
        if (t.len) out = Span{(uint32_t)t.off, t.len};
    }
    __device__ void scalar(int d, const JTok& t, bool pa) {
        const uint8_t c = value_ctx(d, pa);
        if (d == 0) return;
        if (pa && ctx(d - 1) == N_ADDR) {  // a non-empty addresses list (canonical: the host codec's, or k_canon's)
            if (CANON) ne |= 1u;
            else host = true;
        }
        switch (c) {
            case N_META: err = KWOK_EDOMAIN; break;  // metadata must be an object (null included)
            case N_NAME: ref(t, name); break;
            case N_ANN:
            case N_LAB:
                if (t.kind != J_NULL) err = KWOK_EDOMAIN;  // a label map: an object or null
                break;
            case N_ANNV:
            case N_LABV: {
                if (t.kind != J_STR) {
                    err = KWOK_EDOMAIN;  // label / annotation values are strings
                    break;
                }
                if (!km_man && !km_dis) break;
                if (t.esc) {
                    host = true;
                    break;
                }
                const bool ann = c == N_ANNV;
                if (km_man) sel_value(man_sel(ann), man, km_man, t);
                if (km_dis) {
                    if (ann) sel_value(&cfg->dis_ann, dis_a, km_dis, t);
                    else sel_value(&cfg->dis_lab, dis_l, km_dis, t);
                }
                break;
            }
            case N_PHASE:
                if (t.kind == J_STR) {
                    if (t.esc) host = true;
                    else phase = !t.len ? KWOK_PHASE_NONE : lit_eq(*r, t.off, t.len, "Running") ? KWOK_PHASE_RUNNING
                                                                                                 : KWOK_PHASE_OTHER;
                }
                break;
            case N_ADDR:
            case N_ALLOC:
            case N_CAP:
                if (t.kind != J_NULL) err = KWOK_EDOMAIN;  // the wrong type
                break;
            case N_INFOV:  // (constant indices: an indexed span would keep the scan state in scratch)
                switch (info_k) {
                    case 0: ref(t, info[0]); break;
                    case 1: ref(t, info[1]); break;
                    case 2: ref(t, info[2]); break;
                    case 3: ref(t, info[3]); break;
                    case 4: ref(t, info[4]); break;
                    case 5: ref(t, info[5]); break;
                    case 6: ref(t, info[6]); break;
                    case 7: ref(t, info[7]); break;
                    case 8: ref(t, info[8]); break;
                    default: ref(t, info[9]); break;
                }
                break;
            default: break;
        }
    }
    __device__ void begin(int d, bool a, bool pa) {
        const uint8_t c = value_ctx(d, pa);
        uint8_t mine = N_NONE;
        if (d == 0) {
            root_obj = !a;
            set_ctx(0, a ? N_NONE : N_ROOT);
            return;
        }
        if (pa && ctx(d - 1) == N_ADDR) {
            if (CANON) ne |= 1u;
            else host = true;
        }
        switch (c) {
            case N_META: if (a) err = KWOK_EDOMAIN; else mine = N_META, meta_obj = true; break;
            case N_STATUS: if (!a) mine = N_STATUS; break;  // (a status that is no object is ignored)
            case N_NAME: case N_ANNV: case N_LABV: case N_INFOV: err = KWOK_EDOMAIN; break;  // strings
            case N_ANN: case N_LAB: if (a) err = KWOK_EDOMAIN; else mine = c; break;
            case N_ADDR: if (!a) err = KWOK_EDOMAIN; else mine = c; break;
            case N_ALLOC: case N_CAP: if (a) err = KWOK_EDOMAIN; else mine = c; break;
            case N_INFO: if (!a) mine = N_INFO; break;  // (ignored unless an object)
            default: break;
        }
        set_ctx(d, mine);
        if (CANON) {  // the value's '[' / '{' (selects of values: a store picked by a condition would index the spans)
            const uint32_t p = (uint32_t)(r->pos - 1);
            b_addr.off = mine == N_ADDR ? p : b_addr.off;
            b_alloc.off = mine == N_ALLOC ? p : b_alloc.off;
            b_cap.off = mine == N_CAP ? p : b_cap.off;
        }
    }
    // (a blob was listed at its first member; an empty one is absent.  CANON: the value ends here)
    __device__ void end(int d, bool, bool) {
        if (!CANON) return;
        const uint8_t c = ctx(d);
        const uint32_t p = (uint32_t)r->pos;
        b_addr.len = c == N_ADDR ? p - b_addr.off : b_addr.len;
        b_alloc.len = c == N_ALLOC ? p - b_alloc.off : b_alloc.len;
        b_cap.len = c == N_CAP ? p - b_cap.off : b_cap.len;
    }
    __device__ bool matches(const JsonSel& S, const SelState& st) const {
        for (uint32_t q = 0; q < S.nreq; q++) {
            const bool has = (st.has >> q) & 1, in = (st.in >> q) & 1;
            switch (S.op[q]) {
                case JREQ_IN: if (!in) return false; break;
                case JREQ_NOTIN: if (in) return false; break;
                case JREQ_EXISTS: if (!has) return false; break;
                default: if (has) return false; break;
            }
        }
        return true;
    }
};

// one thread per node document; op[i]: the caller's watch event (the record's op)
template <bool CANON>
__device__ __forceinline__ void json_node_doc(const JsonNodeArgs& A) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    const uint64_t off = A.doc_off[i];
    const uint32_t len = A.doc_len[i];
    kwok_node_event ev;
    ev.op = A.op[i];
    ev.managed = ev.lockable = 0;
    ev.phase = KWOK_PHASE_NONE;
    ev.name = ev.addresses = ev.allocatable = ev.capacity = kwok_str{0, 0};
    for (int k = 0; k < KWOK_NI_COUNT; k++) ev.node_info[k] = kwok_str{0, 0};
    int32_t status;
    NodeScanT<CANON> p;
    for (int k = 0; k < KWOK_NI_COUNT; k++) p.info[k] = Span{0, 0};
    if (off > A.arena_len || len > A.arena_len - off) {
        status = KWOK_EINVAL;  // (codec.cpp parse_doc: a span outside the arena)
    } else if (A.cfg->all_host) {
        status = JSON_HOST;
    } else {
        JRd rd{A.arena, (jpos)off, (jpos)(off + len), ~0u, make_uint4(0, 0, 0, 0)};
        p.r = &rd;
        p.cfg = A.cfg;
        p.skip_status = ev.op == KWOK_OP_DELETE;
        const bool ok = jparse(rd, p);
        // (a document the scan routed past an escaped key may hold errors the host's
        // first-key lookup does not see: the host decides it, errors included)
        if (!ok || !p.root_obj) status = KWOK_EDOMAIN;
        else if (p.host) status = JSON_HOST;
        else if (p.err) status = p.err;
        else if (!p.meta_obj || !p.name.len) status = KWOK_EDOMAIN;
        else status = KWOK_OK;
        if (status == KWOK_OK) {
            const JsonCfg& C = *A.cfg;
            ev.managed = C.manage_all ? 1 : C.man_ann.set ? (p.matches(C.man_ann, p.man) ? 1 : 0)
                                                           : (C.man_lab.set && p.matches(C.man_lab, p.man) ? 1 : 0);
            const bool disregard = (C.dis_ann.set && p.n_ann && p.matches(C.dis_ann, p.dis_a)) ||
                                   (C.dis_lab.set && p.n_lab && p.matches(C.dis_lab, p.dis_l));
            ev.lockable = disregard ? 0 : 1;
            ev.phase = p.phase;
            ev.name = kwok_str{p.name.off, p.name.len};
            for (int k = 0; k < KWOK_NI_COUNT; k++) ev.node_info[k] = kwok_str{p.info[k].off, p.info[k].len};
            if (CANON && p.ne) {  // the raw spans of the non-empty blobs: k_canon decides the document
                const uint32_t m0 = p.ne & 1u ? ~0u : 0u, m1 = p.ne & 2u ? ~0u : 0u, m2 = p.ne & 4u ? ~0u : 0u;
                ev.addresses = kwok_str{p.b_addr.off & m0, p.b_addr.len & m0};
                ev.allocatable = kwok_str{p.b_alloc.off & m1, p.b_alloc.len & m1};
                ev.capacity = kwok_str{p.b_cap.off & m2, p.b_cap.len & m2};
                A.canon_list[atomicAdd(&A.canon_ctr->n, 1u)] = A.base + i;
                atomicAdd(reinterpret_cast<unsigned long long*>(&A.canon_ctr->raw),
                          (unsigned long long)ev.addresses.len + ev.allocatable.len + ev.capacity.len);
            }
        }
    }
    if (status != KWOK_OK) ev.op = 0xFF;  // (not applied: the host completes it, or its status is the decode's)
    A.ev[i] = ev;
    A.status[i] = status;
    if (status == JSON_HOST) A.host_list[atomicAdd(A.n_host, 1u)] = A.base + i;
}
__global__ __launch_bounds__(256) void k_json_nodes(JsonNodeArgs A) { json_node_doc<false>(A); }
// ... with the canonicaliser on (A.canon_list set)
__global__ __launch_bounds__(256) void k_json_nodes_canon(JsonNodeArgs A) { json_node_doc<true>(A); }

void launch_json_nodes(const JsonNodeArgs& A, hipStream_t st) {
    if (!A.n) return;
    const uint32_t bs = json_block(A.n);
    if (A.canon_list) hipLaunchKernelGGL(k_json_nodes_canon, dim3((A.n + bs - 1) / bs), dim3(bs), 0, st, A);
    else hipLaunchKernelGGL(k_json_nodes, dim3((A.n + bs - 1) / bs), dim3(bs), 0, st, A);
}

// ---------------------------------------------------------------------------
// the node status blob canonicaliser (kwok_canon.h): what
// codec.cpp canon() writes for the addresses / allocatable / capacity values of
// the documents k_json_nodes_canon listed - members of every object in bytewise
// key order (a shorter prefix first), `,` and `:` without whitespace, scalars
// verbatim - into a compact buffer of its own, never into the arena.
//
// One lane per listed document, its blobs one after the other, each in one
// jparse pass over the value's raw span (the scanner accepted the document, so
// the grammar holds).  The device domain ("clean"): a blob is an array of
// scalars and of objects of scalars (addresses) or an object of scalars
// (allocatable, capacity) - CANON_MAX_DEPTH containers deep at the most - with
// at most CANON_MAX_MEMBERS members per object, no duplicate key, no backslash
// escape, no byte go_string would change (`<`, `>`, `&`), no byte >= 0x80, every
// number a plain_int.  Anything else marks the whole document JSON_HOST and
// appends it to the scanner's host list; nothing of it is used.
//
// The per-lane table - an object's key offsets, sorted by insertion when the
// object closes - lives in LDS, entry e of lane l at tab[e * CANON_BLOCK + l]
// (a wave's lanes at the same entry hit 64 different banks): 8 KiB per block of
// one wave, no scratch.  The object is written from the sorted offsets by
// tokenizing each member again (a second reader: the parse position stays).
// ---------------------------------------------------------------------------
constexpr uint32_t CANON_MAX_MEMBERS = 32;  // members of one object
constexpr int CANON_MAX_DEPTH = 2;          // containers, the blob's own included (addresses: the list, its objects)
constexpr uint32_t CANON_BLOCK = 64;

namespace {
__device__ __forceinline__ bool canon_plain_byte(uint32_t c) { return c < 0x80 && c != '<' && c != '>' && c != '&'; }

struct CanonScan {
    JRd* r;          // the parse
    JRd* r2;         // the writer's reader
    uint32_t* tab;   // this lane's column of the block's table
    uint8_t* out;
    uint32_t cap, w = 0;  // the blob's raw length (the canonical form is no longer), bytes written
    bool arr;        // the blob is the addresses list
    bool bad = false;
    uint32_t m = 0, elems = 0;  // members of the open object; elements of the list written

    __device__ void put(uint32_t c) {
        if (w < cap) out[w] = (uint8_t)c;
        else bad = true;
        w++;
    }
    __device__ void copy(jpos off, uint32_t len) {
        for (uint32_t k = 0; k < len; k++) put(r2->at(off + k));
    }
    __device__ bool clean_str(const JTok& t) {
        if (t.esc) return false;
        for (uint32_t k = 0; k < t.len; k++)
            if (!canon_plain_byte(r->at(t.off + k))) return false;
        return true;
    }
    __device__ bool plain_int(const JTok& t) {  // codec.cpp plain_int
        uint32_t k = r->at(t.off) == '-' ? 1 : 0;
        if (k >= t.len) return false;
        if (r->at(t.off + k) == '0' && t.len > k + 1) return false;
        for (; k < t.len; k++) {
            const uint32_t c = r->at(t.off + k);
            if (c < '0' || c > '9') return false;
        }
        return true;
    }
    // the keys at a and b (inside their quotes; clean: the closing quote ends each): < 0, 0, > 0 as
    // std::string_view compares them
    __device__ int key_cmp(jpos a, jpos b) {
        for (uint32_t k = 0;; k++) {
            const uint32_t x = r->at(a + k), y = r2->at(b + k);
            const bool xe = x == '"', ye = y == '"';
            if (xe || ye) return xe && ye ? 0 : xe ? -1 : 1;
            if (x != y) return x < y ? -1 : 1;
        }
    }
    // the object just closed: its members from the table, sorted, each tokenized again and copied
    __device__ void write_object() {
        for (uint32_t a = 1; a < m && !bad; a++) {
            const uint32_t x = tab[a * CANON_BLOCK];
            uint32_t b = a;
            while (b > 0) {
                const uint32_t y = tab[(b - 1) * CANON_BLOCK];
                const int c = key_cmp(y, x);
                if (c == 0) bad = true;  // a duplicate key
                if (c <= 0) break;
                tab[b * CANON_BLOCK] = y;
                b--;
            }
            tab[b * CANON_BLOCK] = x;
        }
        if (bad) return;
        put('{');
        for (uint32_t q = 0; q < m; q++) {
            if (q) put(',');
            JTok t;
            r2->pos = tab[q * CANON_BLOCK] - 1;
            if (!jstring(*r2, t)) {
                bad = true;
                return;
            }
            copy(t.off - 1, t.len + 2);
            put(':');
            for (;;) {  // whitespace, the colon, whitespace
                const int c = r2->peek();
                if (c != ' ' && c != '\t' && c != '\n' && c != '\r' && c != ':') break;
                r2->pos++;
            }
            if (r2->peek() == '"') {
                if (!jstring(*r2, t)) {
                    bad = true;
                    return;
                }
                copy(t.off - 1, t.len + 2);
            } else {  // a plain integer, true, false or null: up to the byte that ends it
                for (;;) {
                    const int c = r2->peek();
                    if (c < 0 || c == ',' || c == '}' || c == ' ' || c == '\t' || c == '\n' || c == '\r') break;
                    put((uint32_t)c);
                    r2->pos++;
                }
            }
        }
        put('}');
    }

    __device__ void key(int, const JTok& t) {
        if (bad) return;
        if (!clean_str(t) || m >= CANON_MAX_MEMBERS) {
            bad = true;
            return;
        }
        tab[m * CANON_BLOCK] = (uint32_t)t.off;
        m++;
    }
    __device__ void scalar(int d, const JTok& t, bool pa) {
        if (bad) return;
        if (t.kind == J_STR ? !clean_str(t) : t.kind == J_NUM && !plain_int(t)) {
            bad = true;
            return;
        }
        if (d == 1 && pa) {  // an element of the list that is no object: verbatim
            if (elems++) put(',');
            if (t.kind == J_STR) copy(t.off - 1, t.len + 2);
            else copy(t.off, t.len);
        }
    }
    __device__ void begin(int d, bool a, bool) {
        if (bad) return;
        if (d == 0) {
            if (a) put('[');
        } else if (d >= CANON_MAX_DEPTH || !arr || a) {
            bad = true;  // a container in an object, a list in the list, or deeper
            return;
        }
        m = 0;
    }
    __device__ void end(int d, bool a, bool) {
        if (bad) return;
        if (a) {
            put(']');
            return;
        }
        if (d == 1 && elems++) put(',');
        write_object();
    }
};
}  // namespace

__global__ __launch_bounds__(CANON_BLOCK) void k_canon_len(const kwok_node_event* ev, const uint32_t* list, uint32_t n, uint64_t* lens) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const kwok_node_event& x = ev[list[k]];
    lens[k] = (uint64_t)x.addresses.len + x.allocatable.len + x.capacity.len;
}

__global__ __launch_bounds__(CANON_BLOCK) void k_canon(CanonArgs A) {
    __shared__ uint32_t tab[CANON_MAX_MEMBERS * CANON_BLOCK];
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= A.n) return;
    const uint32_t i = A.list[k];
    CanonDoc* D = A.docs + k;  // (written field by field where it lies: no local array, no scratch)
    uint64_t o = A.off[k];
    bool bad = false;
    // blob j of the document: parsed and written at o; its pair (one call site of the parser)
    const kwok_str b0 = A.ev[i].addresses, b1 = A.ev[i].allocatable, b2 = A.ev[i].capacity;
    for (int j = 0; j < 3; j++) {
        const kwok_str raw{j == 0 ? b0.off : j == 1 ? b1.off : b2.off, j == 0 ? b0.len : j == 1 ? b1.len : b2.len};
        D->off[j] = o;
        D->raw[j] = raw.len;
        uint32_t len = 0;
        if (raw.len && !bad) {
            JRd rd{A.arena, (jpos)raw.off, (jpos)(raw.off + raw.len), ~0u, make_uint4(0, 0, 0, 0)};
            JRd r2 = rd;
            CanonScan h;
            h.r = &rd, h.r2 = &r2;
            h.tab = tab + threadIdx.x;
            h.out = A.out + o;
            h.cap = raw.len;
            h.arr = j == 0;
            if (!jparse(rd, h) || h.bad) bad = true;
            else len = h.w;
            o += raw.len;
        }
        D->len[j] = len;
    }
    D->doc = i;
    D->host = bad ? 1u : 0u;
    if (bad) {  // the host decides the whole document, errors included
        D->len[0] = D->len[1] = D->len[2] = 0;
        kwok_node_event ev;
        ev.op = 0xFF;
        ev.managed = ev.lockable = 0;
        ev.phase = KWOK_PHASE_NONE;
        ev.name = ev.addresses = ev.allocatable = ev.capacity = kwok_str{0, 0};
        for (int q = 0; q < KWOK_NI_COUNT; q++) ev.node_info[q] = kwok_str{0, 0};
        A.ev[i] = ev;
        A.status[i] = JSON_HOST;
        A.host_list[atomicAdd(A.n_host, 1u)] = i;
    }
}

void launch_canon_len(const kwok_node_event* ev, const uint32_t* list, uint32_t n, uint64_t* lens, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_canon_len, dim3((n + CANON_BLOCK - 1) / CANON_BLOCK), dim3(CANON_BLOCK), 0, st, ev, list, n, lens);
}
void launch_canon(const CanonArgs& A, hipStream_t st) {
    if (A.n) hipLaunchKernelGGL(k_canon, dim3((A.n + CANON_BLOCK - 1) / CANON_BLOCK), dim3(CANON_BLOCK), 0, st, A);
}

// node records of a batch gathered for the host (list[k] -> out[k]) / written back (in[k] -> list[k])
__global__ void k_node_gather(const kwok_node_event* ev, const uint32_t* list, uint32_t n, kwok_node_event* out) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) out[k] = ev[list[k]];
}
__global__ void k_node_scatter(kwok_node_event* ev, const kwok_node_event* in, const uint32_t* list, uint32_t n) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) ev[list[k]] = in[k];
}
void launch_node_gather(const kwok_node_event* ev, const uint32_t* list, uint32_t n, kwok_node_event* out, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_node_gather, dim3((n + 255) / 256), dim3(256), 0, st, ev, list, n, out);
}
void launch_node_scatter(kwok_node_event* ev, const kwok_node_event* in, const uint32_t* list, uint32_t n, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_node_scatter, dim3((n + 255) / 256), dim3(256), 0, st, ev, in, list, n);
}

}  // namespace kwok

namespace kwok {
// the listed documents' records and sides, compacted for the host (json_complete)
__global__ void k_json_gather(const kwok_pod_event* ev, const JsonPodSide* side, const uint32_t* list, uint32_t n,
                              kwok_pod_event* out_ev, JsonPodSide* out_side) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out_ev[i] = ev[list[i]];
    out_side[i] = side[list[i]];
}
// ... and the host's completed records back in place
__global__ void k_json_scatter(kwok_pod_event* ev, const kwok_pod_event* in, const uint32_t* list, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) ev[list[i]] = in[i];
}
void launch_json_gather(const kwok_pod_event* ev, const JsonPodSide* side, const uint32_t* list, uint32_t n,
                        kwok_pod_event* out_ev, JsonPodSide* out_side, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_json_gather, dim3((n + 255) / 256), dim3(256), 0, st, ev, side, list, n, out_ev, out_side);
}
void launch_json_scatter(kwok_pod_event* ev, const kwok_pod_event* in, const uint32_t* list, uint32_t n, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_json_scatter, dim3((n + 255) / 256), dim3(256), 0, st, ev, in, list, n);
}
}  // namespace kwok

// ---------------------------------------------------------------------------
// the watch stream framer (kwok_watch.h, kwok_frame_watch_gpu): a watch response
// is newline-terminated frames {"type":"MODIFIED","object":{...}}\n.
//   line split   k_frame_count: each lane loads 16 bytes, a SWAR newline test gives
//                a per-lane mask, its popcounts are reduced to one count per tile
//                (KWOK_WATCH_TILE_BYTES: 256 lanes x 16 bytes x 4 steps);
//                k_frame_scan: an exclusive scan over the tile counts, one block,
//                KWOK_WATCH_SCAN_TILES tiles per step with a carry between steps;
//                k_frame_emit: a second pass over the tile writes each newline's
//                offset at base + rank (ranks in stream order: a block scan of the
//                lanes' popcounts per step)
//   frame parse  k_frame_parse: one thread per line, jparse with a handler that
//                keeps the root's `type` and `object` and the object's own
//                metadata.uid / resourceVersion / name / namespace
// The stream buffer is padded to whole 16-byte windows past its length; a window
// is loaded only when it starts below the length, and its bytes at or past the
// length are masked out.
// ---------------------------------------------------------------------------
namespace kwok {
namespace {
constexpr uint32_t FR_THREADS = 256, FR_STEP = FR_THREADS * 16, FR_STEPS = KWOK_WATCH_TILE_BYTES / FR_STEP;
static_assert(FR_STEP * FR_STEPS == KWOK_WATCH_TILE_BYTES, "a tile is whole block steps");

// bit k set for each byte k of x that is a newline (the SWAR zero-byte test of str_special4)
__device__ __forceinline__ uint32_t nl4(uint32_t x) {
    const uint32_t y = x ^ 0x0A0A0A0Au;
    const uint32_t m = ~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y | 0x7F7F7F7Fu);
    return (((m >> 7) & 0x01010101u) * 0x01020408u) >> 24;
}
// the newline mask of the 16-byte window at off (bit k: byte off + k), 0 past the stream
__device__ __forceinline__ uint32_t nl_window(const uint8_t* s, uint64_t off, uint64_t len) {
    if (off >= len) return 0;
    const uint4 w = *reinterpret_cast<const uint4*>(s + off);
    uint32_t m = nl4(w.x) | nl4(w.y) << 4 | nl4(w.z) << 8 | nl4(w.w) << 12;
    if (len - off < 16) m &= (1u << (uint32_t)(len - off)) - 1u;
    return m;
}
// inclusive scan over the wave's 64 lanes
__device__ __forceinline__ uint32_t wave_incl(uint32_t v, uint32_t lane) {
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(v, o);
        if (lane >= o) v += t;
    }
    return v;
}

enum : uint8_t { F_NONE = 0, F_TYPE, F_OBJ, F_META, F_UID, F_RV, F_NAME, F_NS };
// S: how far the routed depths are shifted up.  0: a watch line, the object under the root's
// `object`; 1: a response body (k_resp_parse), the object IS the root - no `type` / `object` keys
template <int S>
struct FrameScanT {
    JRd* r;
    uint8_t next = F_NONE;
    bool err = false, host = false, root_obj = false;
    bool in_obj = false, in_meta = false, obj_set = false;
    uint32_t seen_root = 0, seen_obj = 0, seen_meta = 0;
    uint8_t type = KWOK_WATCH_NONE, flags = 0;
    jpos obj_pos = 0;
    uint32_t obj_len = 0;
    Span uid{0, 0}, rv{0, 0}, name{0, 0}, ns{0, 0};

    __device__ uint8_t first(uint32_t& seen, int bit, uint8_t c) {
        if (seen & (1u << bit)) return F_NONE;
        seen |= 1u << bit;
        return c;
    }
    __device__ void key(int d, const JTok& t) {
        next = F_NONE;
        const bool routed = (!S && d == 0) || (d == 1 - S && in_obj) || (d == 2 - S && in_meta);
        if (!routed) return;
        if (t.esc) {  // a routed key is compared as decoded text: the host framer decides the line
            host = true;
            return;
        }
        if (!S && d == 0) {
            if (lit_eq(*r, t.off, t.len, "type")) next = first(seen_root, 0, F_TYPE);
            else if (lit_eq(*r, t.off, t.len, "object")) next = first(seen_root, 1, F_OBJ);
        } else if (d == 1 - S) {
            if (lit_eq(*r, t.off, t.len, "metadata")) next = first(seen_obj, 0, F_META);
        } else {
            if (lit_eq(*r, t.off, t.len, "uid")) next = first(seen_meta, 0, F_UID);
            else if (lit_eq(*r, t.off, t.len, "resourceVersion")) next = first(seen_meta, 1, F_RV);
            else if (lit_eq(*r, t.off, t.len, "name")) next = first(seen_meta, 2, F_NAME);
            else if (lit_eq(*r, t.off, t.len, "namespace")) next = first(seen_meta, 3, F_NS);
        }
    }
    __device__ void scalar(int d, const JTok& t, bool pa) {
        if (pa || d == 0) return;
        if (!S && d == 1) {
            if (next == F_OBJ) err = true;  // object must be a JSON object
            if (next != F_TYPE) return;
            if (t.kind != J_STR) err = true;
            else if (t.esc) host = true;
            else if (lit_eq(*r, t.off, t.len, "ADDED")) type = KWOK_WATCH_ADDED;
            else if (lit_eq(*r, t.off, t.len, "MODIFIED")) type = KWOK_WATCH_MODIFIED;
            else if (lit_eq(*r, t.off, t.len, "DELETED")) type = KWOK_WATCH_DELETED;
            else if (lit_eq(*r, t.off, t.len, "BOOKMARK")) type = KWOK_WATCH_BOOKMARK;
            else if (lit_eq(*r, t.off, t.len, "ERROR")) type = KWOK_WATCH_ERROR;
            else err = true;  // "got invalid watch event type"
            return;
        }
        if (d != 3 - S || !in_meta || t.kind != J_STR) return;  // (a non-string value: an empty span)
        const Span s = t.len ? Span{(uint32_t)t.off, t.len} : Span{0, 0};
        switch (next) {
            case F_UID: uid = s; if (t.esc) flags |= KWOK_FRAME_ESC_UID; break;
            case F_RV: rv = s; if (t.esc) flags |= KWOK_FRAME_ESC_RV; break;
            case F_NAME: name = s; if (t.esc) flags |= KWOK_FRAME_ESC_NAME; break;
            case F_NS: ns = s; if (t.esc) flags |= KWOK_FRAME_ESC_NS; break;
            default: break;
        }
    }
    __device__ void begin(int d, bool a, bool pa) {
        if (d == 0) {
            root_obj = !a;
            if (S && !a) in_obj = obj_set = true, obj_pos = r->pos - 1;
            return;
        }
        if (pa) return;
        if (!S && d == 1) {
            if (next == F_TYPE) err = true;  // type must be a string
            if (next != F_OBJ) return;
            if (a) err = true;
            else in_obj = obj_set = true, obj_pos = r->pos - 1;
        } else if (d == 2 - S && in_obj && next == F_META && !a) {
            in_meta = true;
        }
    }
    __device__ void end(int d, bool, bool) {
        if (d == 1 - S && in_obj) in_obj = false, obj_len = (uint32_t)(r->pos - obj_pos);
        if (d == 2 - S) in_meta = false;
    }
};
using FrameScan = FrameScanT<0>;
}  // namespace

__global__ __launch_bounds__(FR_THREADS) void k_frame_count(const uint8_t* s, uint64_t len, uint32_t* tile_cnt) {
    __shared__ uint32_t wsum[FR_THREADS / 64];
    const uint64_t base = (uint64_t)blockIdx.x * KWOK_WATCH_TILE_BYTES + threadIdx.x * 16u;
    uint32_t c = 0;
    for (uint32_t q = 0; q < FR_STEPS; q++) c += __popc(nl_window(s, base + (uint64_t)q * FR_STEP, len));
    for (uint32_t o = 32; o; o >>= 1) c += __shfl_down(c, o);
    if ((threadIdx.x & 63u) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (uint32_t w = 0; w < FR_THREADS / 64; w++) t += wsum[w];
        tile_cnt[blockIdx.x] = t;
    }
}

// one block: tile_base[i] = the newlines before tile i, *total = all of them
__global__ __launch_bounds__(KWOK_WATCH_SCAN_TILES) void k_frame_scan(const uint32_t* tile_cnt, uint32_t n_tiles,
                                                                     uint32_t* tile_base, uint32_t* total) {
    constexpr uint32_t NW = KWOK_WATCH_SCAN_TILES / 64;
    static_assert(NW <= 64, "the wave totals are scanned by one wave");
    __shared__ uint32_t wtot[NW];
    __shared__ uint32_t carry_s;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t carry = 0;
    for (uint32_t c0 = 0; c0 < n_tiles; c0 += KWOK_WATCH_SCAN_TILES) {
        const uint32_t i = c0 + tid;
        const uint32_t v = i < n_tiles ? tile_cnt[i] : 0u;
        const uint32_t incl = wave_incl(v, lane);
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        if (wave == 0) {  // the wave totals -> their exclusive prefixes
            const uint32_t x = lane < NW ? wtot[lane] : 0u;
            const uint32_t xi = wave_incl(x, lane);
            if (lane < NW) wtot[lane] = xi - x;
        }
        __syncthreads();
        const uint32_t excl = carry + wtot[wave] + incl - v;
        if (i < n_tiles) tile_base[i] = excl;
        if (tid == KWOK_WATCH_SCAN_TILES - 1) carry_s = excl + v;
        __syncthreads();
        carry = carry_s;
    }
    if (tid == 0) *total = carry;
}

// ends[k] = the offset of the stream's k-th newline
__global__ __launch_bounds__(FR_THREADS) void k_frame_emit(const uint8_t* s, uint64_t len, const uint32_t* tile_base,
                                                          uint32_t* ends, uint32_t n_ends) {
    __shared__ uint32_t wtot[2][FR_THREADS / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t run = tile_base[blockIdx.x];
    for (uint32_t q = 0; q < FR_STEPS; q++) {
        const uint64_t off = (uint64_t)blockIdx.x * KWOK_WATCH_TILE_BYTES + (uint64_t)q * FR_STEP + tid * 16u;
        uint32_t m = nl_window(s, off, len);
        const uint32_t c = __popc(m);
        const uint32_t incl = wave_incl(c, lane);
        if (lane == 63) wtot[q & 1][wave] = incl;  // (two sets: a step's totals are read while the next step's are written)
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (uint32_t w = 0; w < FR_THREADS / 64; w++) {
            const uint32_t t = wtot[q & 1][w];
            if (w < wave) before += t;
            all += t;
        }
        uint32_t k = run + before + incl - c;
        while (m) {
            const uint32_t b = (uint32_t)__builtin_ctz(m);
            m &= m - 1;
            if (k < n_ends) ends[k] = (uint32_t)(off + b);
            k++;
        }
        run += all;
    }
}

// one thread per line [ends[i - 1] + 1, ends[i])
__global__ __launch_bounds__(256) void k_frame_parse(const uint8_t* s, const uint32_t* ends, uint32_t n,
                                                     kwok_watch_frame* frames, uint32_t* host_list, uint32_t* n_host) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const jpos lo = i ? ends[i - 1] + 1u : 0u, hi = ends[i];
    kwok_watch_frame f;
    f.line_off = lo;
    f.doc_off = f.doc_len = 0;
    f.type = KWOK_WATCH_NONE, f.flags = 0, f.status = KWOK_OK, f.reserved0 = 0;
    f.uid = f.resource_version = f.name = f.namespace_ = kwok_str{0, 0};
    JRd rd{s, lo, hi, ~0u, make_uint4(0, 0, 0, 0)};
    for (;;) {  // a line of only whitespace: KWOK_WATCH_NONE
        const int c = rd.peek();
        if (c != ' ' && c != '\t' && c != '\n' && c != '\r') break;
        rd.pos++;
    }
    if (rd.pos < hi) {
        FrameScan p;
        p.r = &rd;
        const bool ok = jparse(rd, p);
        if (!ok || !p.root_obj) {
            f.status = KWOK_EINVAL;
        } else if (p.host) {
            host_list[atomicAdd(n_host, 1u)] = i;  // (its frame is the host framer's)
        } else if (p.err || p.type == KWOK_WATCH_NONE || !p.obj_set) {
            f.status = KWOK_EINVAL;
        } else {
            f.type = p.type, f.flags = p.flags;
            f.doc_off = p.obj_pos, f.doc_len = p.obj_len;
            f.uid = kwok_str{p.uid.off, p.uid.len};
            f.resource_version = kwok_str{p.rv.off, p.rv.len};
            f.name = kwok_str{p.name.off, p.name.len};
            f.namespace_ = kwok_str{p.ns.off, p.ns.len};
        }
    }
    frames[i] = f;
}

// the response framer (kwok_watch.h, kwok_frame_responses_gpu): one thread per document
// [off[i], +dlen[i]) of the uploaded buffer, the object at the root (FrameScanT<1>); a span
// that does not lie inside the buffer is refused before a byte of it is read
__global__ __launch_bounds__(256) void k_resp_parse(const uint8_t* s, uint64_t len, const uint64_t* off, const uint32_t* dlen,
                                                    uint32_t n, kwok_watch_frame* frames, uint32_t* host_list, uint32_t* n_host) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t o = off[i];
    const uint32_t l = dlen[i];
    kwok_watch_frame f;
    f.line_off = f.doc_off = f.doc_len = 0;
    f.type = KWOK_WATCH_NONE, f.flags = 0, f.status = KWOK_OK, f.reserved0 = 0;
    f.uid = f.resource_version = f.name = f.namespace_ = kwok_str{0, 0};
    if (o > len || l > len - o) {
        f.status = KWOK_EINVAL;
        frames[i] = f;
        return;
    }
    const jpos lo = (jpos)o, hi = lo + l;
    f.line_off = lo;
    JRd rd{s, lo, hi, ~0u, make_uint4(0, 0, 0, 0)};
    for (;;) {  // a span of only whitespace: KWOK_WATCH_NONE
        const int c = rd.peek();
        if (c != ' ' && c != '\t' && c != '\n' && c != '\r') break;
        rd.pos++;
    }
    if (rd.pos < hi) {
        FrameScanT<1> p;
        p.r = &rd;
        const bool ok = jparse(rd, p);  // (d0 = 0: only whitespace may follow the value)
        if (!ok || !p.root_obj) {
            f.status = KWOK_EINVAL;
        } else if (p.host) {
            host_list[atomicAdd(n_host, 1u)] = i;  // (its frame is the host framer's)
        } else {
            f.type = KWOK_WATCH_MODIFIED, f.flags = p.flags;
            f.doc_off = p.obj_pos, f.doc_len = p.obj_len;
            f.uid = kwok_str{p.uid.off, p.uid.len};
            f.resource_version = kwok_str{p.rv.off, p.rv.len};
            f.name = kwok_str{p.name.off, p.name.len};
            f.namespace_ = kwok_str{p.ns.off, p.ns.len};
        }
    }
    frames[i] = f;
}

void launch_frame_count(const uint8_t* s, uint64_t len, uint32_t n_tiles, uint32_t* tile_cnt, hipStream_t st) {
    if (n_tiles) hipLaunchKernelGGL(k_frame_count, dim3(n_tiles), dim3(FR_THREADS), 0, st, s, len, tile_cnt);
}
void launch_frame_scan(const uint32_t* tile_cnt, uint32_t n_tiles, uint32_t* tile_base, uint32_t* total, hipStream_t st) {
    hipLaunchKernelGGL(k_frame_scan, dim3(1), dim3(KWOK_WATCH_SCAN_TILES), 0, st, tile_cnt, n_tiles, tile_base, total);
}
void launch_frame_emit(const uint8_t* s, uint64_t len, uint32_t n_tiles, const uint32_t* tile_base, uint32_t* ends,
                       uint32_t n_ends, hipStream_t st) {
    if (n_tiles && n_ends)
        hipLaunchKernelGGL(k_frame_emit, dim3(n_tiles), dim3(FR_THREADS), 0, st, s, len, tile_base, ends, n_ends);
}
void launch_frame_parse(const uint8_t* s, const uint32_t* ends, uint32_t n, kwok_watch_frame* frames, uint32_t* host_list,
                        uint32_t* n_host, hipStream_t st) {
    if (!n) return;
    const uint32_t bs = json_block(n);
    hipLaunchKernelGGL(k_frame_parse, dim3((n + bs - 1) / bs), dim3(bs), 0, st, s, ends, n, frames, host_list, n_host);
}
void launch_resp_parse(const uint8_t* s, uint64_t len, const uint64_t* off, const uint32_t* dlen, uint32_t n,
                       kwok_watch_frame* frames, uint32_t* host_list, uint32_t* n_host, hipStream_t st) {
    if (!n) return;
    const uint32_t bs = json_block(n);
    hipLaunchKernelGGL(k_resp_parse, dim3((n + bs - 1) / bs), dim3(bs), 0, st, s, len, off, dlen, n, frames, host_list, n_host);
}

// ---------------------------------------------------------------------------
// the List body framer (kwok_watch.h, kwok_frame_list_gpu): one JSON value,
// {"kind":"PodList","metadata":{..},"items":[{..},{..}]}, no newline between items.
// An item ends where the bracket depth returns to the array's, the depth needs the
// in-string state, the state needs escaped quotes - scans that cross tiles:
//   k_list_quotes  per 16-byte window the masks of unescaped quotes and of brackets;
//                  per tile the count of unescaped quotes and the tile's net depth
//                  change for both in-string states it may be entered in
//   k_frame_scan   over the quote counts: a tile's entry state is its base's parity
//   k_list_pick    the depth change of each tile's actual entry state;
//   k_frame_scan   over those: a tile's entry depth (a wrapping 32-bit sum)
//   k_list_split   <false> counts, per tile, the `{` that raise the depth 2 -> 3 and
//                  the `}` that bring it back, and records the `[` / `]` that open and
//                  close an array directly under the root; after two more scans <true>
//                  writes their offsets at base + rank, in stream order
//   k_list_range   the candidates inside the root array: a contiguous rank range
//   k_list_parse   one thread per item: jparse (d0 = 2) over exactly the item's span,
//                  and the gap before it (after the last one too): whitespace and,
//                  between items, exactly one comma.  Any failure marks the body.
// No kernel waits on another block: separate launches with scans between them.
// Loads are guarded as nl_window's are.
// ---------------------------------------------------------------------------
namespace {
// bit k set for each byte k of x equal to the byte repeated in pat (nl4's zero-byte test)
__device__ __forceinline__ uint32_t eq4(uint32_t x, uint32_t pat) {
    const uint32_t y = x ^ pat;
    const uint32_t m = ~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y | 0x7F7F7F7Fu);
    return (((m >> 7) & 0x01010101u) * 0x01020408u) >> 24;
}
__device__ __forceinline__ uint32_t eq16(const uint4& w, uint32_t pat) {
    return eq4(w.x, pat) | eq4(w.y, pat) << 4 | eq4(w.z, pat) << 8 | eq4(w.w, pat) << 12;
}
// bit k set for each byte k of x whose bit 5 is set (`{` `}` have it, `[` `]` do not)
__device__ __forceinline__ uint32_t bit5_4(uint32_t x) { return (((x >> 5) & 0x01010101u) * 0x01020408u) >> 24; }

// one 16-byte window: its unescaped quotes, its opening and closing brackets of
// both kinds (inside strings too), and which bytes are braces
struct LWin {
    uint32_t q, open, close, brace;
};
// A quote is escaped when the run of backslashes before it is odd.  The run may
// begin in an earlier window: whether the byte before the window is a backslash
// comes from the neighbour lane (lane 0: from memory), and only then does the lane
// follow the run backwards through memory - bounded by the run, never before
// offset 0.  Called by all lanes of the wave.
__device__ __forceinline__ LWin list_window(const uint8_t* s, uint64_t off, uint64_t len, uint32_t lane) {
    LWin r{0, 0, 0, 0};
    uint32_t bs = 0;
    const bool live = off < len;
    if (live) {
        const uint4 w = *reinterpret_cast<const uint4*>(s + off);
        const uint32_t keep = len - off < 16 ? (1u << (uint32_t)(len - off)) - 1u : 0xFFFFu;
        const uint4 v = make_uint4(w.x | 0x20202020u, w.y | 0x20202020u, w.z | 0x20202020u, w.w | 0x20202020u);
        r.q = eq16(w, 0x22222222u) & keep;
        bs = eq16(w, 0x5C5C5C5Cu) & keep;
        r.open = eq16(v, 0x7B7B7B7Bu) & keep;   // `[` 5B | 20 = `{` 7B
        r.close = eq16(v, 0x7D7D7D7Du) & keep;  // `]` 5D | 20 = `}` 7D
        r.brace = bit5_4(w.x) | bit5_4(w.y) << 4 | bit5_4(w.z) << 8 | bit5_4(w.w) << 12;
    }
    uint32_t prev = __shfl_up(bs, 1) >> 15;
    if (lane == 0) prev = live && off && s[off - 1] == '\\';
    if (live && (bs | prev)) {
        bool esc = false;  // the next byte is escaped
        if (prev) {
            uint64_t k = off - 1;
            while (k > 0 && s[k - 1] == '\\') k--;
            esc = ((off - k) & 1) != 0;
        }
        uint32_t e = 0;
        for (uint32_t k = 0; k < 16; k++) {
            if (esc) e |= 1u << k, esc = false;
            else esc = (bs >> k) & 1u;
        }
        r.q &= ~e;
    }
    return r;
}
// bit k: the parity of the set bits 0..k of the 16-bit mask
__device__ __forceinline__ uint32_t prefix_xor16(uint32_t m) {
    m ^= m << 1;
    m ^= m << 2;
    m ^= m << 4;
    m ^= m << 8;
    return m & 0xFFFFu;
}
__device__ __forceinline__ uint32_t wave_incl_xor(uint32_t v, uint32_t lane) {
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(v, o);
        if (lane >= o) v ^= t;
    }
    return v;
}
constexpr uint32_t FR_WAVES = FR_THREADS / 64;
// the block's exclusive prefix of v over its 256 lanes and the block's total; wt: one
// of two sets of wave totals (a step's are read while the next step's are written)
template <bool XOR>
__device__ __forceinline__ uint32_t block_excl(uint32_t v, uint32_t lane, uint32_t wave, uint32_t* wt, uint32_t& all) {
    const uint32_t incl = XOR ? wave_incl_xor(v, lane) : wave_incl(v, lane);
    if (lane == 63) wt[wave] = incl;
    __syncthreads();
    uint32_t before = 0;
    all = 0;
    for (uint32_t w = 0; w < FR_WAVES; w++) {
        const uint32_t t = wt[w];
        if (XOR) {
            if (w < wave) before ^= t;
            all ^= t;
        } else {
            if (w < wave) before += t;
            all += t;
        }
    }
    return XOR ? before ^ incl ^ v : before + incl - v;
}

// FrameScan's object half for an item of the list: the item is at depth 2
struct ItemScan {
    JRd* r;
    uint8_t next = F_NONE;
    bool host = false, root_obj = false, in_meta = false;
    uint32_t seen_obj = 0, seen_meta = 0;
    uint8_t flags = 0;
    Span uid{0, 0}, rv{0, 0}, name{0, 0}, ns{0, 0};

    __device__ uint8_t first(uint32_t& seen, int bit, uint8_t c) {
        if (seen & (1u << bit)) return F_NONE;
        seen |= 1u << bit;
        return c;
    }
    __device__ void key(int d, const JTok& t) {
        next = F_NONE;
        const bool routed = d == 2 || (d == 3 && in_meta);
        if (!routed) return;
        if (t.esc) {  // a routed key is compared as decoded text: the host framer decides the item
            host = true;
            return;
        }
        if (d == 2) {
            if (lit_eq(*r, t.off, t.len, "metadata")) next = first(seen_obj, 0, F_META);
        } else {
            if (lit_eq(*r, t.off, t.len, "uid")) next = first(seen_meta, 0, F_UID);
            else if (lit_eq(*r, t.off, t.len, "resourceVersion")) next = first(seen_meta, 1, F_RV);
            else if (lit_eq(*r, t.off, t.len, "name")) next = first(seen_meta, 2, F_NAME);
            else if (lit_eq(*r, t.off, t.len, "namespace")) next = first(seen_meta, 3, F_NS);
        }
    }
    __device__ void scalar(int d, const JTok& t, bool pa) {
        if (pa || d != 4 || !in_meta || t.kind != J_STR) return;  // (a non-string value: an empty span)
        const Span s = t.len ? Span{(uint32_t)t.off, t.len} : Span{0, 0};
        switch (next) {
            case F_UID: uid = s; if (t.esc) flags |= KWOK_FRAME_ESC_UID; break;
            case F_RV: rv = s; if (t.esc) flags |= KWOK_FRAME_ESC_RV; break;
            case F_NAME: name = s; if (t.esc) flags |= KWOK_FRAME_ESC_NAME; break;
            case F_NS: ns = s; if (t.esc) flags |= KWOK_FRAME_ESC_NS; break;
            default: break;
        }
    }
    __device__ void begin(int d, bool a, bool pa) {
        if (d == 2) {
            root_obj = !a;
            return;
        }
        if (!pa && d == 3 && next == F_META && !a) in_meta = true;
    }
    __device__ void end(int d, bool, bool) {
        if (d == 3) in_meta = false;
    }
};
}  // namespace

// tile_q[i]: the unescaped quotes of tile i; tile_d0 / tile_d1[i]: its net depth change
// when it is entered outside / inside a string
__global__ __launch_bounds__(FR_THREADS) void k_list_quotes(const uint8_t* s, uint64_t len, uint32_t* tile_q,
                                                           uint32_t* tile_d0, uint32_t* tile_d1) {
    __shared__ uint32_t wx[2][FR_WAVES];
    __shared__ uint32_t red[3][FR_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t state = 0;  // the in-string parity at the step's start, the tile entered outside a string
    uint32_t nq = 0, d0 = 0, d1 = 0;
    for (uint32_t q = 0; q < FR_STEPS; q++) {
        const uint64_t off = (uint64_t)blockIdx.x * KWOK_WATCH_TILE_BYTES + (uint64_t)q * FR_STEP + tid * 16u;
        const LWin w = list_window(s, off, len, lane);
        const uint32_t c = __popc(w.q);
        uint32_t all;
        const uint32_t in = state ^ block_excl<true>(c & 1u, lane, wave, wx[q & 1], all);
        state ^= all;
        const uint32_t str = prefix_xor16(w.q) ^ (in ? 0xFFFFu : 0u);  // the window's bytes inside a string
        nq += c;
        d0 += __popc(w.open & ~str) - __popc(w.close & ~str);
        d1 += __popc(w.open & str) - __popc(w.close & str);
    }
    for (uint32_t o = 32; o; o >>= 1) nq += __shfl_down(nq, o), d0 += __shfl_down(d0, o), d1 += __shfl_down(d1, o);
    if (lane == 0) red[0][wave] = nq, red[1][wave] = d0, red[2][wave] = d1;
    __syncthreads();
    if (tid < 3) {
        uint32_t t = 0;
        for (uint32_t w = 0; w < FR_WAVES; w++) t += red[tid][w];
        (tid == 0 ? tile_q : tid == 1 ? tile_d0 : tile_d1)[blockIdx.x] = t;
    }
}

// tile_d0[i] <- the depth change of tile i for the state it is entered in
__global__ void k_list_pick(const uint32_t* q_base, uint32_t* tile_d0, const uint32_t* tile_d1, uint32_t n_tiles) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_tiles && (q_base[i] & 1u)) tile_d0[i] = tile_d1[i];
}

// EMIT false: tile_s / tile_e[i] = the candidate starts / ends of tile i (a `{` that
// raises the depth 2 -> 3, a `}` that lowers it 3 -> 2), and the root arrays' brackets
// in lc.  EMIT true: tile_s / tile_e are the scanned bases; starts / ends[rank] = offset.
template <bool EMIT>
__global__ __launch_bounds__(FR_THREADS) void k_list_split(const uint8_t* s, uint64_t len, const uint32_t* q_base,
                                                          const uint32_t* d_base, uint32_t* tile_s, uint32_t* tile_e,
                                                          uint32_t* starts, uint32_t* ends, uint32_t n_cand, uint32_t* lc) {
    __shared__ uint32_t wx[2][FR_WAVES], wd[2][FR_WAVES], wr[2][FR_WAVES];
    __shared__ uint32_t red[2][FR_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t state = q_base[blockIdx.x] & 1u;
    uint32_t depth = d_base[blockIdx.x];
    uint32_t run_s = EMIT ? tile_s[blockIdx.x] : 0u, run_e = EMIT ? tile_e[blockIdx.x] : 0u;
    uint32_t cnt = 0;  // starts in the low half, ends in the high half (a tile holds at most 16384 of each)
    for (uint32_t q = 0; q < FR_STEPS; q++) {
        const uint64_t off = (uint64_t)blockIdx.x * KWOK_WATCH_TILE_BYTES + (uint64_t)q * FR_STEP + tid * 16u;
        const LWin w = list_window(s, off, len, lane);
        uint32_t all;
        const uint32_t in = state ^ block_excl<true>(__popc(w.q) & 1u, lane, wave, wx[q & 1], all);
        state ^= all;
        const uint32_t str = prefix_xor16(w.q) ^ (in ? 0xFFFFu : 0u);
        const uint32_t op = w.open & ~str, cl = w.close & ~str;
        uint32_t d = depth + block_excl<false>(__popc(op) - __popc(cl), lane, wave, wd[q & 1], all);
        depth += all;
        // the window's brackets in order; only depths 1..3 matter
        uint32_t m = op | cl, c = 0, sm = 0, em = 0;
        if (m && d <= 19u) {
            while (m) {
                const uint32_t b = (uint32_t)__builtin_ctz(m), bit = 1u << b;
                m &= m - 1;
                const bool brace = (w.brace & bit) != 0;
                if (op & bit) {
                    if (d == 2 && brace) c += 1u, sm |= bit;
                    if (!EMIT && d == 1 && !brace) atomicAdd(lc + LC_OPEN_N, 1u), atomicMin(lc + LC_OPEN_POS, (uint32_t)(off + b));
                    d++;
                } else {
                    d--;
                    if (d == 2 && brace) c += 0x10000u, em |= bit;
                    if (!EMIT && d == 1 && !brace) atomicAdd(lc + LC_CLOSE_N, 1u), atomicMax(lc + LC_CLOSE_POS, (uint32_t)(off + b));
                }
            }
        }
        if (!EMIT) {
            cnt += c;
        } else {
            const uint32_t ex = block_excl<false>(c, lane, wave, wr[q & 1], all);
            uint32_t ks = run_s + (ex & 0xFFFFu), ke = run_e + (ex >> 16);
            while (sm) {
                const uint32_t b = (uint32_t)__builtin_ctz(sm);
                sm &= sm - 1;
                if (ks < n_cand) starts[ks] = (uint32_t)(off + b);
                ks++;
            }
            while (em) {
                const uint32_t b = (uint32_t)__builtin_ctz(em);
                em &= em - 1;
                if (ke < n_cand) ends[ke] = (uint32_t)(off + b);
                ke++;
            }
            run_s += all & 0xFFFFu, run_e += all >> 16;
        }
    }
    if (!EMIT) {
        uint32_t a = cnt & 0xFFFFu, b = cnt >> 16;  // (a lane's four windows: at most 64 of each)
        for (uint32_t o = 32; o; o >>= 1) a += __shfl_down(a, o), b += __shfl_down(b, o);
        if (lane == 0) red[0][wave] = a, red[1][wave] = b;
        __syncthreads();
        if (tid < 2) {
            uint32_t t = 0;
            for (uint32_t w = 0; w < FR_WAVES; w++) t += red[tid][w];
            (tid == 0 ? tile_s : tile_e)[blockIdx.x] = t;
        }
    }
}

// lc[LC_R0], lc[LC_R1]: the candidates whose `{` lies inside the root array (open, close)
__global__ void k_list_range(const uint32_t* starts, uint32_t n_cand, uint32_t open, uint32_t close, uint32_t* lc) {
    if (threadIdx.x > 1 || blockIdx.x) return;
    const uint32_t key = threadIdx.x ? close : open;
    uint32_t lo = 0, hi = n_cand;
    while (lo < hi) {  // the first candidate past key
        const uint32_t mid = lo + (hi - lo) / 2;
        if (starts[mid] > key) hi = mid;
        else lo = mid + 1;
    }
    lc[threadIdx.x ? LC_R1 : LC_R0] = lo;
}

// one thread per item r0 + i: the gap before it, its parse over exactly its span, its frame
__global__ __launch_bounds__(256) void k_list_parse(const uint8_t* s, const uint32_t* starts, const uint32_t* ends, uint32_t r0,
                                                    uint32_t n, uint32_t open, uint32_t close, kwok_watch_frame* frames,
                                                    uint32_t* host_list, uint32_t* lc) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const jpos lo = starts[r0 + i], last = ends[r0 + i], hi = last + 1u;
    const jpos gap = i ? ends[r0 + i - 1] + 1u : open + 1u;
    kwok_watch_frame f;
    f.line_off = f.doc_off = lo;
    f.doc_len = hi - lo;
    f.type = KWOK_WATCH_ADDED, f.flags = 0, f.status = KWOK_OK, f.reserved0 = 0;
    f.uid = f.resource_version = f.name = f.namespace_ = kwok_str{0, 0};
    // (spans the depth count paired wrongly - an invalid body - are not read at all)
    bool ok = gap <= lo && lo < last && last < close;
    if (ok) {
        JRd rd{s, gap, close, ~0u, make_uint4(0, 0, 0, 0)};
        uint32_t commas = 0;
        for (jpos p = gap; p < lo && ok; p++) {
            const uint32_t c = rd.at(p);
            if (c == ',') ok = ++commas <= (i ? 1u : 0u);
            else ok = c == ' ' || c == '\t' || c == '\n' || c == '\r';
        }
        ok = ok && commas == (i ? 1u : 0u);
        if (ok && i == n - 1)
            for (jpos p = hi; p < close && ok; p++) {
                const uint32_t c = rd.at(p);
                ok = c == ' ' || c == '\t' || c == '\n' || c == '\r';
            }
    }
    if (ok) {
        JRd rd{s, lo, hi, ~0u, make_uint4(0, 0, 0, 0)};
        ItemScan p;
        p.r = &rd;
        ok = jparse(rd, p, 2) && p.root_obj && rd.pos == hi;
        if (ok && p.host) {
            host_list[atomicAdd(lc + LC_HOST, 1u)] = i;  // (its frame is the host framer's)
        } else if (ok) {
            f.flags = p.flags;
            f.uid = kwok_str{p.uid.off, p.uid.len};
            f.resource_version = kwok_str{p.rv.off, p.rv.len};
            f.name = kwok_str{p.name.off, p.name.len};
            f.namespace_ = kwok_str{p.ns.off, p.ns.len};
        }
    }
    if (!ok) atomicOr(lc + LC_BAD, 1u);
    frames[i] = f;
}

void launch_list_quotes(const uint8_t* s, uint64_t len, uint32_t n_tiles, uint32_t* tile_q, uint32_t* tile_d0,
                        uint32_t* tile_d1, hipStream_t st) {
    if (n_tiles) hipLaunchKernelGGL(k_list_quotes, dim3(n_tiles), dim3(FR_THREADS), 0, st, s, len, tile_q, tile_d0, tile_d1);
}
void launch_list_pick(const uint32_t* q_base, uint32_t* tile_d0, const uint32_t* tile_d1, uint32_t n_tiles, hipStream_t st) {
    if (n_tiles) hipLaunchKernelGGL(k_list_pick, dim3((n_tiles + 255) / 256), dim3(256), 0, st, q_base, tile_d0, tile_d1, n_tiles);
}
void launch_list_count(const uint8_t* s, uint64_t len, uint32_t n_tiles, const uint32_t* q_base, const uint32_t* d_base,
                       uint32_t* tile_s, uint32_t* tile_e, uint32_t* lc, hipStream_t st) {
    if (n_tiles)
        hipLaunchKernelGGL(k_list_split<false>, dim3(n_tiles), dim3(FR_THREADS), 0, st, s, len, q_base, d_base, tile_s, tile_e,
                           (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, lc);
}
void launch_list_emit(const uint8_t* s, uint64_t len, uint32_t n_tiles, const uint32_t* q_base, const uint32_t* d_base,
                      uint32_t* s_base, uint32_t* e_base, uint32_t* starts, uint32_t* ends, uint32_t n_cand, hipStream_t st) {
    if (n_tiles && n_cand)
        hipLaunchKernelGGL(k_list_split<true>, dim3(n_tiles), dim3(FR_THREADS), 0, st, s, len, q_base, d_base, s_base, e_base,
                           starts, ends, n_cand, (uint32_t*)nullptr);
}
void launch_list_range(const uint32_t* starts, uint32_t n_cand, uint32_t open, uint32_t close, uint32_t* lc, hipStream_t st) {
    hipLaunchKernelGGL(k_list_range, dim3(1), dim3(64), 0, st, starts, n_cand, open, close, lc);
}
void launch_list_parse(const uint8_t* s, const uint32_t* starts, const uint32_t* ends, uint32_t r0, uint32_t n, uint32_t open,
                       uint32_t close, kwok_watch_frame* frames, uint32_t* host_list, uint32_t* lc, hipStream_t st) {
    if (!n) return;
    const uint32_t bs = json_block(n);
    hipLaunchKernelGGL(k_list_parse, dim3((n + bs - 1) / bs), dim3(bs), 0, st, s, starts, ends, r0, n, open, close, frames,
                       host_list, lc);
}
}  // namespace kwok
