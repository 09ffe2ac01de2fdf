// codec.h - the host codec's internal interface to the engine (codec.cpp)
#pragma once
#include "../../include/kwok_engine.h"
#include "../../include/kwok_watch.h"
#include "device.h"

namespace kwok {
// the codec's compiled selectors in the device scanner's layout (json.hip)
int codec_export(const kwok_codec* c, JsonCfg* out);
// the host framer over one line [lo, hi) of a watch stream (kwok_watch.h; hi: its newline)
void frame_line(const char* stream, uint32_t lo, uint32_t hi, kwok_watch_frame* f);
// the host framer over one item [lo, hi) of a List body (kwok_watch.h): false when the
// span is not one JSON object at the items' depth that fills it
bool frame_item(const char* body, uint32_t lo, uint32_t hi, kwok_watch_frame* f);
// the host framer over one response body [lo, hi) (kwok_watch.h): the object at the root
void frame_response(const char* buf, uint32_t lo, uint32_t hi, kwok_watch_frame* f);
// the envelope of a List body whose root holds one array [open, close] (the
// brackets' offsets): the body with that array emptied is parsed.  KWOK_EINVAL: it
// is no JSON object; 1: it is, but its first `items` is not that array (info
// untouched); KWOK_OK: info filled, offsets into the body
int list_envelope(const char* body, size_t len, uint32_t open, uint32_t close, kwok_list_info* info);
}  // namespace kwok
