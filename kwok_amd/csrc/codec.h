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
}  // namespace kwok
