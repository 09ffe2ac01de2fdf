// node_spans.h - the host helper of the device-input node ingest that needs no device: the check of
// the documents the device listed for the host before their spans are taken from the host's frames.  Included by
// engine.cpp and by the sanitizer program of tools/node_spans_asan.sh.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace kwok {

// list: the listed documents as indices into the kept list kidx (the frame index of every kept record), both read
// back from the device.  True when every listed index names a kept record and that record one of n_frames frames,
// so that frames[kidx[list[q]]] reads inside both arrays.
inline bool listed_in_range(const std::vector<uint32_t>& list, const std::vector<uint32_t>& kidx, size_t n_frames) {
    for (uint32_t i : list)
        if (i >= kidx.size() || kidx[i] >= n_frames) return false;
    return true;
}

}  // namespace kwok
