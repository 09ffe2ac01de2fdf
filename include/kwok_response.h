/* kwok_response.h - echo-ledger notes from resident response frames.
 *
 * The responses to the engine's own patches are framed by kwok_frame_responses_gpu
 * (kwok_watch.h); the note every response owes the echo ledger (kwok_watch.h, §24) is
 * then taken from the resident frames.  The entry lives in a header of its own because
 * the ledger's ABI test picks kwok_watch.h's entries by name.
 */
#ifndef KWOK_RESPONSE_H
#define KWOK_RESPONSE_H

#include "kwok_watch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One KWOK_ECHO_NOTE per record, uid and rv taken from frame frame_idx[i] of the resident
 * stream, applied in array order per uid: exactly what kwok_echo_update does with the same
 * pairs.  No uid or rv byte crosses the link (n indices in, n statuses out).
 * out_status[i] (optional): KWOK_OK the note was applied, or ignored because the uid or rv
 * is empty; KWOK_EDOMAIN a uid longer than KWOK_UID_MAX, an rv longer than KWOK_RV_MAX or a
 * frame with KWOK_FRAME_ESC_UID / _RV (nothing stored: the caller notes the decoded text
 * through kwok_echo_update); KWOK_EINVAL a frame index out of range, a frame whose status
 * is not KWOK_OK or that is not ingestible (NONE / BOOKMARK / ERROR).  The ledger not
 * enabled or a stale stream_id: KWOK_EINVAL for the call; KWOK_EFULL as kwok_echo_update
 * (nothing stored).  Returns the number of records not KWOK_OK, or an error. */
int kwok_echo_note_framed(kwok_engine* e, uint64_t stream_id, const uint32_t* frame_idx, size_t n, int32_t* out_status);

#ifdef __cplusplus
}
#endif
#endif
