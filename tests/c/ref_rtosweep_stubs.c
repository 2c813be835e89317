/*
 * ref_rtosweep_stubs.c — TEST INFRASTRUCTURE ONLY (tests/make_rtosweep_golden.py).
 *
 * The reference's timer.c refers to the rest of mTCP.  HandleRTO ends in the
 * list and event functions below: each is a counting stub that tells
 * ref_rtosweep_gen.c which one ran for which stream.  RemoveFromControlList is
 * not reached by the cases (no stream is on the control list) and aborts.
 * Deliberately compiled without the reference's headers (names only).
 */
#include <stdlib.h>

void (*rto_stub_hook)(int which, void *stream);

void AddtoSendList(void *mtcp, void *stream) { rto_stub_hook(0, stream); }
void AddtoControlList(void *mtcp, void *stream, unsigned cur_ts) { rto_stub_hook(1, stream); }
void RaiseErrorEvent(void *mtcp, void *stream) { rto_stub_hook(2, stream); }
void DestroyTCPStream(void *mtcp, void *stream) { rto_stub_hook(3, stream); }
void RemoveFromControlList(void *mtcp, void *stream) { abort(); }
/* named by the trace lines at timer.c:220-222 and :298-300, which -DDBGERR compiles in */
const char *TCPStateToString(void *stream) { return "-"; }
