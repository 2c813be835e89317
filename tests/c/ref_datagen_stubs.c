/*
 * ref_datagen_stubs.c — TEST INFRASTRUCTURE ONLY (tests/make_datagen_golden.py).
 *
 * The reference's tcp_out.c, ip_out.c, tcp_util.c and timer.c refer to the rest
 * of mTCP.  WriteTCPDataList for an ESTABLISHED stream, as ref_datagen_gen.c
 * drives it, reaches none of these but the state's name for a trace line; each
 * stub aborts, so reaching one would be loud.  Deliberately compiled without the reference's headers (names only).
 */
#include <stdlib.h>

#define STUB(name) void name(void) { abort(); }
STUB(DestroyTCPStream)
STUB(RaiseErrorEvent)
/* named by the TRACE_ERROR at tcp_out.c:388-391 (snd_nxt behind head_seq), which -DDBGERR compiles in */
const char *TCPStateToString(void) { return "ESTABLISHED"; }
