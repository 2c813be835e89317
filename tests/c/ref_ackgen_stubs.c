/*
 * ref_ackgen_stubs.c — TEST INFRASTRUCTURE ONLY (tests/make_ackgen_golden.py).
 *
 * The reference's tcp_out.c, ip_out.c and tcp_util.c refer to the rest of
 * mTCP.  EnqueueACK and WriteTCPACKList for an ESTABLISHED stream, as
 * ref_ackgen_gen.c drives them, reach none of these; each stub aborts, so
 * reaching one would be loud.  Deliberately compiled without the reference's
 * headers (names only).
 */
#include <stdlib.h>

#define STUB(name) void name(void) { abort(); }
STUB(DestroyTCPStream)
STUB(TCPStateToString)
