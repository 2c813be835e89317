/*
 * ref_ackwalk_stubs.c — TEST INFRASTRUCTURE ONLY (tests/make_ackwalk_golden.py).
 *
 * The reference's tcp_in.c and timer.c refer to the rest of mTCP.  The walk of
 * an ESTABLISHED stream that ref_ackwalk_gen.c drives reaches none of these;
 * each stub aborts, so reaching one would be loud.  Deliberately compiled
 * without the reference's headers (names only).
 */
#include <stdlib.h>

#define STUB(name) void name(void) { abort(); }
STUB(AddEpollEvent)
STUB(AddtoControlList)
STUB(CreateTCPStream)
STUB(DestroyTCPStream)
STUB(IPOutputStandalone)
STUB(ListenerHTSearch)
STUB(RaiseCloseEvent)
STUB(RaiseErrorEvent)
STUB(RemoveFromControlList)
STUB(SendTCPPacketStandalone)
STUB(StreamEnqueue)
STUB(StreamHTSearch)
STUB(TCPStateToString)
