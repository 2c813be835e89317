/*
 * ref_rcvwalk_stubs.c — TEST INFRASTRUCTURE ONLY (tests/make_rcvwalk_golden.py).
 *
 * The reference's tcp_in.c refers to the rest of mTCP.  The receive walk of an
 * ESTABLISHED stream that ref_rcvwalk_gen.c drives reaches none of these; each
 * stub aborts, so reaching one would be loud.  Deliberately compiled without
 * the reference's headers (names only): the names oracle/ref/ref_stubs.c lists,
 * less the five the generator defines or links, plus StreamHTSearch.
 */
#include <stdlib.h>

#define STUB(name) void name(void) { abort(); }
STUB(AddEpollEvent)
STUB(AddtoControlList)
STUB(AddtoSendList)
STUB(AddtoTimeoutList)
STUB(AddtoTimewaitList)
STUB(CreateTCPStream)
STUB(DestroyTCPStream)
STUB(IPOutputStandalone)
STUB(ListenerHTSearch)
STUB(RaiseCloseEvent)
STUB(RaiseErrorEvent)
STUB(RaiseWriteEvent)
STUB(RemoveFromRTOList)
STUB(RemoveFromSendList)
STUB(RemoveFromTimewaitList)
STUB(SBRemove)
STUB(SendTCPPacketStandalone)
STUB(StreamEnqueue)
STUB(StreamHTSearch)
STUB(UpdateRetransmissionTimer)
STUB(UpdateTimeoutList)
