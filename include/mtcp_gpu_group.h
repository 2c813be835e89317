/*
 * mtcp_gpu_group.h — grouping an rx batch by stream into per-stream packet
 * lists.
 *
 * RunMainLoop hands the frames of one rx burst to ProcessPacket one after the
 * other, on one thread (mtcp/src/core.c:768-777).  ProcessTCPPacket finds each
 * frame's stream (StreamHTSearch, mtcp/src/tcp_in.c:1181-1186), and everything
 * behind that line is sequential per stream and independent across streams:
 * the state handlers with ValidateSequence, ProcessACK and ProcessTCPPayload ->
 * RBPut (the stateful tail, tcp_in.c:1186 onwards).  The reference gets a
 * stream's segments in arrival order for free, because it walks the burst in
 * arrival order.
 *
 * A batch has no such order: the records of one stream are scattered over the
 * array.  mtcp_gpu_flowtab_lookup[_dev] (mtcp_gpu_flowtab.h) answers which
 * stream every record belongs to; the entry points here act on that answer: a
 * stable partition of the batch by stream id, on the device, behind the lookup
 * launch.  Per stream the caller gets the list of packet indices in arrival
 * order, and a segment table that names every list, so that a wave, a lane or
 * a host thread can take one stream and walk it.
 *
 * Stability is the contract: two segments of one stream come out in the order
 * they went in.  Nothing behind the grouping is built here; its first consumer,
 * the receive walk of every stream's list, is mtcp_gpu_rcvwalk.h.
 *
 * Plain C, as mtcp_gpu.h; MTCP_GPU_ABI_VERSION is unchanged (nothing that
 * exists changes): test for MTCP_GPU_HAS_GROUP.
 */
#ifndef MTCP_GPU_GROUP_H
#define MTCP_GPU_GROUP_H

#include "mtcp_gpu.h"
#include "mtcp_gpu_flowtab.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MTCP_GPU_HAS_GROUP          1
#define MTCP_GPU_GROUP_MAX_PKTS     (1u << 26)

/*
 * The input.  d_sid[n]: u32 values as mtcp_gpu_flowtab_lookup_dev writes them.
 * Only this array is read, so the records of a 40 B and of a 16 B context are
 * served alike.  max_id is the caller's largest stream number, at most
 * MTCP_GPU_FLOWTAB_MAX_ID; it bounds the work: the number of key bits handled
 * is that of max_id + 2, not 32.
 *
 * The class of record i:
 *   - d_sid[i] <= max_id: its stream;
 *   - d_sid[i] == MTCP_GPU_FLOW_MISS: the MISS class (TCP_OK, no stream yet:
 *     where the reference goes on to CreateNewFlowHTEntry, tcp_in.c:1188);
 *   - every other value, MTCP_GPU_FLOW_NONE and any value above max_id: the
 *     NONE class.  (It keeps a caller's garbage from indexing outside
 *     anything, like the rest list of mtcp_gpu_steer.h.)
 *
 * The outputs.  d_idx[n]: packet indices.  All packets of one class are
 * contiguous; the classes are ordered by ascending stream id, then MISS, then
 * NONE; within a class the indices are strictly ascending (arrival order).
 * The segment table: d_nseg[0] = m, the number of non-empty classes;
 * d_seg_sid[0 .. m): the class's stream id, MTCP_GPU_FLOW_MISS or
 * MTCP_GPU_FLOW_NONE for those two; d_seg_start[0 .. m]: positions in d_idx,
 * class j occupies [d_seg_start[j], d_seg_start[j + 1]), d_seg_start[m] = n.
 * The caller sizes d_seg_sid for n and d_seg_start for n + 1 entries; entries
 * past m and m + 1 are not written.
 *
 * The result is a pure function of d_sid and max_id: two runs give identical
 * bytes, nothing depends on what the workspace held, and every store is
 * bounded by n whatever d_sid holds.
 */

/* Records per workgroup tile (sizing, tests) of the grouping that feeds the
 * stateful tail behind core.c:768-777 and tcp_in.c:1181-1186.  A batch of at
 * most one tile (the io_module's 4 096-record aggregate is one) runs as one
 * launch of one workgroup and uses no workspace. */
uint32_t mtcp_gpu_group_tile(void);

/* Bytes of workspace mtcp_gpu_group_dev needs for n records and stream
 * numbers up to max_id (core.c:768-777, tcp_in.c:1181-1186 and the stateful
 * tail: see above).  Host only, needs no GPU.  0 if n is above
 * MTCP_GPU_GROUP_MAX_PKTS or max_id above MTCP_GPU_FLOWTAB_MAX_ID, never 0
 * otherwise; non-decreasing in n and in max_id. */
uint64_t mtcp_gpu_group_work_bytes(uint32_t n, uint32_t max_id);

/*
 * Group n device-resident stream ids: what the burst walk of core.c:768-777
 * gives the stateful tail behind StreamHTSearch (tcp_in.c:1181-1186) for
 * free, each stream's segments together and in arrival order.  Asynchronous
 * on `stream` (NULL = the context's stream); allocates nothing, waits for
 * nothing and copies nothing to the host, so it can sit in a stream capture
 * behind the rx and lookup launches.  All scratch is the caller's d_work: 16 B
 * aligned, work_bytes >= mtcp_gpu_group_work_bytes(n, max_id).
 * MTCP_GPU_EINVAL: NULL arguments, d_sid, d_idx, d_seg_sid, d_seg_start or
 * d_nseg not 4 B aligned, d_work not 16 B aligned, a workspace that is too
 * small, n above MTCP_GPU_GROUP_MAX_PKTS, max_id above
 * MTCP_GPU_FLOWTAB_MAX_ID.  MTCP_GPU_EIO on an abandoned context.  n == 0 is
 * MTCP_GPU_OK without a launch, nothing written.
 */
int mtcp_gpu_group_dev(mtcp_gpu_ctx *ctx, const uint32_t *d_sid, uint32_t n, uint32_t max_id,
                       uint32_t *d_idx, uint32_t *d_seg_sid, uint32_t *d_seg_start, uint32_t *d_nseg,
                       void *d_work, uint64_t work_bytes, void *stream);

/*
 * The same for stream ids in host memory (core.c:768-777, tcp_in.c:1181-1186,
 * the stateful tail): idx[n], seg_sid[n], seg_start[n + 1] and nseg[1] in host
 * memory, of which idx[0 .. n), seg_sid[0 .. m), seg_start[0 .. m] and nseg[0]
 * are written.  Synchronous, built like mtcp_gpu_steer: the ids go up on the
 * context's stream, the lists come back; the workspace comes from the
 * context's staging.  Bounded by the context's wait limit
 * (mtcp_gpu_set_wait_limit): past it nothing of the caller's is written,
 * MTCP_GPU_ETIMEDOUT is returned and the context is ABANDONED.
 */
int mtcp_gpu_group(mtcp_gpu_ctx *ctx, const uint32_t *sid, uint32_t n, uint32_t max_id,
                   uint32_t *idx, uint32_t *seg_sid, uint32_t *seg_start, uint32_t *nseg);

#ifdef __cplusplus
}
#endif

#endif /* MTCP_GPU_GROUP_H */
