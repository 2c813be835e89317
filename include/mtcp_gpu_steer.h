/*
 * mtcp_gpu_steer.h — steering an rx batch into per-queue packet lists
 * (SURVEY §8 row f6).
 *
 * In the reference the RSS queue number has one purpose.  The NIC's RSS
 * redirection table (mtcp/src/dpdk_module.c:101-121) puts each frame into the
 * receive ring of one core, and each mTCP thread reads only its own ring
 * (rte_eth_rx_burst(portid, ctxt->cpu, ...), dpdk_module.c:401-402): a flow's
 * segments reach one share-nothing core, in arrival order.  The rx entry
 * points of mtcp_gpu.h compute that queue for every frame (rss_queue,
 * GetRSSCPUCore, mtcp/src/rss.c:90-103); the entry points here act on it: a
 * stable partition of the batch by destination queue, on the device, behind
 * the rx launch.  Per queue the caller gets the list of packet indices in
 * arrival order, and optionally the descriptors gathered the same way.
 *
 * Stability is the contract: two segments of one flow carry the same 4-tuple,
 * get the same queue, and come out in the order they went in.
 *
 * Plain C, as mtcp_gpu.h; MTCP_GPU_ABI_VERSION is unchanged (nothing that
 * exists changes): test for MTCP_GPU_HAS_STEER.
 */
#ifndef MTCP_GPU_STEER_H
#define MTCP_GPU_STEER_H

#include "mtcp_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MTCP_GPU_HAS_STEER          1
#define MTCP_GPU_STEER_MAX_QUEUES   128u        /* GetRSSCPUCore never returns 128 or more:
                                                   (h & 0x7F), permuted within groups of 4, % nq */
#define MTCP_GPU_STEER_MAX_PKTS     (1u << 26)
#define MTCP_GPU_STEER_DROP_BAD     0x1u        /* flags */

/*
 * The lists.  Q is the context's rss_num_queues (1 for a context opened
 * without MTCP_GPU_F_RSS).  There are Q + 1 lists: lists 0 .. Q-1 are the
 * queues, list Q is the REST list of the packets no queue gets.  The list of
 * record i, of which only verdict and rss_queue are read:
 *   - rss_queue >= Q: the rest list.  (Records the same context's rx wrote
 *     never reach this; it keeps a caller's garbage record from indexing
 *     outside the lists.)
 *   - with MTCP_GPU_STEER_DROP_BAD, the verdicts MTCP_GPU_V_IP_CSUM_BAD,
 *     _TCP_CSUM_BAD, _TRUNCATED, _BAD_DESC and every value above _BAD_DESC:
 *     the rest list.  These are the frames for which an io_module's get_rptr
 *     answers NULL (the pattern of dpdk_module.c:473-479), and the frames
 *     that were never read.
 *   - every other packet: the list of its rss_queue.  Frames that never reach
 *     the TCP head carry rss_queue 0 and land in queue 0, where a NIC's RSS
 *     puts the frames it cannot hash.
 *
 * Outputs.  d_start[Q + 2]: d_start[l] is the position in d_idx where list l
 * begins, d_start[Q + 1] = n.  d_idx[n]: packet indices; list l occupies
 * positions [d_start[l], d_start[l + 1]), strictly ascending within every
 * list.  d_desc_out[p] = d_desc[d_idx[p]] when both pointers are given, so
 * that each queue's slice is a ps_chunk-style info[] array of its own; both
 * NULL is allowed.  The result is a pure function of the records: two runs
 * give identical bytes.
 */

/* Packets per workgroup tile (sizing, tests).  A batch of at most one tile
 * runs as one launch of one workgroup. */
uint32_t mtcp_gpu_steer_tile(void);

/* Bytes of workspace mtcp_gpu_steer_dev needs for n records on this context
 * (dpdk_module.c:101-121, :401-402, mtcp/src/rss.c:90-103: see above); 0 if
 * ctx is NULL, its Q is above MTCP_GPU_STEER_MAX_QUEUES or n is above
 * MTCP_GPU_STEER_MAX_PKTS. */
uint64_t mtcp_gpu_steer_work_bytes(const mtcp_gpu_ctx *ctx, uint32_t n);

/*
 * Steer n device-resident rx records: what the NIC's redirection table
 * (dpdk_module.c:101-121) and the per-core rx burst (dpdk_module.c:401-402)
 * do with GetRSSCPUCore's queue (mtcp/src/rss.c:90-103).  d_res holds this
 * context's rx records (40 B, or 16 B on an MTCP_GPU_F_COMPACT context).
 * Asynchronous on `stream` (NULL = the context's stream); allocates nothing,
 * waits for nothing and copies nothing to the host, so it can sit in a stream
 * capture behind the rx launch.  All scratch is the caller's d_work: 16 B
 * aligned, work_bytes >= mtcp_gpu_steer_work_bytes(ctx, n).
 * MTCP_GPU_EINVAL: NULL arguments, misaligned arguments (d_idx or d_start not
 * 4 B aligned, the descriptor arrays or d_res not 8 B aligned, d_work not
 * 16 B), exactly one of d_desc / d_desc_out NULL, unknown flag bits, Q above
 * MTCP_GPU_STEER_MAX_QUEUES, n above MTCP_GPU_STEER_MAX_PKTS, a workspace
 * that is too small.  MTCP_GPU_EIO on an abandoned context.  n == 0 is
 * MTCP_GPU_OK without a launch, nothing written.
 */
int mtcp_gpu_steer_dev(mtcp_gpu_ctx *ctx, const mtcp_gpu_result *d_res, uint32_t n, uint32_t flags,
                       uint32_t *d_idx, uint32_t *d_start,
                       const mtcp_gpu_desc *d_desc, mtcp_gpu_desc *d_desc_out,
                       void *d_work, uint64_t work_bytes, void *stream);

/*
 * The same for records in host memory (dpdk_module.c:101-121, :401-402,
 * mtcp/src/rss.c:90-103): idx[n] and start[Q + 2] written to host memory.
 * Synchronous, built like mtcp_gpu_flow_hash: the records go up on the
 * context's stream, the lists come back; the workspace comes from the
 * context's staging.  Bounded by the context's wait limit
 * (mtcp_gpu_set_wait_limit): past it neither idx nor start is written,
 * MTCP_GPU_ETIMEDOUT is returned and the context is ABANDONED.
 */
int mtcp_gpu_steer(mtcp_gpu_ctx *ctx, const mtcp_gpu_result *res, uint32_t n, uint32_t flags,
                   uint32_t *idx, uint32_t *start);

#ifdef __cplusplus
}
#endif

#endif /* MTCP_GPU_STEER_H */
