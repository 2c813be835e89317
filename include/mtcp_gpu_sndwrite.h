/*
 * mtcp_gpu_sndwrite.h — the batched application write into device send buffers
 * (SURVEY §8 row f18): the producer of the bytes that mtcp_gpu_datagen.h flushes,
 * the mirror image of mtcp_gpu_rcvread.h.
 *
 * What the reference does for one mtcp_write on an ESTABLISHED stream:
 *
 *   mtcp_write    mtcp/src/api.c:1458-1567: the state test (:1495-1501), len <= 0
 *                 (:1503-1510), CopyFromUser, the sendq insertion when ret > 0 &&
 *                 !(on_sendq || on_send_list) (:1535-1541), the write event when
 *                 snd_wnd > 0 (:1548-1563);
 *   CopyFromUser  api.c:1416-1456: sndlen = MIN((int)snd_wnd, len) (:1423), EAGAIN
 *                 where that is <= 0 (:1424-1427), SBInit where there is no buffer
 *                 (:1430-1438), SBPut (:1440), snd_wnd = size - len (:1442),
 *                 written also when SBPut failed, EAGAIN then (:1443-1448);
 *   SBPut         mtcp/src/tcp_send_buffer.c:116-146: to_put = MIN(len, size -
 *                 buf->len), -2 where that is 0 (:125-128); if tail_off + to_put <
 *                 size the memcpy to data + tail_off and tail_off += to_put
 *                 (:130-133); otherwise (:134-141, the exact fit tail_off + to_put
 *                 == size included) memmove(data, head, len), head_off = 0, the
 *                 memcpy to head + len, tail_off = len + to_put; len and cum_len
 *                 grow (:142-143);
 *   SBRemove      tcp_send_buffer.c:166-170: an empty buffer always has head_off
 *                 == tail_off == 0;
 *   the sendq     drained into AddtoSendList, mtcp/src/core.c:479-483 and
 *                 tcp_out.c:837-855.
 *
 * The entry points here do that for a batch of write requests, one per stream,
 * against d_snd (mtcp_gpu_ackwalk.h), d_dtx (mtcp_gpu_datagen.h) and the payload
 * arena the send buffers live in, and write a group table that
 * mtcp_gpu_datagen_dev takes unchanged: application bytes in, data frames out.
 * The next ACK walk, RTO sweep and write follow on the stream with no host
 * refresh in between.
 *
 * Not done here: SBInit (allocation stays with the host: NO_SNDBUF), writes in
 * CLOSE_WAIT (DEFER_STATE), mtcp_writev's further CopyFromUser calls on one
 * stream (one request per stream and batch; the others come back DUP), blocking
 * writes and snd_br_list, epoll events (ROOM says what :1549 tests), PipeWrite,
 * cum_len (the device keeps no mirror of it: the host adds `written`).
 *
 * One difference from the reference: the streams flush in request order.
 * Members already on the host's send list do not go first.  This only matters
 * for which stream meets NO_ROOM in row f15.
 *
 * Plain C, as mtcp_gpu.h; MTCP_GPU_ABI_VERSION is unchanged (nothing that
 * exists changes): test for MTCP_GPU_HAS_SNDWRITE.
 */
#ifndef MTCP_GPU_SNDWRITE_H
#define MTCP_GPU_SNDWRITE_H

#include "mtcp_gpu.h"
#include "mtcp_gpu_ackgen.h"
#include "mtcp_gpu_ackwalk.h"
#include "mtcp_gpu_datagen.h"
#include "mtcp_gpu_rcvwalk.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MTCP_GPU_HAS_SNDWRITE          1

/* The synchronous form packs the requests' bytes into one stage of the
 * context's staging: the sum over the requests of len rounded up to 16 is at
 * most this. */
#define MTCP_GPU_SNDWRITE_HOST_MAX_BYTES (32u << 20)

/* One write, 32 B: the caller's array d_wreq[n], 16 B aligned. */
typedef struct mtcp_gpu_sndwrite_req {
    uint32_t sid;             /*  0 the stream's id                                        */
    uint32_t len;             /*  4 the application's buffer length: CopyFromUser's len    */
    uint64_t src_off;         /*  8 where the bytes lie, as a byte offset into the source region */
    uint32_t flags;           /* 16 must be 0                                              */
    uint32_t rsvd[3];         /* 20 must be 0                                              */
} mtcp_gpu_sndwrite_req;

/* verdict of a request; the first that applies, in this order */
enum mtcp_gpu_sndwrite_verdict {
    MTCP_GPU_SNDWRITE_NONE        = 0,  /* never written */
    MTCP_GPU_SNDWRITE_BAD_REQ     = 1,  /* sid > max_id, a reserved word or flag bit set, len > 0x7FFFFFFF, or
                                           src_off + len > src_bytes: nothing changes */
    MTCP_GPU_SNDWRITE_DUP         = 2,  /* an earlier request of the batch names the same sid: nothing changes */
    MTCP_GPU_SNDWRITE_BAD_STATE   = 3,  /* the records do not describe a writable buffer (below): nothing changes */
    MTCP_GPU_SNDWRITE_DEFER_STATE = 4,  /* tcp_state != 4 (api.c:1495-1501): nothing changes, the host writes itself */
    MTCP_GPU_SNDWRITE_ZERO        = 5,  /* len == 0 (api.c:1503-1510): the host answers by the socket's options */
    MTCP_GPU_SNDWRITE_EAGAIN      = 6,  /* MIN((int)snd_wnd, len) <= 0 (api.c:1423-1427): nothing changes */
    MTCP_GPU_SNDWRITE_NO_SNDBUF   = 7,  /* has_sndbuf == 0 (api.c:1430): the thread runs its own mtcp_write, which allocates */
    MTCP_GPU_SNDWRITE_FULL        = 8,  /* to_put == 0 (tcp_send_buffer.c:125-128): snd_wnd = sb_size - sb_len is
                                           written (api.c:1442), nothing else; the return is EAGAIN (:1443-1448) */
    MTCP_GPU_SNDWRITE_WRITTEN     = 9   /* SBPut's bytes and bookkeeping, snd_wnd, the send list */
};

/* flags of a result */
#define MTCP_GPU_SNDWRITE_ROOM          0x1u  /* snd_wnd > 0 after the call: the test at api.c:1549 */
#define MTCP_GPU_SNDWRITE_SEND_LIST_ADD 0x2u  /* on_send_list was 0: api.c:1535-1541 with core.c:479-483 ran */
#define MTCP_GPU_SNDWRITE_COMPACTED     0x4u  /* tcp_send_buffer.c:134-141 ran: the host's own tcp_send_buffer takes
                                                 head_off = 0, tail_off = len + ret */

/* One per request, 16 B: d_wres[n], 16 B aligned, every one written. */
typedef struct mtcp_gpu_sndwrite_res {
    uint32_t sid;             /*  0 the request's sid                                      */
    uint32_t written;         /*  4 bytes put: what mtcp_write returns; 0 unless WRITTEN   */
    uint32_t snd_wnd;         /*  8 d_snd[sid].snd_wnd after the call; 0 with BAD_REQ, DUP and BAD_STATE */
    uint8_t  verdict;         /* 12 enum mtcp_gpu_sndwrite_verdict                         */
    uint8_t  flags;           /* 13 MTCP_GPU_SNDWRITE_ROOM | _SEND_LIST_ADD | _COMPACTED; 0 with BAD_REQ, DUP and BAD_STATE */
    uint16_t rsvd;            /* 14 0                                                      */
} mtcp_gpu_sndwrite_res;

/*
 * The contract.
 *
 * Where a send buffer lies.  No new mirror: d_snd[sid] has snd_wnd, sb_head_seq,
 * sb_len, sb_size, has_sndbuf (any value but 0 counts as a buffer, as row f15
 * reads it) and tcp_state; d_dtx[sid] has sb_off, sb_base_seq and on_send_list.
 * For a stream written through this call d_dtx[sid] is ANCHORED: sb_off is the
 * arena offset of the chunk's first byte (buf->data), hence head_off =
 * sb_head_seq - sb_base_seq in uint32_t with its wrap and tail_off = head_off +
 * sb_len, the invariant SBInit, SBPut and SBRemove keep.  Row f15 reads an
 * anchored pair exactly as before.  With sb_len == 0 the step takes head_off = 0
 * whatever sb_base_seq holds (the reset at tcp_send_buffer.c:166-170, which the
 * ACK walk does not apply to d_dtx) and writes sb_base_seq = sb_head_seq when it
 * writes.  After a compaction sb_base_seq = sb_head_seq; sb_off keeps its value
 * always.
 *
 * The verdict of request i, the first rule that applies:
 *
 *  1. BAD_REQ.  sid > max_id; flags or a reserved word is not 0; len >
 *     0x7FFFFFFF (CopyFromUser takes an int); src_off + len > src_bytes.
 *  2. DUP.  A request j < i has the same sid (whatever j's own verdict is, as
 *     long as its sid <= max_id).  The lowest index wins.
 *  3. BAD_STATE.  d_snd[sid] is BAD by mtcp_gpu_ackwalk.h's rule (rsvd != 0,
 *     eff_mss == 0, wscale_peer > 31, sb_size > 2^30, sb_len > sb_size);
 *     d_dtx[sid] is BAD by mtcp_gpu_datagen.h's rule (rsvd != 0 or a flag byte
 *     above 1); with has_sndbuf != 0: sb_size == 0, sb_off + sb_size >
 *     payload_bytes, or head_off > sb_size - sb_len.
 *  4. DEFER_STATE.  d_snd[sid].tcp_state != 4.
 *  5. ZERO.  len == 0.
 *  6. EAGAIN.  sndlen = MIN((int)snd_wnd, (int)len) <= 0: a snd_wnd at or above
 *     2^31 is negative here, as in the reference.
 *  7. NO_SNDBUF.  has_sndbuf == 0.
 *  8. FULL.  to_put = MIN(sndlen, sb_size - sb_len) == 0.  d_snd[sid].snd_wnd =
 *     sb_size - sb_len is written (api.c:1442); nothing else changes.
 *  9. WRITTEN.  to_put bytes go from [src_off, src_off + to_put) of the source
 *     region to the chunk: if tail_off + to_put < sb_size to sb_off + tail_off
 *     (:130-133); else the sb_len bytes at sb_off + head_off move to sb_off
 *     (:136, a move onto itself with head_off == 0), the bytes go to sb_off +
 *     sb_len and COMPACTED is set (:134-141).  d_snd[sid].sb_len += to_put,
 *     d_snd[sid].snd_wnd = sb_size - sb_len; d_dtx[sid].sb_base_seq by the rules
 *     above; d_dtx[sid].on_send_list = 1, SEND_LIST_ADD if it was 0.  Every other
 *     byte of both records keeps its value.  written = to_put.
 *
 * The result record.  sid as given.  With BAD_REQ, DUP and BAD_STATE written,
 * snd_wnd and flags are 0.  Otherwise snd_wnd is the record's value after the
 * call and ROOM says that it is above 0.
 *
 * Calling convention.  The thread drains its own sendq (core.c:479-483) before
 * the call, so on_sendq is 0 for every stream; the call folds the enqueue and
 * the drain into on_send_list = 1.
 *
 * The table, which mtcp_gpu_datagen_dev accepts unchanged with n bursts and
 * d_ack and d_ack_stop NULL: d_nseg[0] = n; d_seg_sid[i] = sid where request i
 * is WRITTEN, else MTCP_GPU_FLOW_NONE; d_seg_start[0 .. n] = 0; d_seg_stop[0 ..
 * n) = 0.  d_dres[i] of the data generation then belongs to request i.  No
 * stream appears twice, because of DUP.
 *
 * Totals.  d_total[0] = the requests written, d_total[1] = the bytes written.
 *
 * Replaying d_wres[i] on the host: the return value is written, or -1 / EAGAIN
 * with EAGAIN and FULL; sndvar->snd_wnd = snd_wnd; the host's tcp_send_buffer
 * takes len += written, cum_len += written and tail_off += written, or with
 * COMPACTED head_off = 0, head = data, tail_off = len (the new one); with
 * SEND_LIST_ADD on_send_list = TRUE; with ROOM the write event is raised where
 * the socket asks for it (api.c:1548-1563).  BAD_REQ, DUP, BAD_STATE, DEFER_STATE,
 * ZERO and NO_SNDBUF: the thread runs its own mtcp_write.
 *
 * Bounds.
 *  - Chunk stores land only in [tail_off, tail_off + to_put) of a WRITTEN
 *    request's chunk (no move), or in [0, sb_len) (the move, and only where
 *    head_off != 0) and [sb_len, sb_len + to_put) (the copy).  Every other byte
 *    of the chunk and of the arena keeps its value: the whole chunk is
 *    byte-equal to the reference's data[].  Range edges are written with byte,
 *    short and dword stores, never by reading and rewriting a 16 B piece.
 *  - Loads stay inside the aligned 16 B pieces that hold a byte of the source
 *    run (or of the moved window), inside d_src or the arena: d_src and
 *    d_payload are 16 B aligned and src_bytes and payload_bytes multiples of 16,
 *    else MTCP_GPU_EINVAL.
 *  - Record stores are bounded by n and max_id.
 *  - The outputs are a pure function of the inputs for any bytes in d_snd,
 *    d_dtx and d_wreq, provided the chunks of the WRITTEN requests are pairwise
 *    disjoint and none overlaps the source region.  With overlapping chunks the
 *    stores only stay bounded.
 *  - Nothing depends on what the workspace held.
 */

/* Bytes of workspace mtcp_gpu_sndwrite_dev needs (the claim words of max_id + 1
 * streams and the copy plan of n requests of api.c:1416-1456).  Host only, needs
 * no GPU.  0 if n is above MTCP_GPU_GROUP_MAX_PKTS or max_id above
 * MTCP_GPU_FLOWTAB_MAX_ID, never 0 otherwise; non-decreasing in n and max_id. */
uint64_t mtcp_gpu_sndwrite_work_bytes(uint32_t n, uint32_t max_id);

/* Bytes one copy unit moves (the memcpy of tcp_send_buffer.c:132 / :140 is cut
 * into units on the destination's 16 B grid, one wave each).  Host only. */
uint32_t mtcp_gpu_sndwrite_tile(void);

/*
 * mtcp_write's body, CopyFromUser and SBPut (api.c:1416-1567,
 * tcp_send_buffer.c:116-146) for the n requests of d_wreq.  d_snd[max_id + 1]
 * and d_dtx[max_id + 1] are read, and updated for the FULL and WRITTEN
 * requests; d_src[src_bytes] is read: device memory, or registered host memory
 * passed as its device-accessible address (the user buffers are then read over
 * PCIe); d_payload[payload_bytes] is written inside the WRITTEN requests'
 * chunks.  d_wres[n], d_seg_sid[n], d_seg_start[n + 1], d_seg_stop[n], d_nseg[1]
 * and d_total[2] are written.
 *
 * The launches: claim (two, row f17's own kernels: "none" to the claim word of
 * every request's sid, then an atomic minimum of the request index into it),
 * plan (a lane per request: the verdict, the records, the result, the table,
 * the request's copy units), scan (one workgroup), move (a wave per request,
 * which leaves at once unless the request compacts: SBPut's memmove, before any
 * byte of the batch is copied), copy (a wave per 4 KiB unit).  Asynchronous on
 * `stream` (NULL = the context's stream); allocates nothing, waits for nothing
 * and copies nothing to the host, so it can sit in a stream capture in front of
 * mtcp_gpu_data_send_dev.  No workgroup waits on another.
 * MTCP_GPU_EINVAL: NULL arguments with n != 0, d_snd not 128 B aligned, d_dtx,
 * d_wreq, d_wres, d_src, d_payload or d_work not 16 B, d_total not 8 B, the
 * table's arrays not 4 B, src_bytes or payload_bytes not a multiple of 16,
 * work_bytes below mtcp_gpu_sndwrite_work_bytes(n, max_id), n above
 * MTCP_GPU_GROUP_MAX_PKTS, max_id above MTCP_GPU_FLOWTAB_MAX_ID.  MTCP_GPU_EIO on
 * an abandoned context.  n == 0 is MTCP_GPU_OK without a launch (nothing is
 * written).
 */
int mtcp_gpu_sndwrite_dev(mtcp_gpu_ctx *ctx, const mtcp_gpu_sndwrite_req *d_wreq, uint32_t n, uint32_t max_id,
                          mtcp_gpu_ack_state *d_snd, mtcp_gpu_datagen_state *d_dtx, const void *d_src,
                          uint64_t src_bytes, void *d_payload, uint64_t payload_bytes, mtcp_gpu_sndwrite_res *d_wres,
                          uint32_t *d_seg_sid, uint32_t *d_seg_start, uint32_t *d_seg_stop, uint32_t *d_nseg,
                          uint64_t *d_total, void *d_work, uint64_t work_bytes, void *stream);

/*
 * The synchronous form (api.c:1416-1567, tcp_send_buffer.c:116-146): wreq[n],
 * src[src_bytes], wres[n], seg_sid[n], seg_start[n + 1], seg_stop[n], nseg[1] and
 * total[2] are plain host memory (src_bytes any value); the mirrors and the
 * arena stay device-resident (d_snd, d_dtx, d_payload as above).  The bytes of
 * every request that passes BAD_REQ's tests go up packed, request after request
 * at 16 B aligned offsets of len bytes each: the sum of the requests' len
 * rounded up to 16 must not exceed MTCP_GPU_SNDWRITE_HOST_MAX_BYTES, else
 * MTCP_GPU_EINVAL (split the batch).  Bounded by the context's wait limit
 * (mtcp_gpu_set_wait_limit): past it nothing of the caller's is written,
 * MTCP_GPU_ETIMEDOUT is returned and the context is ABANDONED.  MTCP_GPU_ENOMEM
 * if the table of pack offsets cannot be allocated.  The other errors as
 * mtcp_gpu_sndwrite_dev's, without the alignment of the host arrays.
 */
int mtcp_gpu_sndwrite(mtcp_gpu_ctx *ctx, const mtcp_gpu_sndwrite_req *wreq, uint32_t n, uint32_t max_id,
                      mtcp_gpu_ack_state *d_snd, mtcp_gpu_datagen_state *d_dtx, const void *src, uint64_t src_bytes,
                      void *d_payload, uint64_t payload_bytes, mtcp_gpu_sndwrite_res *wres, uint32_t *seg_sid,
                      uint32_t *seg_start, uint32_t *seg_stop, uint32_t *nseg, uint64_t total[2]);

/*
 * mtcp_gpu_sndwrite_dev, then mtcp_gpu_data_send_dev over the table it wrote
 * (d_ack and d_ack_stop NULL, n bursts), on one stream: mtcp_write down to the
 * finished frames (api.c:1458-1567, core.c:479-483, tcp_out.c:607-660, :357-449,
 * :220-354).  d_wtotal and d_wwork are the write's totals and workspace,
 * d_total and d_work the data send's; d_idx[n] is the data send's (any values:
 * every list is empty).  Every argument of both calls is checked before
 * anything is launched: the errors of both calls, n == 0 included (the data
 * send then writes seg_cap void records).
 */
int mtcp_gpu_write_send_dev(mtcp_gpu_ctx *ctx, const mtcp_gpu_sndwrite_req *d_wreq, uint32_t n, uint32_t max_id,
                            mtcp_gpu_ack_state *d_snd, mtcp_gpu_datagen_state *d_dtx, const void *d_src,
                            uint64_t src_bytes, void *d_payload, uint64_t payload_bytes, mtcp_gpu_sndwrite_res *d_wres,
                            uint32_t *d_seg_sid, uint32_t *d_seg_start, uint32_t *d_seg_stop, uint32_t *d_nseg,
                            uint64_t *d_wtotal, void *d_wwork, uint64_t wwork_bytes, const uint32_t *d_idx,
                            const mtcp_gpu_rcv_state *d_state, mtcp_gpu_ackgen_state *d_tx, uint32_t cur_ts,
                            const mtcp_gpu_tx_link *d_links, uint32_t n_links, void *d_buf, uint64_t buf_off,
                            uint64_t buf_len, uint32_t off_shift, uint32_t slot_bytes, uint16_t max_mss,
                            uint32_t flags, mtcp_gpu_tx_seg *d_seg, mtcp_gpu_desc *d_desc, uint32_t seg_cap,
                            mtcp_gpu_datagen_res *d_dres, uint64_t *d_total, uint8_t *d_status, void *d_work,
                            uint64_t work_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MTCP_GPU_SNDWRITE_H */
