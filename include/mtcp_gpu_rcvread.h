/*
 * mtcp_gpu_rcvread.h — the batched application read out of device receive
 * buffers: the consumer of the merged runs that
 * mtcp_gpu_rcvwalk.h and mtcp_gpu_rcvcopy.h leave in the arena.
 *
 * What the reference does for one mtcp_read / mtcp_recv on an ESTABLISHED
 * stream:
 *
 *   CopyToUser   mtcp/src/api.c:1114-1149: copylen = MIN(merged_len, len)
 *                (:1121), EAGAIN where that is 0 (:1122-1125), the memcpy from
 *                rcvbuf->head (:1129), RBRemove (:1130), rcv_wnd = size -
 *                merged_len (:1131) and the window-advertisement decision
 *                (:1134-1145);
 *   PeekForUser  api.c:1096-1112: the same copy with nothing removed (MSG_PEEK);
 *   RBRemove     mtcp/src/tcp_ring_buffer.c:384-421: head_offset, head_seq,
 *                merged_len, last_len, and the first fragment freed (:403-411)
 *                or trimmed (:412-415).
 *
 * The entry points here do that for a batch of read requests, one per stream,
 * against the mirrors the receive chain keeps: d_state (mtcp_gpu_rcvwalk.h),
 * d_rbuf and the arena (mtcp_gpu_rcvcopy.h), need_wnd_adv in d_tx
 * (mtcp_gpu_ackgen.h) and eff_mss in d_snd (mtcp_gpu_ackwalk.h).  The next
 * batch's walk and copy then see the advanced window and head_offset with no
 * host refresh in between.
 *
 * Not done here: the ackq and the window-update ACK itself (api.c:1136-1142 are
 * replayed by the host from the result's WND_ADV), epoll events, blocking
 * reads, the FIN_WAIT and CLOSE_WAIT reads of mtcp_recv (api.c:1180-1200),
 * mtcp_readv's further CopyToUser calls on one stream (one request per stream
 * and batch; the others come back DUP).
 *
 * Plain C, as mtcp_gpu.h; MTCP_GPU_ABI_VERSION is unchanged (nothing that
 * exists changes): test for MTCP_GPU_HAS_RCVREAD.
 */
#ifndef MTCP_GPU_RCVREAD_H
#define MTCP_GPU_RCVREAD_H

#include "mtcp_gpu.h"
#include "mtcp_gpu_ackgen.h"
#include "mtcp_gpu_ackwalk.h"
#include "mtcp_gpu_rcvcopy.h"
#include "mtcp_gpu_rcvwalk.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MTCP_GPU_HAS_RCVREAD          1

/* flags of a request */
#define MTCP_GPU_RCVREAD_PEEK         0x1u  /* MSG_PEEK: PeekForUser, api.c:1096-1112 */
#define MTCP_GPU_RCVREAD_ON_ACKQ      0x2u  /* the host's sndvar->on_ackq (api.c:1136), which the device does not mirror */

/* The synchronous form gathers the bytes into one stage of the context's
 * staging: the sum over the requests of len rounded up to 16 is at most this. */
#define MTCP_GPU_RCVREAD_HOST_MAX_BYTES (32u << 20)

/* One read, 32 B: the caller's array d_req[n], 16 B aligned. */
typedef struct mtcp_gpu_rcvread_req {
    uint32_t sid;             /*  0 the stream's id                                        */
    uint32_t len;             /*  4 the application's buffer length: CopyToUser's len      */
    uint64_t dst_off;         /*  8 where the bytes go, as a byte offset into the destination region */
    uint32_t flags;           /* 16 MTCP_GPU_RCVREAD_PEEK | MTCP_GPU_RCVREAD_ON_ACKQ       */
    uint32_t rsvd[3];         /* 20 must be 0                                              */
} mtcp_gpu_rcvread_req;

/* verdict of a request; the first that applies, in this order */
enum mtcp_gpu_rcvread_verdict {
    MTCP_GPU_RCVREAD_NONE        = 0,  /* never written */
    MTCP_GPU_RCVREAD_BAD_REQ     = 1,  /* sid > max_id, a reserved word or an unknown flag set, or dst_off +
                                          MIN(len, d_rbuf[sid].size) > dst_bytes: nothing changes */
    MTCP_GPU_RCVREAD_DUP         = 2,  /* an earlier request of the batch names the same sid: nothing changes */
    MTCP_GPU_RCVREAD_BAD_STATE   = 3,  /* the records do not describe a readable buffer (below): nothing changes */
    MTCP_GPU_RCVREAD_DEFER_STATE = 4,  /* tcp_state != 4: nothing changes, the host reads itself */
    MTCP_GPU_RCVREAD_EAGAIN      = 5,  /* copylen == 0 (api.c:1103-1106, :1122-1125): nothing changes */
    MTCP_GPU_RCVREAD_PEEKED      = 6,  /* PeekForUser: copylen bytes copied, nothing else changes */
    MTCP_GPU_RCVREAD_READ        = 7   /* CopyToUser: copylen bytes copied, RBRemove, rcv_wnd, the advertisement */
};

/* flags of a result */
#define MTCP_GPU_RCVREAD_MORE         0x1u  /* merged_len > 0 after the call: the level-triggered EPOLLIN test, api.c:1248-1251 */
#define MTCP_GPU_RCVREAD_WND_ADV      0x2u  /* api.c:1134-1142 fired: need_wnd_adv was cleared; the host replays
                                               on_ackq = TRUE, StreamEnqueue(ackq) and wakeup_flag */
#define MTCP_GPU_RCVREAD_FRAG_FREED   0x4u  /* RBRemove freed the first fragment (tcp_ring_buffer.c:403-411): the host
                                               replays RBFragEnqueue */

/* One per request, 16 B: d_rres[n], 16 B aligned, every one written. */
typedef struct mtcp_gpu_rcvread_res {
    uint32_t sid;             /*  0 the request's sid                                      */
    uint32_t copylen;         /*  4 bytes copied: what mtcp_read returns; 0 unless PEEKED or READ */
    uint32_t rcv_wnd;         /*  8 d_state[sid].rcv_wnd after the call; 0 with BAD_REQ, DUP and BAD_STATE */
    uint8_t  verdict;         /* 12 enum mtcp_gpu_rcvread_verdict                          */
    uint8_t  flags;           /* 13 MTCP_GPU_RCVREAD_MORE | _WND_ADV | _FRAG_FREED; 0 with BAD_REQ, DUP and BAD_STATE */
    uint16_t rsvd;            /* 14 0                                                      */
} mtcp_gpu_rcvread_res;

/*
 * The contract.
 *
 * The run.  A stream's in-order bytes are the merged_len bytes at data_off +
 * head_offset of the arena (rcvbuf->head, api.c:1109 and :1129).  copylen =
 * MIN(d_state[sid].merged_len, len) (api.c:1102, :1121).
 *
 * The verdict of request i, the first rule that applies:
 *
 *  1. BAD_REQ.  sid > max_id; a reserved word or a flag other than PEEK and
 *     ON_ACKQ is set; or dst_off + MIN(len, d_rbuf[sid].size) > dst_bytes.  The
 *     last test uses len and the record's size, not copylen: whether a request
 *     is refused does not depend on how many bytes have arrived.
 *  2. DUP.  A request j < i has the same sid (whatever j's own verdict is, as
 *     long as its sid <= max_id).  The lowest index wins; the host runs the
 *     others in the next batch or itself.
 *  3. BAD_STATE.  d_state[sid] is BAD by mtcp_gpu_rcvwalk.h's rule (rsvd != 0,
 *     nfrag > 4, size > 2^30, merged_len > size, a live frag[k].len >= 2^31);
 *     d_rbuf[sid] is BAD by mtcp_gpu_rcvcopy.h's rule (rsvd != 0, size == 0 or
 *     above 2^30, data_off + size > arena_bytes, head_offset > tail_offset,
 *     tail_offset > size, last_len != tail_offset - head_offset); the two size
 *     fields differ; merged_len > last_len; merged_len > 0 with nfrag == 0;
 *     merged_len > 0 with frag[0].seq != head_seq (with merged_len == 0 the
 *     first fragment may lie ahead of head_seq, a hole at the head: that is
 *     EAGAIN, as in the reference); copylen > frag[0].len, the reference's
 *     assert(0) (tcp_ring_buffer.c:416-418).
 *  4. DEFER_STATE.  d_state[sid].tcp_state != MTCP_GPU_RCV_ST_ESTABLISHED: the
 *     mirrors are kept for ESTABLISHED streams only.
 *  5. EAGAIN.  copylen == 0.
 *  6. PEEKED (the request has PEEK).  copylen bytes of the run are copied to
 *     [dst_off, dst_off + copylen) of the destination; nothing else changes.
 *  7. READ.  The same copy, then RBRemove (tcp_ring_buffer.c:395-415):
 *       d_rbuf[sid]:  head_offset += copylen, last_len -= copylen;
 *       d_state[sid]: head_seq += copylen in uint32_t with its wrap, merged_len
 *                     -= copylen, rcv_wnd = size - merged_len (api.c:1131);
 *       fragments:    copylen == frag[0].len: the entries shift down, nfrag
 *                     drops by one, the freed slot is zero, FRAG_FREED; else
 *                     frag[0].seq += copylen, frag[0].len -= copylen;
 *       advertisement (api.c:1134-1145): if d_tx and d_snd are not NULL,
 *                     d_tx[sid].need_wnd_adv == 1, rcv_wnd > d_snd[sid].eff_mss
 *                     and the request's ON_ACKQ is clear, d_tx[sid].need_wnd_adv
 *                     = 0 and WND_ADV.  Byte 19 is the only byte of d_tx that is
 *                     written, eff_mss the only field of d_snd that is read.
 *     Every other byte of the records keeps its value.
 *
 * The result record.  sid as given.  With DEFER_STATE, EAGAIN, PEEKED and READ
 * rcv_wnd is d_state[sid].rcv_wnd after the call and MORE says merged_len > 0
 * after the call.  With BAD_REQ, DUP and BAD_STATE copylen, rcv_wnd and flags
 * are 0.
 *
 * Totals.  d_total[0] = the requests that copied (PEEKED or READ), d_total[1]
 * = the bytes they copied.
 *
 * Replaying d_rres[i] on the host: the return value is copylen, or -1 with
 * EAGAIN; with READ the host's tcp_ring_buffer takes RBRemove's five
 * assignments (or runs RBRemove itself: it gives the same), with FRAG_FREED
 * RBFragEnqueue on the first fragment; rcvvar->rcv_wnd = rcv_wnd; with WND_ADV
 * api.c:1137-1142; with MORE the read event is raised again where the socket
 * is level-triggered (api.c:1248-1251).  BAD_REQ, DUP, BAD_STATE and
 * DEFER_STATE: the thread runs its own mtcp_read.
 *
 * Bounds.
 *  - Every store of destination bytes lands inside [dst_off, dst_off +
 *    copylen) of a PEEKED or READ request, which lies inside dst_bytes.  Bytes
 *    next to a range keep their value: the two edges of a range are written
 *    with byte, short and dword stores, never by reading and rewriting a 16 B
 *    piece, because another request's range may end there and be written at
 *    the same time.
 *  - Every load of arena bytes stays inside the aligned 16 B pieces that hold a
 *    byte of the run, which lie inside the arena: d_arena is 16 B aligned and
 *    arena_bytes a multiple of 16, else MTCP_GPU_EINVAL.  The arena is never
 *    written.
 *  - Record stores are bounded by n and max_id.
 *  - The outputs are a pure function of the inputs for any bytes in d_state,
 *    d_rbuf, d_tx, d_snd and d_req, provided the destination ranges of the
 *    PEEKED and READ requests are pairwise disjoint.  With overlapping ranges
 *    the stores only stay bounded.
 *  - Nothing depends on what the workspace held.
 */

/* Bytes of workspace mtcp_gpu_rcvread_dev needs (the claim words of max_id + 1
 * streams and the copy plan of n requests of api.c:1114-1149).  Host only, needs
 * no GPU.  0 if n is above MTCP_GPU_GROUP_MAX_PKTS or max_id above
 * MTCP_GPU_FLOWTAB_MAX_ID, never 0 otherwise; non-decreasing in n and max_id. */
uint64_t mtcp_gpu_rcvread_work_bytes(uint32_t n, uint32_t max_id);

/* Bytes one copy unit moves (the memcpy of api.c:1129 is cut into units on the
 * destination's 16 B grid, one wave each): a run spans as many waves as it has
 * units (sizing, tests).  Host only. */
uint32_t mtcp_gpu_rcvread_tile(void);

/*
 * CopyToUser / PeekForUser and RBRemove (api.c:1096-1149,
 * tcp_ring_buffer.c:384-421) for the n requests of d_req.  d_state[max_id + 1]
 * and d_rbuf[max_id + 1] are read, and updated for the READ requests; d_tx
 * [max_id + 1] (byte 19 only) and d_snd[max_id + 1] (eff_mss only) may both be
 * NULL: no advertisement decision is taken then.  d_arena[arena_bytes] is read;
 * d_dst[dst_bytes] is written: device memory, or registered host memory passed
 * as its device-accessible address (the user buffers are then written over
 * PCIe).  d_rres[n] and d_total[2] are written.
 *
 * The launches: claim (two: "none" to the claim word of every request's sid,
 * then an atomic minimum of the request index into it; the workspace is never
 * cleared as a whole), plan (a lane per request: the verdict, the records, the
 * request's copy units), scan (one workgroup), copy (a wave per unit).
 * Asynchronous on `stream` (NULL = the context's stream); allocates nothing,
 * waits for nothing and copies nothing to the host, so it can sit in a stream
 * capture behind mtcp_gpu_rcvcopy_dev.  No workgroup waits on another.
 * MTCP_GPU_EINVAL: NULL arguments with n != 0 (d_tx and d_snd may be NULL, but only both),
 * d_state not 64 B aligned, d_snd not 128 B, d_rbuf or d_tx not 32 B, d_req,
 * d_rres, d_arena, d_dst or d_work not 16 B, d_total not 8 B, arena_bytes not a
 * multiple of 16, work_bytes below mtcp_gpu_rcvread_work_bytes(n, max_id), n
 * above MTCP_GPU_GROUP_MAX_PKTS, max_id above MTCP_GPU_FLOWTAB_MAX_ID.
 * MTCP_GPU_EIO on an abandoned context.  n == 0 is MTCP_GPU_OK without a launch
 * (d_total is not written).
 */
int mtcp_gpu_rcvread_dev(mtcp_gpu_ctx *ctx, const mtcp_gpu_rcvread_req *d_req, uint32_t n, uint32_t max_id,
                         mtcp_gpu_rcv_state *d_state, mtcp_gpu_rcv_buf *d_rbuf, mtcp_gpu_ackgen_state *d_tx,
                         const mtcp_gpu_ack_state *d_snd, const void *d_arena, uint64_t arena_bytes, void *d_dst,
                         uint64_t dst_bytes, mtcp_gpu_rcvread_res *d_rres, uint64_t *d_total, void *d_work,
                         uint64_t work_bytes, void *stream);

/*
 * The synchronous form (api.c:1096-1149, tcp_ring_buffer.c:384-421): req[n],
 * dst[dst_bytes], rres[n] and total[2] are plain host memory; the mirrors and
 * the arena stay device-resident (d_state, d_rbuf, d_tx, d_snd, d_arena as
 * above), as mtcp_gpu_flowtab_lookup keeps its table.  The requests go up, the
 * bytes are gathered into the context's staging, request after request at
 * 16 B aligned offsets of len bytes each, and that gather and the records come
 * down in one copy; the bytes of the PEEKED and READ requests are then copied
 * to dst + dst_off.  What comes down is therefore the sum of the requests' len
 * rounded up to 16, not dst_bytes: it must not exceed
 * MTCP_GPU_RCVREAD_HOST_MAX_BYTES, else MTCP_GPU_EINVAL (split the batch).
 * Bounded by the context's wait limit (mtcp_gpu_set_wait_limit): past it
 * nothing of the caller's is written, MTCP_GPU_ETIMEDOUT is returned and the
 * context is ABANDONED.  MTCP_GPU_ENOMEM if the table of gather offsets cannot
 * be allocated.  The other errors as mtcp_gpu_rcvread_dev's, without
 * the alignment of req, dst, rres and total.
 */
int mtcp_gpu_rcvread(mtcp_gpu_ctx *ctx, const mtcp_gpu_rcvread_req *req, uint32_t n, uint32_t max_id,
                     mtcp_gpu_rcv_state *d_state, mtcp_gpu_rcv_buf *d_rbuf, mtcp_gpu_ackgen_state *d_tx,
                     const mtcp_gpu_ack_state *d_snd, const void *d_arena, uint64_t arena_bytes, void *dst,
                     uint64_t dst_bytes, mtcp_gpu_rcvread_res *rres, uint64_t total[2]);

#ifdef __cplusplus
}
#endif

#endif /* MTCP_GPU_RCVREAD_H */
