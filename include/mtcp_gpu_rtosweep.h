/*
 * mtcp_gpu_rtosweep.h — the retransmission-timeout sweep over device send
 * states: the loss-recovery path that runs when the ACKs
 * stop coming.
 *
 * Once per main-loop iteration the reference runs (mtcp/src/core.c:800):
 *
 *   CheckRtmTimeout   mtcp/src/timer.c:363-419: walks the slots of its RTO
 *                     wheel from rto_now_ts up to cur_ts (:380), takes every
 *                     stream of a slot off the list (:394-397) and calls
 *                     HandleRTO for it, at most thresh of them (:386-388);
 *   HandleRTO         timer.c:176-337: the retransmission count and the LOST
 *                     exit (:186-206), max_nrtx (:207-209), the backed-off rto
 *                     (:212-224), ssthresh and cwnd (:234-238), snd_nxt =
 *                     snd_una (:305), and for an ESTABLISHED stream
 *                     AddtoSendList (:309);
 *   AddtoSendList     mtcp/src/tcp_out.c:837-855 as built with -DNDEBUG: no
 *                     send buffer returns (:842-848), else on_send_list = TRUE
 *                     if it was not (:850-851).
 *
 * The entry points here do that for every stream of the thread's
 * d_snd[max_id + 1] (mtcp_gpu_ackwalk.h) at one cur_ts: everything the timer
 * reads is in that mirror, kept by the ACK walk and by the data generation's
 * commit.  The fired streams come out as a group table of empty segments that
 * mtcp_gpu_datagen_dev (mtcp_gpu_datagen.h) accepts unchanged, so the timeout
 * retransmission leaves the device as finished frames (mtcp_gpu_rto_send_dev).
 *
 * Not done here: every state but ESTABLISHED (HandleRTO's SYN, FIN and
 * CLOSE_WAIT branches, control_list_waiting: timer.c:249-271, :277-334),
 * CheckTimewaitExpire and CheckConnectionTimeout (timer.c:422-502), the wheel
 * itself: the host keeps its lists and replays d_rto.
 *
 * Plain C, as mtcp_gpu.h; MTCP_GPU_ABI_VERSION is unchanged (nothing that
 * exists changes): test for MTCP_GPU_HAS_RTOSWEEP.
 */
#ifndef MTCP_GPU_RTOSWEEP_H
#define MTCP_GPU_RTOSWEEP_H

#include "mtcp_gpu.h"
#include "mtcp_gpu_ackwalk.h"
#include "mtcp_gpu_datagen.h"
#include "mtcp_gpu_txseg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MTCP_GPU_HAS_RTOSWEEP       1
#define MTCP_GPU_RTO_MAX_BACKOFF    7    /* TCP_MAX_BACKOFF, tcp_in.h:68 */
#define MTCP_GPU_RTO_ST_CLOSED      0    /* TCP_ST_CLOSED, tcp_in.h:72-82 */

/* verdict of a handled stream; the first that applies, in this order */
enum mtcp_gpu_rto_verdict {
    MTCP_GPU_RTO_NONE        = 0,  /* never written */
    MTCP_GPU_RTO_BAD         = 1,  /* the d_snd record is bad by mtcp_gpu_ackwalk.h's rule or the d_dtx record by
                                      mtcp_gpu_datagen.h's: nothing changes */
    MTCP_GPU_RTO_DEFER_STATE = 2,  /* tcp_state != 4: nothing changes, the thread runs its own HandleRTO (SYN, FIN
                                      and CLOSE_WAIT retransmissions stay with the host, timer.c:249-334) */
    MTCP_GPU_RTO_LOST        = 3,  /* nrtx >= MTCP_GPU_ACK_MAX_RTX (timer.c:186-206): on_rto = 0 (:395-397),
                                      tcp_state = 0 (:196); nothing else changes.  The thread sets close_reason and
                                      raises the error event or destroys the stream (:197-202) */
    MTCP_GPU_RTO_RETRANSMIT  = 4   /* timer.c:207-238, :305-309 */
};

/* flags of a handled stream */
#define MTCP_GPU_RTO_SEND_LIST_ADD  0x01u /* AddtoSendList listed the stream: on_send_list was 0 (tcp_out.c:850-851) */

/* One per handled stream, 16 B: d_rto[j] for j < handled, in ascending id.
 * The caller sizes the array for cap; entries past handled are not written. */
typedef struct mtcp_gpu_rto_rec {
    uint32_t sid;             /*  0 the stream's id                                             */
    uint32_t rto;             /*  4 d_snd[sid].rto after the step                               */
    uint8_t  nrtx;            /*  8 d_snd[sid].nrtx after the step: the host's max_nrtx is
                                    MAX(max_nrtx, nrtx) where the verdict is RETRANSMIT
                                    (timer.c:207-209)                                           */
    uint8_t  verdict;         /*  9 enum mtcp_gpu_rto_verdict                                   */
    uint8_t  flags;           /* 10 MTCP_GPU_RTO_*                                              */
    uint8_t  rsvd0;           /* 11 0                                                           */
    uint32_t rsvd1;           /* 12 0                                                           */
} mtcp_gpu_rto_rec;

/*
 * The contract.
 *
 * Which streams fire.  Stream id <= max_id is due iff d_snd[id].on_rto == 1 and
 * (int32_t)(cur_ts - d_snd[id].ts_rto) >= 0.  This is what the wheel gives a
 * stream that AddtoRTOList placed with 0 <= ts_rto - rto_now_ts < RTO_HASH
 * (timer.c:47-52) when the thread checks every tick (:380).  Two differences
 * from the wheel:
 *   1. Order.  Due streams are taken in ascending id, not in wheel-slot order.
 *      HandleRTO touches only its own stream and the lists, so the order only
 *      changes the position a stream gets on the send list, which the device
 *      does not keep.
 *   2. Long timeouts.  The overflow list (rto_list[RTO_HASH], RearrangeRTOStore
 *      timer.c:340-360) tests the reversed difference (:349).  The device takes
 *      ts_rto at its word instead: a stream with a timeout of RTO_HASH ticks or
 *      more fires when ts_rto is reached.
 *
 * The cap.  The first min(due, cap) due streams in ascending id are handled;
 * the rest keep every byte and fire at the next sweep: CheckRtmTimeout's
 * thresh (timer.c:386-388).  d_total[0] = due, d_total[1] = handled.
 *
 * The step for a handled stream, the first rule that applies:
 *   1. the record is BAD by mtcp_gpu_ackwalk.h's rule (rsvd != 0, eff_mss == 0,
 *      wscale_peer > 31, sb_size > 2^30, sb_len > sb_size) or the d_dtx record
 *      by mtcp_gpu_datagen.h's (rsvd != 0, a flag byte above 1): BAD, nothing
 *      changes;
 *   2. tcp_state != 4: DEFER_STATE, nothing changes;
 *   3. nrtx >= MTCP_GPU_ACK_MAX_RTX (timer.c:186-206): LOST; on_rto = 0
 *      (:395-397), tcp_state = 0 (:196), nothing else changes;
 *   4. otherwise RETRANSMIT: on_rto = 0 (:395-397); nrtx += 1 (:187); backoff =
 *      MIN(nrtx, 7) (:214); rto = ((srtt >> 3) + rttvar) << backoff in uint32_t
 *      with its wrap, and if that is 0 the previous rto stays (:216-224; rto is
 *      unsigned, so "<= 0" is "== 0"); ssthresh = MIN(cwnd, peer_wnd) / 2,
 *      raised to 2 * mss if below (:234-237); cwnd = mss (:238); snd_nxt =
 *      snd_una (:305); ts_rto keeps its value (:231 is commented out);
 *      AddtoSendList (:309, tcp_out.c:842-851 under NDEBUG): with has_sndbuf ==
 *      0 it returns without listing, otherwise d_dtx[id].on_send_list = 1, and
 *      SEND_LIST_ADD iff it was 0.
 * Every other byte of d_snd and d_dtx keeps its value.  Bytes 88-127 of a d_snd
 * record are neither read nor written.
 *
 * The table.  d_nseg[0] = handled; d_seg_sid[j] = the j-th handled id for j <
 * handled (entries past handled are not written); d_seg_start[0 .. cap] = 0;
 * d_seg_stop[0 .. cap) = 0: a group table of empty segments, one per handled
 * stream, that mtcp_gpu_datagen_dev accepts with n = cap, d_ack and d_ack_stop
 * NULL and any valid d_idx.  Behind it a RETRANSMIT stream flushes from snd_una
 * under MIN(cwnd, peer_wnd) = MIN(mss, peer_wnd), and the data generation's
 * commit arms ts_rto = cur_ts + rto with RTO_ADD.  LOST, DEFER_STATE and BAD
 * streams come out of it as DEFERRED or BAD with nothing changed.
 *
 * Replaying d_rto[j] on the host: RemoveFromRTOList (timer.c:395-397) for LOST
 * and RETRANSMIT; max_nrtx (:207-209) and, with SEND_LIST_ADD, the send list
 * insertion (tcp_out.c:850-853) for RETRANSMIT; close_reason and the error
 * event or DestroyTCPStream (:197-202) for LOST; the thread's own HandleRTO for
 * DEFER_STATE and BAD.
 *
 * Purity.  The outputs are a pure function of the inputs for any bytes in d_snd
 * and d_dtx; nothing depends on what the workspace held; every store is
 * bounded by max_id, cap and handled.
 */

/* Bytes of workspace mtcp_gpu_rto_sweep_dev needs (the due masks and counts of
 * timer.c:380's test over max_id + 1 streams).  Host only, needs no GPU.  0 if
 * cap is 0 or above MTCP_GPU_TXSEG_MAX_BURSTS or max_id above
 * MTCP_GPU_FLOWTAB_MAX_ID, never 0 otherwise; non-decreasing in both. */
uint64_t mtcp_gpu_rto_sweep_work_bytes(uint32_t max_id, uint32_t cap);

/* Streams one workgroup sweeps (timer.c:363-419 over one tile): with max_id + 1
 * and cap both at most this the sweep is a single one-workgroup launch, else
 * three launches (sizing, tests). */
uint32_t mtcp_gpu_rto_sweep_tile(void);

/*
 * CheckRtmTimeout's firing decision, HandleRTO's ESTABLISHED path and the
 * AddtoSendList it ends in (timer.c:363-419, :176-337, tcp_out.c:837-855) for
 * every stream of d_snd[max_id + 1] at cur_ts.  d_snd and d_dtx[max_id + 1] are
 * read and updated; d_rto[j] and d_seg_sid[j] for j < handled, d_seg_start[cap
 * + 1], d_seg_stop[cap], d_nseg[1] and d_total[2] are written.
 *
 * The launches: count (a lane per stream, per-wave ballots and popcounts, no
 * atomic), scan (one workgroup), emit (ranks from the ballots, the step, the
 * stores); or one workgroup doing all three where max_id + 1 and cap fit
 * mtcp_gpu_rto_sweep_tile().  Asynchronous on `stream` (NULL = the context's
 * stream); allocates nothing, waits for nothing and copies nothing to the
 * host, so it can sit in a stream capture in front of mtcp_gpu_datagen_dev.  No
 * workgroup waits on another.  MTCP_GPU_EINVAL: NULL arguments, d_snd not 128 B
 * aligned, d_dtx, d_rto or d_work not 16 B, d_total not 8 B, the others not
 * 4 B; cap 0 or above MTCP_GPU_TXSEG_MAX_BURSTS; max_id above
 * MTCP_GPU_FLOWTAB_MAX_ID; work_bytes below mtcp_gpu_rto_sweep_work_bytes(max_id,
 * cap).  MTCP_GPU_EIO on an abandoned context.
 */
int mtcp_gpu_rto_sweep_dev(mtcp_gpu_ctx *ctx, uint32_t max_id, mtcp_gpu_ack_state *d_snd,
                           mtcp_gpu_datagen_state *d_dtx, uint32_t cur_ts, uint32_t cap, mtcp_gpu_rto_rec *d_rto,
                           uint32_t *d_seg_sid, uint32_t *d_seg_start, uint32_t *d_seg_stop, uint32_t *d_nseg,
                           uint64_t *d_total, void *d_work, uint64_t work_bytes, void *stream);

/*
 * The same for host memory (timer.c:363-419, :176-337): snd and dtx[max_id + 1]
 * are read and written back; rto[handled], seg_sid[handled], seg_start[cap +
 * 1], seg_stop[cap], nseg[1] and total[2] are written.  Synchronous, built like
 * mtcp_gpu_datagen: the inputs go up on the context's stream, the results come
 * back; the workspace comes from the context's staging.  Bounded by the
 * context's wait limit (mtcp_gpu_set_wait_limit): past it nothing of the
 * caller's is written (snd[] and dtx[] included), MTCP_GPU_ETIMEDOUT is
 * returned and the context is ABANDONED.
 */
int mtcp_gpu_rto_sweep(mtcp_gpu_ctx *ctx, uint32_t max_id, mtcp_gpu_ack_state *snd, mtcp_gpu_datagen_state *dtx,
                       uint32_t cur_ts, uint32_t cap, mtcp_gpu_rto_rec *rto, uint32_t *seg_sid, uint32_t *seg_start,
                       uint32_t *seg_stop, uint32_t *nseg, uint64_t total[2]);

/*
 * mtcp_gpu_rto_sweep_dev, then mtcp_gpu_data_send_dev over the table the sweep
 * wrote, on one stream: CheckRtmTimeout down to the finished frames
 * (timer.c:363-419, :176-337; tcp_out.c:607-660, :357-449, :220-354).  The data
 * send gets d_ack and d_ack_stop NULL and n = cap; d_idx[cap] is any valid
 * array (the segments are empty: no entry is read).  d_total[2] is the sweep's
 * (due, handled), d_dtotal[2] the data send's; d_rwork with rwork_bytes is the
 * sweep's workspace, d_work with work_bytes the data send's
 * (mtcp_gpu_datagen_work_bytes(cap, max_id)).  Every argument of both calls is
 * checked before anything is launched: the errors of both.
 */
int mtcp_gpu_rto_send_dev(mtcp_gpu_ctx *ctx, uint32_t max_id, mtcp_gpu_ack_state *d_snd,
                          mtcp_gpu_datagen_state *d_dtx, uint32_t cur_ts, uint32_t cap, mtcp_gpu_rto_rec *d_rto,
                          uint32_t *d_seg_sid, uint32_t *d_seg_start, uint32_t *d_seg_stop, uint32_t *d_nseg,
                          uint64_t *d_total, void *d_rwork, uint64_t rwork_bytes, const uint32_t *d_idx,
                          const mtcp_gpu_rcv_state *d_state, mtcp_gpu_ackgen_state *d_tx, const void *d_payload,
                          uint64_t payload_bytes, const mtcp_gpu_tx_link *d_links, uint32_t n_links, void *d_buf,
                          uint64_t buf_off, uint64_t buf_len, uint32_t off_shift, uint32_t slot_bytes,
                          uint16_t max_mss, uint32_t flags, mtcp_gpu_tx_seg *d_seg, mtcp_gpu_desc *d_desc,
                          uint32_t seg_cap, mtcp_gpu_datagen_res *d_dres, uint64_t *d_dtotal, uint8_t *d_status,
                          void *d_work, uint64_t work_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MTCP_GPU_RTOSWEEP_H */
