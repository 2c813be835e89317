/*
 * mtcp_gpu_datagen.h — data tx segments from a walked rx batch (SURVEY §8 row
 * f15): the send side behind the ACK walk.
 *
 * The ACK walk (mtcp_gpu_ackwalk.h) leaves each stream's new snd_nxt, cwnd,
 * peer_wnd, snd_una and sb_len in d_snd and writes, per packet, the two send
 * list calls ProcessACK made: MTCP_GPU_ACK_FAST_RTX (AddtoSendList,
 * mtcp/src/tcp_in.c:426, tcp_out.c:850-851) and MTCP_GPU_ACK_SEND_LIST_REMOVE
 * (RemoveFromSendList, tcp_in.c:453, tcp_out.c:891-892).  The reference then,
 * once per main-loop iteration, behind its control list and its ack list
 * (mtcp/src/core.c:663-668), runs for every stream of its send list:
 *
 *   WriteTCPDataList       mtcp/src/tcp_out.c:607-660, the body for one stream:
 *                          on_control_list delays it (-1, :614-617), else the
 *                          flush; ret >= 0 takes it off the list (:639) and
 *                          lowers ack_cnt by the ACKs that rode along
 *                          (:643-650); ret < 0 keeps it listed (:633-636);
 *   FlushTCPSendingBuffer  tcp_out.c:357-449: no send buffer (:369-373 as built
 *                          with -DNDEBUG), an empty one (:377-380), window =
 *                          MIN(cwnd, peer_wnd) (:382), snd_nxt behind head_seq
 *                          (:387-394 under NDEBUG: break), buffered_len (:395),
 *                          the loop (:401-443, row f8's), the 500 ms test and
 *                          EnqueueACK(ACK_OPT_WACK) (:429-431, :931-933);
 *   SendTCPPacket          what a data segment leaves behind: ts_lastack_sent
 *                          (tcp_out.c:290), need_wnd_adv (:301-306), snd_nxt
 *                          (:332), ts_rto and AddtoRTOList (:346-350, whose
 *                          guard is mtcp/src/timer.c:37); IPOutput's ip_id++
 *                          (mtcp/src/ip_out.c:139).
 *
 * The entry points here do that for every stream of a grouped, walked batch:
 * they fold the two flags into on_send_list, make one mtcp_gpu_tx_burst per
 * segment of the group's table from the device-resident records (d_snd, d_state,
 * d_tx, and a 16 B record d_dtx that says where the send buffer's bytes lie),
 * hand the bursts to mtcp_gpu_tx_segment_dev (mtcp_gpu_txseg.h) and commit what
 * SendTCPPacket and WriteTCPDataList change afterwards.  The retransmission
 * falls out: the reference retransmits by snd_nxt = ack_seq (tcp_in.c:406) and
 * flushing from there, which is what a burst that starts at the ACK walk's
 * snd_nxt does.  Timestamps are on and SACK is off, as everywhere in this tree.
 *
 * One difference from the reference.  WriteTCPDataList breaks out of its list
 * walk at the first stream whose ret is negative (tcp_out.c:633-636), -3
 * included, and serves the rest in later loop iterations.  The call serves
 * every stream in one pass: the result of the reference run with each stream
 * alone on its send list.  Only NO_ROOM carries over to later streams: row
 * f8's rule gives them NO_ROOM with nothing emitted and nothing changed.
 *
 * Not done here: streams on the host's send list that are not in the batch
 * (the application wrote: they stay with the host, or go through
 * mtcp_gpu_tx_send_dev from host-made bursts), control_list_waiting
 * (tcp_out.c:653-657), AddtoACKList behind WACK_ENQUEUED, UpdateTimeoutList and
 * last_active_ts (tcp_out.c:291-292), the RTO list itself (RTO_ADD says that
 * the stream joined it), every state but ESTABLISHED.
 *
 * Plain C, as mtcp_gpu.h; MTCP_GPU_ABI_VERSION is unchanged (nothing that
 * exists changes): test for MTCP_GPU_HAS_DATAGEN.
 */
#ifndef MTCP_GPU_DATAGEN_H
#define MTCP_GPU_DATAGEN_H

#include "mtcp_gpu.h"
#include "mtcp_gpu_ackgen.h"
#include "mtcp_gpu_ackwalk.h"
#include "mtcp_gpu_group.h"
#include "mtcp_gpu_rcvwalk.h"
#include "mtcp_gpu_txbuild.h"
#include "mtcp_gpu_txseg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MTCP_GPU_HAS_DATAGEN        1
#define MTCP_GPU_DATAGEN_MAX_DIST   (1u << 30)  /* the largest sequence distance a burst is made from */

/*
 * Where one stream's send buffer lies, and its list membership, 16 B: the
 * caller's array d_dtx[max_id + 1], 16 B aligned, indexed by stream id like
 * d_snd.  The byte with sequence number s lies at sb_off + (uint32_t)(s -
 * sb_base_seq) in the payload arena (d_payload with payload_bytes, as
 * mtcp_gpu_tx_build_dev and mtcp_gpu_tx_segment_dev take them).  Between two of
 * the host's SBPut calls the buffer is linear and only its head moves
 * (mtcp/src/tcp_send_buffer.c:161-164), so the ACK walk's SBRemove bookkeeping
 * does not invalidate the pair; the host refreshes it after SBPut, which may
 * memmove (tcp_send_buffer.c:136-140), and after the reset at :167-170.
 *
 * A record is BAD if rsvd != 0 or a flag byte is above 1.  The call changes
 * on_send_list only.
 */
typedef struct mtcp_gpu_datagen_state {
    uint64_t sb_off;          /*  0 byte offset in the payload arena of the byte whose sequence number is sb_base_seq */
    uint32_t sb_base_seq;     /*  8 the sequence number sb_off refers to                       */
    uint8_t  on_send_list;    /* 12 sndvar->on_send_list, 0/1                                  */
    uint8_t  on_control_list; /* 13 sndvar->on_control_list, 0/1                               */
    uint8_t  rsvd[2];         /* 14 must be 0                                                  */
} mtcp_gpu_datagen_state;

/* status of a result; the first that applies, in this order */
enum mtcp_gpu_datagen_status {
    MTCP_GPU_DATAGEN_NONE         = 0,  /* a MISS or NONE segment, or an id above max_id: nothing of a stream is
                                           read or written */
    MTCP_GPU_DATAGEN_BAD          = 1,  /* the d_dtx record is bad, the d_tx record is bad by mtcp_gpu_ackgen.h's
                                           rule, or the d_snd record by mtcp_gpu_ackwalk.h's: nothing changes */
    MTCP_GPU_DATAGEN_DEFERRED     = 2,  /* the host handles the stream: d_seg_stop[j] or d_ack_stop[j] lies before
                                           the segment's end, d_state[id].tcp_state != 4 or d_snd[id].tcp_state
                                           != 4.  The fold of the walked prefix is committed to on_send_list,
                                           nothing else changes */
    MTCP_GPU_DATAGEN_IDLE         = 3,  /* not on the list after the fold; only on_send_list may have changed */
    MTCP_GPU_DATAGEN_CONTROL_WAIT = 4,  /* on_control_list: ret -1 (tcp_out.c:614-617); stays listed, nothing sent */
    MTCP_GPU_DATAGEN_NO_SNDBUF    = 5,  /* has_sndbuf == 0: tcp_out.c:369-373 under NDEBUG, ret 0 */
    MTCP_GPU_DATAGEN_EMPTY        = 6,  /* sb_len == 0: tcp_out.c:377-380, ret 0 */
    MTCP_GPU_DATAGEN_BEHIND_HEAD  = 7,  /* TCP_SEQ_LT(snd_nxt, sb_head_seq): tcp_out.c:387-394 under NDEBUG, the
                                           loop breaks, ret 0 */
    MTCP_GPU_DATAGEN_BAD_BURST    = 8,  /* snd_nxt - sb_head_seq > sb_len (the reference would read past its
                                           buffer); snd_nxt - snd_una, snd_nxt - sb_base_seq or sb_head_seq -
                                           sb_base_seq above MTCP_GPU_DATAGEN_MAX_DIST; or row f8 answers a
                                           status other than MTCP_GPU_TXS_OK for the burst (mss < 13, the payload
                                           range outside payload_bytes, ...).  The stream stays listed (the fold
                                           is committed to on_send_list), nothing else changes */
    MTCP_GPU_DATAGEN_SENT         = 9,  /* the flush ran until buffered_len == 0 (tcp_out.c:401), possibly with
                                           no segment: ret n_seg */
    MTCP_GPU_DATAGEN_WINDOW       = 10, /* row f8's STOP_WINDOW: ret -3 (tcp_out.c:433); the PEER_WINDOW bit is
                                           copied into stop */
    MTCP_GPU_DATAGEN_NO_ROOM      = 11  /* row f8's STOP_NO_ROOM: ret -2 (tcp_out.c:439-441) */
};

/* flags of a result */
#define MTCP_GPU_DATAGEN_ON_LIST_BEFORE 0x01u /* on_send_list on entry */
#define MTCP_GPU_DATAGEN_ON_LIST_AFTER  0x02u /* on_send_list as the call leaves it */
#define MTCP_GPU_DATAGEN_RTO_ADD        0x04u /* AddtoRTOList took the stream in: on_rto was 0 (timer.c:37) */
#define MTCP_GPU_DATAGEN_WACK_ENQUEUED  0x08u /* EnqueueACK(ACK_OPT_WACK) ran (tcp_out.c:429-431): is_wack is 1,
                                                 the host runs AddtoACKList */
#define MTCP_GPU_DATAGEN_NEED_WND_ADV   0x10u /* a segment of this call advertised a zero window (tcp_out.c:304-306) */

/* One per segment of the group's table, 16 B: d_dres[j] for j < m, m being
 * d_nseg[0] clamped to n.  The caller sizes the array for n; entries past m
 * are not written.  With NONE and BAD flags is 0. */
typedef struct mtcp_gpu_datagen_res {
    uint32_t first_seg;       /*  0 index of the stream's first record: the running total, as row f8's result */
    uint32_t n_seg;           /*  4 records emitted */
    uint32_t bytes;           /*  8 payload bytes in them: what snd_nxt advanced by */
    uint8_t  status;          /* 12 enum mtcp_gpu_datagen_status */
    uint8_t  stop;            /* 13 MTCP_GPU_TXS_STOP_* bits of row f8's result; 0 unless SENT, WINDOW or NO_ROOM */
    uint8_t  flags;           /* 14 MTCP_GPU_DATAGEN_* */
    uint8_t  rsvd;            /* 15 0 */
} mtcp_gpu_datagen_res;

/*
 * The contract.
 *
 * Which streams.  Every segment of the group's table, as mtcp_gpu_ackgen_dev:
 * the streams that received packets in this batch.  Bursts are in the table's
 * order.
 *
 * The fold (tcp_in.c:426, :453; tcp_out.c:850-851, :891-892) runs over
 * [d_seg_start[j], stop) in list order, stop being d_ack_stop[j] clamped to the
 * segment.  For each packet p = d_idx[position] (an index at or above n is
 * skipped) d_ack[p].flags is applied: MTCP_GPU_ACK_SEND_LIST_REMOVE sets
 * on_send_list = 0, then MTCP_GPU_ACK_FAST_RTX sets it to 1 (the ACK walk never
 * sets both; the order is fixed so that the result is a pure function of any
 * bytes).  d_ack and d_ack_stop may both be NULL (both or neither): the fold is
 * then the identity.  Only the 4 B holding flags are read of a record.
 *
 * The burst of a stream whose status is SENT, WINDOW or NO_ROOM, as row f8
 * reads it (tcp_out.c:382, :385, :395, :404-405; :284, :289, :301-302;
 * :118-122):
 *   seq          d_snd.snd_nxt               len        sb_head_seq + sb_len - snd_nxt
 *   in_flight    snd_nxt - snd_una           window     MIN(cwnd, peer_wnd)
 *   peer_wnd     d_snd.peer_wnd              mss        d_snd.mss
 *   payload_off  sb_off + (uint32_t)(snd_nxt - sb_base_seq), mod 2^64
 *   ack          d_state.rcv_nxt             ts_val     cur_ts
 *   ts_ecr       d_state.ts_recent           tcp_window MIN(rcv_wnd >> wscale_mine, 65535)
 *   saddr, daddr, sport, dport, link, ip_id  d_tx's
 * Every other segment of the table (and every index from m to n - 1) gets a
 * burst of len 0 that row f8 accepts as OK.  Records, descriptors, room, void
 * records and d_total are row f8's (mtcp_gpu_txseg.h) for these n bursts.
 *
 * The commit, e being the n_seg and bytes the bytes of row f8's result:
 *   SENT, WINDOW, NO_ROOM: d_snd.snd_nxt += bytes (tcp_out.c:332).  With e > 0:
 *     d_snd.ts_rto = cur_ts + rto (:346), d_snd.on_rto = 1 and RTO_ADD iff on_rto
 *     was 0 (timer.c:37); d_tx.ip_id += e (ip_out.c:139); d_tx.ts_lastack_sent =
 *     cur_ts (:290); d_tx.need_wnd_adv = 1 and NEED_WND_ADV where rcv_wnd >>
 *     wscale_mine == 0 (:304-306).
 *   WINDOW with PEER_WINDOW: TS_TO_MSEC(cur_ts - ts_lastack_sent) > 500 literally
 *     in uint32_t, ((cur_ts - t) * 1000u) / 1000u with its wrap
 *     (mtcp/src/include/tcp_in.h:44-50), t being ts_lastack_sent as the burst's
 *     own segments left it: cur_ts when e > 0, which makes the test false.  If it
 *     holds, d_tx.is_wack = 1 and WACK_ENQUEUED (tcp_out.c:429-431, :931-933).
 *   ret >= 0 (SENT: e; NO_SNDBUF, EMPTY, BEHIND_HEAD: 0): on_send_list = 0
 *     (:639); if ack_cnt > 0, ack_cnt = ack_cnt > ret ? ack_cnt - ret : 0, ret an
 *     int (:643-650).
 *   ret < 0 (CONTROL_WAIT -1, WINDOW -3, NO_ROOM -2): on_send_list stays 1, no
 *     decrement, also where segments went out before the -3 (:633-636).
 * Every other byte of d_snd, d_tx and d_dtx keeps its value; d_state is only
 * read.
 *
 * Every store is bounded by n, max_id, m and seg_cap whatever the records and
 * the group arrays hold: an index in d_idx at or above n is skipped, a segment
 * whose id is above max_id is NONE.  The outputs are a pure function of the
 * inputs for any bytes in d_ack, d_state, d_snd, d_tx and d_dtx and for group
 * arrays as mtcp_gpu_group[_dev] writes them (every stream in one segment);
 * nothing depends on what the workspace held.  Records of streams absent from
 * the batch keep every byte.
 */

/* Bytes of workspace mtcp_gpu_datagen_dev needs: the n bursts, row f8's n
 * results, the parked statuses and row f8's own workspace.  Host only, needs no
 * GPU.  0 if n is above MTCP_GPU_TXSEG_MAX_BURSTS (one burst per index; below
 * MTCP_GPU_GROUP_MAX_PKTS) or max_id above MTCP_GPU_FLOWTAB_MAX_ID, never 0
 * otherwise; non-decreasing in n and max_id. */
uint64_t mtcp_gpu_datagen_work_bytes(uint32_t n, uint32_t max_id);

/* The longest list a lane folds by itself (tcp_in.c:426, :453 over one stream's
 * packets); a longer one is folded by its wave, 64 packets a step (sizing,
 * tests). */
uint32_t mtcp_gpu_datagen_lane_len(void);

/*
 * WriteTCPDataList's body and FlushTCPSendingBuffer (tcp_out.c:607-660,
 * :357-449) for every stream of a grouped, walked batch.  d_ack[n], d_ack_stop:
 * what mtcp_gpu_ackwalk_dev wrote, or NULL for both; d_idx, d_seg_sid,
 * d_seg_start, d_nseg: what mtcp_gpu_group_dev wrote with the same n and
 * max_id; d_seg_stop: what mtcp_gpu_rcvwalk_dev wrote; d_state[max_id + 1] is
 * read; d_snd, d_tx and d_dtx[max_id + 1] are read and updated; d_seg[seg_cap],
 * d_desc[seg_cap], d_dres[j] for j < m and d_total[2] are written.
 *
 * The launches: one burst kernel (a lane per segment), row f8's own
 * (mtcp_gpu_tx_segment_dev over n bursts), one commit kernel (a lane per
 * segment).  Asynchronous on `stream` (NULL = the context's stream); allocates
 * nothing, waits for nothing and copies nothing to the host, so it can sit in
 * a stream capture behind mtcp_gpu_ack_send_dev.  No workgroup waits on
 * another.  MTCP_GPU_EINVAL: NULL arguments (d_ack and d_ack_stop may both be
 * NULL; with n == 0 only d_seg, d_desc, d_total and d_work are needed), one of
 * d_ack and d_ack_stop NULL and the other not, d_snd not 128 B aligned, d_state
 * not 64 B, d_tx not 32 B, d_ack, d_dtx, d_dres or d_work not 16 B, d_seg,
 * d_desc or d_total not 8 B, the others not 4 B; work_bytes below
 * mtcp_gpu_datagen_work_bytes(n, max_id); n above MTCP_GPU_TXSEG_MAX_BURSTS;
 * max_id above MTCP_GPU_FLOWTAB_MAX_ID; seg_cap 0 or above
 * MTCP_GPU_TXSEG_MAX_SEGS; off_shift above 16; n_links outside 1..256;
 * slot_bytes or buf_off not a multiple of A = max(2, 1 << off_shift); slot_bytes
 * not 0 and below 67 (the smallest data frame); a context opened with
 * MTCP_GPU_F_COMPACT.  MTCP_GPU_EIO on an abandoned context.  n == 0 writes
 * seg_cap void records and zero totals.  max_mss 0 means 1460.
 */
int mtcp_gpu_datagen_dev(mtcp_gpu_ctx *ctx, const mtcp_gpu_ack_rec *d_ack, const uint32_t *d_ack_stop, uint32_t n,
                         uint32_t max_id, const uint32_t *d_idx, const uint32_t *d_seg_sid,
                         const uint32_t *d_seg_start, const uint32_t *d_nseg, const uint32_t *d_seg_stop,
                         const mtcp_gpu_rcv_state *d_state, mtcp_gpu_ack_state *d_snd, mtcp_gpu_ackgen_state *d_tx,
                         mtcp_gpu_datagen_state *d_dtx, uint32_t cur_ts, uint64_t payload_bytes, uint32_t n_links,
                         uint64_t buf_off, uint64_t buf_len, uint32_t off_shift, uint32_t slot_bytes,
                         uint16_t max_mss, mtcp_gpu_tx_seg *d_seg, mtcp_gpu_desc *d_desc, uint32_t seg_cap,
                         mtcp_gpu_datagen_res *d_dres, uint64_t *d_total, void *d_work, uint64_t work_bytes,
                         void *stream);

/*
 * mtcp_gpu_datagen_dev, then mtcp_gpu_tx_build_dev over all seg_cap records, on
 * one stream: WriteTCPDataList down to the finished frames (tcp_out.c:607-660,
 * :357-449, :220-354, ip_out.c:100-167, eth_out.c:35-80).  d_payload: the
 * arena the send buffers live in; d_status[seg_cap] is the builder's; flags are
 * its call flags (MTCP_GPU_TXB_NO_CSUM).  Every argument is checked before
 * anything is launched: the errors of both calls.
 */
int mtcp_gpu_data_send_dev(mtcp_gpu_ctx *ctx, const mtcp_gpu_ack_rec *d_ack, const uint32_t *d_ack_stop, uint32_t n,
                           uint32_t max_id, const uint32_t *d_idx, const uint32_t *d_seg_sid,
                           const uint32_t *d_seg_start, const uint32_t *d_nseg, const uint32_t *d_seg_stop,
                           const mtcp_gpu_rcv_state *d_state, mtcp_gpu_ack_state *d_snd, mtcp_gpu_ackgen_state *d_tx,
                           mtcp_gpu_datagen_state *d_dtx, uint32_t cur_ts, const void *d_payload,
                           uint64_t payload_bytes, const mtcp_gpu_tx_link *d_links, uint32_t n_links, void *d_buf,
                           uint64_t buf_off, uint64_t buf_len, uint32_t off_shift, uint32_t slot_bytes,
                           uint16_t max_mss, uint32_t flags, mtcp_gpu_tx_seg *d_seg, mtcp_gpu_desc *d_desc,
                           uint32_t seg_cap, mtcp_gpu_datagen_res *d_dres, uint64_t *d_total, uint8_t *d_status,
                           void *d_work, uint64_t work_bytes, void *stream);

/*
 * mtcp_gpu_datagen_dev for host memory (tcp_out.c:607-660, :357-449): ack[n]
 * and ack_stop[m], or NULL for both; the group arrays as mtcp_gpu_group wrote
 * them (idx[n], seg_sid[m], seg_start[m + 1], nseg[1]), seg_stop[m],
 * state[max_id + 1]; snd, tx and dtx[max_id + 1] are read and written back,
 * seg[seg_cap], desc[seg_cap], dres[m] and total[2] are written.  Synchronous,
 * built like mtcp_gpu_ackgen: the inputs go up on the context's stream, the
 * results come back; the workspace comes from the context's staging.  Bounded
 * by the context's wait limit (mtcp_gpu_set_wait_limit): past it nothing of
 * the caller's is written (snd[], tx[] and dtx[] included), MTCP_GPU_ETIMEDOUT
 * is returned and the context is ABANDONED.
 */
int mtcp_gpu_datagen(mtcp_gpu_ctx *ctx, const mtcp_gpu_ack_rec *ack, const uint32_t *ack_stop, uint32_t n,
                     uint32_t max_id, const uint32_t *idx, const uint32_t *seg_sid, const uint32_t *seg_start,
                     const uint32_t *nseg, const uint32_t *seg_stop, const mtcp_gpu_rcv_state *state,
                     mtcp_gpu_ack_state *snd, mtcp_gpu_ackgen_state *tx, mtcp_gpu_datagen_state *dtx, uint32_t cur_ts,
                     uint64_t payload_bytes, uint32_t n_links, uint64_t buf_off, uint64_t buf_len,
                     uint32_t off_shift, uint32_t slot_bytes, uint16_t max_mss, mtcp_gpu_tx_seg *seg,
                     mtcp_gpu_desc *desc, uint32_t seg_cap, mtcp_gpu_datagen_res *dres, uint64_t total[2]);

#ifdef __cplusplus
}
#endif

#endif /* MTCP_GPU_DATAGEN_H */
