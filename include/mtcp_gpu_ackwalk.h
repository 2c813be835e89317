/*
 * mtcp_gpu_ackwalk.h — the per-stream ProcessACK walk behind the receive walk
 * (SURVEY §8 row f13): the send side of the stateful tail of an ESTABLISHED
 * stream.
 *
 * For a packet that passed ValidateSequence the reference runs, behind the
 * payload branch that mtcp_gpu_rcvwalk.h restates
 * (Handle_TCP_ST_ESTABLISHED, mtcp/src/tcp_in.c:864-869):
 *
 *   ProcessACK                 mtcp/src/tcp_in.c:302-531: the window update, the
 *                              duplicate-ACK count, fast retransmit, the
 *                              recovery of snd_nxt, the congestion window,
 *                              SBRemove's bookkeeping
 *                              (mtcp/src/tcp_send_buffer.c:149-173);
 *   EstimateRTT                mtcp/src/tcp_in.c:249-300, and rto at :479;
 *   UpdateRetransmissionTimer  mtcp/src/timer.c:149-173.
 *
 * ProcessACK reads no receive state but ts_lastack_rcvd, which for a packet
 * that passed ValidateSequence on a timestamped stream is the packet's own
 * ts_ref (tcp_in.c:138); the receive walk reads no send state.  So all of a
 * stream's receive steps followed by all of its ACK steps give the reference's
 * interleaved result: the lists of mtcp_gpu_group.h, the placement records of
 * mtcp_gpu_rcvwalk.h and the option records are the whole input.  The entry
 * points here run ProcessACK for every stream of a grouped batch against a
 * device-resident array of send states and write, per packet, an ACK record
 * (what SBRemove removed and every side effect the host has to replay), per
 * stream the updated state, per segment the position where the host's own
 * ProcessACK takes over.
 *
 * Not done here: every state but ESTABLISHED (the fss adjustment at
 * tcp_in.c:322-330 with it), SYN / RST / FIN, SACK (disabled in the
 * reference, tcp_in.c:437-440), the retransmission that FAST_RTX asks for,
 * HandleRTO.  A packet that needs any of it is DEFERRED, with every later
 * packet of its stream in the batch: the state record then holds exactly what
 * the reference would hold before that packet.
 *
 * Plain C, as mtcp_gpu.h; MTCP_GPU_ABI_VERSION is unchanged (nothing that
 * exists changes): test for MTCP_GPU_HAS_ACKWALK.
 */
#ifndef MTCP_GPU_ACKWALK_H
#define MTCP_GPU_ACKWALK_H

#include "mtcp_gpu.h"
#include "mtcp_gpu_group.h"
#include "mtcp_gpu_rcvwalk.h"
#include "mtcp_gpu_tcpopt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MTCP_GPU_HAS_ACKWALK        1
#define MTCP_GPU_ACK_MAX_SIZE       (1u << 30)
#define MTCP_GPU_ACK_ST_ESTABLISHED 4    /* TCP_ST_ESTABLISHED, tcp_in.h:72-82 */
#define MTCP_GPU_ACK_MAX_RTX        16   /* TCP_MAX_RTX, tcp_in.h:66 */

/*
 * The send state of one stream, 128 B: the caller's array d_snd[max_id + 1],
 * 128 B aligned, indexed by stream id.  The caller fills and refreshes it with
 * plain copies; the host's tcp_stream stays the truth.  Bytes 88-127 are the
 * caller's: never read, never written.
 *
 * A record is BAD if rsvd != 0, eff_mss == 0 (the division at tcp_in.c:470),
 * wscale_peer > 31 (the shift at tcp_in.c:317), sb_size > 2^30 or
 * sb_len > sb_size.  It is tested before every packet.
 *
 * The walk changes what the reference changes: snd_nxt, snd_una, snd_wnd,
 * peer_wnd, snd_wl1, snd_wl2, last_ack_seq, cwnd, ssthresh, rto, ts_rto, srtt,
 * mdev, mdev_max, rttvar, rtt_seq, sb_head_seq, sb_len, dup_acks, nrtx and
 * on_rto (0 or 1 once written).  Every other byte keeps its value.
 */
typedef struct mtcp_gpu_ack_state {
    uint32_t snd_nxt;         /*  0 cur_stream->snd_nxt                          */
    uint32_t snd_una;         /*  4 sndvar->snd_una                              */
    uint32_t snd_wnd;         /*  8 sndvar->snd_wnd                              */
    uint32_t peer_wnd;        /* 12 sndvar->peer_wnd                             */
    uint32_t snd_wl1;         /* 16 rcvvar->snd_wl1                              */
    uint32_t snd_wl2;         /* 20 rcvvar->snd_wl2                              */
    uint32_t last_ack_seq;    /* 24 rcvvar->last_ack_seq                         */
    uint32_t cwnd;            /* 28 sndvar->cwnd                                 */
    uint32_t ssthresh;        /* 32 sndvar->ssthresh                             */
    uint32_t rto;             /* 36 sndvar->rto                                  */
    uint32_t ts_rto;          /* 40 sndvar->ts_rto                               */
    uint32_t srtt;            /* 44 rcvvar->srtt                                 */
    uint32_t mdev;            /* 48 rcvvar->mdev                                 */
    uint32_t mdev_max;        /* 52 rcvvar->mdev_max                             */
    uint32_t rttvar;          /* 56 rcvvar->rttvar                               */
    uint32_t rtt_seq;         /* 60 rcvvar->rtt_seq                              */
    uint32_t sb_head_seq;     /* 64 sndvar->sndbuf->head_seq                     */
    uint32_t sb_len;          /* 68 sndvar->sndbuf->len                          */
    uint32_t sb_size;         /* 72 sndvar->sndbuf->size                         */
    uint16_t mss;             /* 76 sndvar->mss                                  */
    uint16_t eff_mss;         /* 78 sndvar->eff_mss                              */
    uint8_t  tcp_state;       /* 80 cur_stream->state, enum tcp_state tcp_in.h:72-82 */
    uint8_t  saw_timestamp;   /* 81 cur_stream->saw_timestamp                    */
    uint8_t  wscale_peer;     /* 82 sndvar->wscale_peer                          */
    uint8_t  dup_acks;        /* 83 rcvvar->dup_acks                             */
    uint8_t  nrtx;            /* 84 sndvar->nrtx                                 */
    uint8_t  on_rto;          /* 85 cur_stream->on_rto_idx >= 0                  */
    uint8_t  has_sndbuf;      /* 86 sndvar->sndbuf != NULL, tcp_in.c:865         */
    uint8_t  rsvd;            /* 87 must be 0                                    */
    uint8_t  user[40];        /* 88 the caller's: never read, never written      */
} mtcp_gpu_ack_state;

/* flags of mtcp_gpu_ack_rec: one bit per side effect the host has to replay */
#define MTCP_GPU_ACK_WND_UPDATE        0x0001u /* the window update was taken      tcp_in.c:341-349 */
#define MTCP_GPU_ACK_WRITE_EVENT_WND   0x0002u /* RaiseWriteEvent                  tcp_in.c:362 */
#define MTCP_GPU_ACK_DUP               0x0004u /* dup = TRUE                       tcp_in.c:382 */
#define MTCP_GPU_ACK_FAST_RTX          0x0008u /* fast retransmit, AddtoSendList   tcp_in.c:392-426 */
#define MTCP_GPU_ACK_SND_NXT_RECOVERED 0x0010u /* snd_nxt = ack_seq                tcp_in.c:451 */
#define MTCP_GPU_ACK_SEND_LIST_REMOVE  0x0020u /* RemoveFromSendList               tcp_in.c:453 */
#define MTCP_GPU_ACK_WRITE_EVENT_ROOM  0x0040u /* RaiseWriteEvent                  tcp_in.c:521 */
#define MTCP_GPU_ACK_RTO_REMOVE        0x0080u /* RemoveFromRTOList                timer.c:157-159 */
#define MTCP_GPU_ACK_RTO_ADD           0x0100u /* ts_rto set, AddtoRTOList         timer.c:162-166 */

/* One value per exit of the walk. */
enum mtcp_gpu_ack_verdict {
    /* not walked: the packet is in the grouping's MISS or NONE class; the
     * record is all zero */
    MTCP_GPU_ACK_NONE            = 0,
    /* deferred to the host: the record is all zero but for the verdict */
    MTCP_GPU_ACK_DEFER_RCV       = 1,  /* the placement record's verdict is a DEFER_* or NONE
                                          (anything but 7-15), or the packet is valid on a
                                          saw_timestamp stream and has no timestamp record
                                          (tcp_in.c:138 has no ts_ref to take) */
    MTCP_GPU_ACK_DEFER_STATE     = 2,  /* tcp_state != TCP_ST_ESTABLISHED (tcp_in.c:322-330, :1232-1258) */
    MTCP_GPU_ACK_DEFER_BAD_STATE = 3,  /* the state record is bad */
    MTCP_GPU_ACK_DEFER_FLAGS     = 4,  /* SYN, RST or FIN (tcp_in.c:844, :1223, :871) */
    MTCP_GPU_ACK_DEFER_ARITH     = 5,  /* the reference's int arithmetic would overflow or divide
                                          by zero: mss * packets > INT_MAX at tcp_in.c:490,
                                          packets * mss * mss > INT_MAX or cwnd == 0 at
                                          tcp_in.c:495-497 */
    MTCP_GPU_ACK_DEFER_BEHIND    = 6,  /* an earlier packet of this stream in this batch was deferred */
    /* walked: the reference line that decides it */
    MTCP_GPU_ACK_NOT_VALID       = 7,  /* ValidateSequence returned FALSE (placement verdicts
                                          7-11): tcp_in.c:1256 is not reached */
    MTCP_GPU_ACK_NO_ACK_FLAG     = 8,  /* tcp_in.c:864 not taken */
    MTCP_GPU_ACK_NO_SNDBUF       = 9,  /* tcp_in.c:865 not taken */
    MTCP_GPU_ACK_ACK_BEYOND      = 10, /* the return at tcp_in.c:332-338 */
    MTCP_GPU_ACK_ACK_OLD         = 11, /* the return at tcp_in.c:459-461 */
    MTCP_GPU_ACK_ACK_NEW         = 12  /* tcp_in.c:464-528 */
};

/*
 * The ACK record of one packet, 16 B: d_ack[n], indexed by packet like
 * d_place.  Every one of the n records is written.  A walked record carries
 * the stream's snd_nxt, cwnd and dup_acks after the packet.
 */
typedef struct mtcp_gpu_ack_rec {
    uint32_t rmlen;           /*  0 what SBRemove removed at tcp_in.c:511, else 0 */
    uint32_t snd_nxt;         /*  4 the stream's after this packet                */
    uint32_t cwnd;            /*  8 the stream's after this packet                */
    uint16_t flags;           /* 12 MTCP_GPU_ACK_*                                */
    uint8_t  verdict;         /* 14 enum mtcp_gpu_ack_verdict                     */
    uint8_t  dup_acks;        /* 15 the stream's after this packet                */
} mtcp_gpu_ack_rec;

/*
 * The contract.
 *
 * The arithmetic is the reference's own, in the reference's order, on a copy
 * of the state that is committed at the packet's exit; a deferred packet
 * commits nothing.  The tests run in this order: DEFER_BEHIND, the BAD test,
 * DEFER_STATE, DEFER_FLAGS, DEFER_RCV, NOT_VALID, tcp_in.c:864, tcp_in.c:865,
 * then ProcessACK; DEFER_ARITH is found where the reference would evaluate
 * the expression (a slow-start step whose guard at tcp_in.c:489 fails
 * multiplies nothing and is walked).
 *
 * TCP_SEQ_* (tcp_in.h:37-41) wherever the reference uses them.  cwindow is
 * window << wscale_peer in 32 bits (tcp_in.c:315-318; SYN is deferred).
 * right_wnd_edge is taken before the window update (tcp_in.c:319).  dup_acks
 * is a uint8_t whose "+ 1 >" test (tcp_in.c:379) is evaluated in int and
 * always holds: the count wraps from 255 to 0, and passes 3 again.  packets is
 * a uint16_t (tcp_in.c:467-473): the quotient is truncated to 16 bits.
 * EstimateRTT (tcp_in.c:249-300) runs with a 64-bit signed m and truncating
 * uint32_t stores, on the packet's own ts_ref (tcp_in.c:138, :477-478), with
 * snd_una as it was before tcp_in.c:512 and snd_nxt as tcp_in.c:406 and :451
 * left it; rto = (srtt >> 3) + rttvar (tcp_in.c:479); a stream without
 * timestamps keeps its rto (tcp_in.c:481-484).  MIN(cwnd, peer_wnd) / 2,
 * 2 * mss and 3 * mss at tcp_in.c:411-415 and the two wrap guards at
 * tcp_in.c:430 and :489 are in 32 bits unsigned.  snd_wnd_prev <= 0 on an
 * unsigned (tcp_in.c:519) means == 0.  SBRemove (tcp_send_buffer.c:149-173)
 * removes MIN(rmlen, sb_len).  UpdateRetransmissionTimer (timer.c:149-173)
 * zeroes nrtx, leaves the RTO list if on_rto, and with
 * TCP_SEQ_GT(snd_nxt, snd_una) sets ts_rto = cur_ts + rto and joins it again.
 *
 * Every store is bounded by n, max_id and the segment table's m, clamped to
 * n, whatever d_snd, d_res, d_opt, d_place and the group arrays hold: an index
 * in d_idx at or above n is skipped, a segment whose id is above max_id is not
 * walked.  The outputs are a pure function of the inputs for any bytes in
 * d_snd, d_res, d_opt and d_place and for group arrays as mtcp_gpu_group[_dev]
 * writes them; nothing depends on what the workspace held.  Records of
 * streams absent from the batch keep every byte.
 */

/* Bytes of workspace mtcp_gpu_ackwalk_dev needs (the walk of tcp_in.c:302-531
 * over n records).  Host only, needs no GPU.  0 if n is above
 * MTCP_GPU_GROUP_MAX_PKTS or max_id above MTCP_GPU_FLOWTAB_MAX_ID, never 0
 * otherwise; non-decreasing in n and max_id. */
uint64_t mtcp_gpu_ackwalk_work_bytes(uint32_t n, uint32_t max_id);

/* Packets of its own segment a lane walks per round; the lengths at which the
 * walker of tcp_in.c:302-531 changes its path are multiples of it (sizing,
 * tests). */
uint32_t mtcp_gpu_ackwalk_short_len(void);

/*
 * Walk the streams of a grouped batch: ProcessACK (tcp_in.c:302-531) for every
 * packet of every stream's list, in list order.  d_res[n]: the 40 B records of
 * the batch; d_opt[n]: its option records, or NULL; d_place[n]: what
 * mtcp_gpu_rcvwalk_dev wrote for the batch; d_idx, d_seg_sid, d_seg_start,
 * d_nseg: what mtcp_gpu_group_dev wrote for it with the same n and max_id.
 * cur_ts: one value for the call, as RunMainLoop takes the time once per
 * iteration (core.c:760-773).  d_snd[max_id + 1] is read and updated, d_ack[n]
 * written, and d_ack_stop[j] for j < m (the caller sizes it for n; entries
 * past m are not written): the position in d_idx of segment j's first deferred
 * packet, or the segment's end; for the MISS and NONE segments their start.
 *
 * Asynchronous on `stream` (NULL = the context's stream); allocates nothing,
 * waits for nothing and copies nothing to the host, so it can sit in a stream
 * capture behind the receive walk.  MTCP_GPU_EINVAL: NULL arguments (d_opt may
 * be NULL), d_snd not 128 B aligned, d_ack, d_place, d_opt or d_work not 16 B
 * aligned, d_res not 8 B aligned, the others not 4 B aligned, work_bytes below
 * mtcp_gpu_ackwalk_work_bytes(n, max_id), n above MTCP_GPU_GROUP_MAX_PKTS,
 * max_id above MTCP_GPU_FLOWTAB_MAX_ID, a context opened with
 * MTCP_GPU_F_COMPACT (16 B records carry no seq).  MTCP_GPU_EIO on an
 * abandoned context.  n == 0 is MTCP_GPU_OK without a launch.
 */
int mtcp_gpu_ackwalk_dev(mtcp_gpu_ctx *ctx, const mtcp_gpu_result *d_res, const mtcp_gpu_tcpopt *d_opt,
                         const mtcp_gpu_rcv_place *d_place, uint32_t n, uint32_t max_id, const uint32_t *d_idx,
                         const uint32_t *d_seg_sid, const uint32_t *d_seg_start, const uint32_t *d_nseg,
                         uint32_t cur_ts, mtcp_gpu_ack_state *d_snd, mtcp_gpu_ack_rec *d_ack, uint32_t *d_ack_stop,
                         void *d_work, uint64_t work_bytes, void *stream);

/*
 * The same for host memory (tcp_in.c:302-531): res[n], opt[n] or NULL,
 * place[n] as mtcp_gpu_rcvwalk wrote it, the group arrays as mtcp_gpu_group
 * wrote them (idx[n], seg_sid[m], seg_start[m + 1], nseg[1]), snd[max_id + 1]
 * read and written back, ack[n] and ack_stop[m] written.  Synchronous, built
 * like mtcp_gpu_rcvwalk: the inputs go up on the context's stream, the results
 * come back; the workspace comes from the context's staging.  Bounded by the
 * context's wait limit (mtcp_gpu_set_wait_limit): past it nothing of the
 * caller's is written (the state array included), MTCP_GPU_ETIMEDOUT is
 * returned and the context is ABANDONED.
 */
int mtcp_gpu_ackwalk(mtcp_gpu_ctx *ctx, const mtcp_gpu_result *res, const mtcp_gpu_tcpopt *opt,
                     const mtcp_gpu_rcv_place *place, uint32_t n, uint32_t max_id, const uint32_t *idx,
                     const uint32_t *seg_sid, const uint32_t *seg_start, const uint32_t *nseg, uint32_t cur_ts,
                     mtcp_gpu_ack_state *snd, mtcp_gpu_ack_rec *ack, uint32_t *ack_stop);

#ifdef __cplusplus
}
#endif

#endif /* MTCP_GPU_ACKWALK_H */
