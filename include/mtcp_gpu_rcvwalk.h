/*
 * mtcp_gpu_rcvwalk.h — the per-stream receive walk behind the grouping
 * (SURVEY §8 row f11): the first consumer of mtcp_gpu_group.h's lists.
 *
 * Behind StreamHTSearch the reference handles a segment of an ESTABLISHED
 * stream in this order (ProcessTCPPacket, mtcp/src/tcp_in.c:1194-1209 and
 * :1256-1258):
 *
 *   ValidateSequence           mtcp/src/tcp_in.c:101-179: PAWS on the packet's
 *                              timestamps, then the window test;
 *   Handle_TCP_ST_ESTABLISHED  its payload branch, tcp_in.c:854-862;
 *   ProcessTCPPayload          mtcp/src/tcp_in.c:537-610;
 *   RBPut                      mtcp/src/tcp_ring_buffer.c:280-382: drop before
 *                              the head, no room, the fragment merge and
 *                              merged_len.
 *
 * That walk is sequential within a stream and independent across streams, the
 * shape mtcp_gpu_group[_dev] gives a batch.  The entry points here run it for
 * every stream of a grouped batch against a device-resident array of receive
 * states and write, per packet, a placement record: where RBPut would copy the
 * payload, which ACK the reference enqueues and whether it raises a read
 * event; per stream the updated state; per segment of the grouping the
 * position where the host has to take over.
 *
 * Not done here: the payload copy (the memcpy at tcp_ring_buffer.c:315 and the
 * compaction at :304-308; the placement records are its input), ProcessACK
 * (the send side; it touches no receive state), every state but ESTABLISHED
 * and the SYN / RST / FIN handling.  A packet that needs any of it is
 * DEFERRED, with every later packet of its stream in the batch: the state
 * record then holds exactly what the reference would hold before that packet.
 *
 * Plain C, as mtcp_gpu.h; MTCP_GPU_ABI_VERSION is unchanged (nothing that
 * exists changes): test for MTCP_GPU_HAS_RCVWALK.
 */
#ifndef MTCP_GPU_RCVWALK_H
#define MTCP_GPU_RCVWALK_H

#include "mtcp_gpu.h"
#include "mtcp_gpu_group.h"
#include "mtcp_gpu_tcpopt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MTCP_GPU_HAS_RCVWALK        1
#define MTCP_GPU_RCV_MAX_FRAGS      4
#define MTCP_GPU_RCV_MAX_SIZE       (1u << 30)
#define MTCP_GPU_RCV_ST_ESTABLISHED 4    /* TCP_ST_ESTABLISHED, tcp_in.h:72-82 */

/*
 * The receive state of one stream, 64 B: the caller's array d_state[max_id + 1],
 * 64 B aligned, indexed by stream id.  The caller fills and refreshes it with
 * plain copies; the host's tcp_stream stays the truth, as with the flow
 * table's mirror.  Where the reference has not allocated the ring buffer yet
 * (tcp_in.c:555-566) the record already says head_seq = irs + 1,
 * merged_len = 0, nfrag = 0.
 *
 * A record is BAD if rsvd != 0, nfrag > 4, size > 2^30, merged_len > size or
 * a live frag[k].len >= 2^31 (struct fragment_ctx keeps len in 31 bits,
 * tcp_ring_buffer.h:36).  It is tested before every packet.
 *
 * The walk changes rcv_nxt, rcv_wnd, merged_len, ts_recent, ts_lastack_rcvd,
 * nfrag and frag[]; a packet that ends PUT_STORED leaves the slots at and past
 * nfrag zero.  Every other byte keeps its value.
 */
typedef struct mtcp_gpu_rcv_frag {
    uint32_t seq;             /* fragment_ctx.seq */
    uint32_t len;             /* fragment_ctx.len */
} mtcp_gpu_rcv_frag;

typedef struct mtcp_gpu_rcv_state {
    uint32_t rcv_nxt;         /*  0 cur_stream->rcv_nxt                         */
    uint32_t rcv_wnd;         /*  4 rcvvar->rcv_wnd                             */
    uint32_t head_seq;        /*  8 rcvbuf->head_seq                            */
    uint32_t merged_len;      /* 12 rcvbuf->merged_len                          */
    uint32_t size;            /* 16 rcvbuf->size                                */
    uint32_t ts_recent;       /* 20 rcvvar->ts_recent                           */
    uint32_t ts_lastack_rcvd; /* 24 rcvvar->ts_lastack_rcvd                     */
    uint8_t  tcp_state;       /* 28 cur_stream->state, enum tcp_state tcp_in.h:72-82 */
    uint8_t  saw_timestamp;   /* 29 cur_stream->saw_timestamp                   */
    uint8_t  nfrag;           /* 30 live entries of frag[], 0..4                */
    uint8_t  rsvd;            /* 31 must be 0                                   */
    mtcp_gpu_rcv_frag frag[MTCP_GPU_RCV_MAX_FRAGS]; /* 32 rcvbuf->fctx in list order */
} mtcp_gpu_rcv_state;

/* flags of mtcp_gpu_rcv_place */
#define MTCP_GPU_RCV_COPY          0x01u /* RBPut reached its memcpy        tcp_ring_buffer.c:315 */
#define MTCP_GPU_RCV_ACK_NOW       0x02u /* EnqueueACK(ACK_OPT_NOW)         tcp_in.c:125, :165, :860 */
#define MTCP_GPU_RCV_ACK_AGGREGATE 0x04u /* EnqueueACK(ACK_OPT_AGGREGATE)   tcp_in.c:157, :163, :858 */
#define MTCP_GPU_RCV_READ_EVENT    0x08u /* tcp_in.c:593 did not fire: RaiseReadEvent, :606 */
#define MTCP_GPU_RCV_TS_NEWER      0x10u /* tcp_in.c:129 held: the host sets ts_last_ts_upd = cur_ts */

/* One value per exit of the walk. */
enum mtcp_gpu_rcv_verdict {
    /* not walked: the packet is in the grouping's MISS or NONE class; the
     * record is all zero */
    MTCP_GPU_RCV_NONE            = 0,
    /* deferred to the host: the record is all zero but for the verdict */
    MTCP_GPU_RCV_DEFER_STATE     = 1,  /* tcp_state != TCP_ST_ESTABLISHED (tcp_in.c:1232-1258) */
    MTCP_GPU_RCV_DEFER_BAD_STATE = 2,  /* the state record is bad, or RBPut's insert would
                                          follow a NULL prev (tcp_ring_buffer.c:370-372) */
    MTCP_GPU_RCV_DEFER_FLAGS     = 3,  /* SYN, RST or FIN (tcp_in.c:844, :1223, :871) */
    MTCP_GPU_RCV_DEFER_TS        = 4,  /* saw_timestamp, and d_opt is NULL or the option
                                          record is MTCP_GPU_TCPOPT_TS_UNPINNED (tcp_in.c:109) */
    MTCP_GPU_RCV_DEFER_FRAG_FULL = 5,  /* RBPut would end with a fifth fragment
                                          (tcp_ring_buffer.c:360-375 with nfrag == 4) */
    MTCP_GPU_RCV_DEFER_BEHIND    = 6,  /* an earlier packet of this stream in this batch was deferred */
    /* walked: the reference line that decides it */
    MTCP_GPU_RCV_PAWS_NO_TS      = 7,  /* tcp_in.c:109-115, no ACK                */
    MTCP_GPU_RCV_PAWS_OLD        = 8,  /* tcp_in.c:119-126, ACK_NOW               */
    MTCP_GPU_RCV_SEQ_WINPROBE    = 9,  /* tcp_in.c:152-158, ACK_AGGREGATE         */
    MTCP_GPU_RCV_SEQ_OLD         = 10, /* tcp_in.c:162-163, ACK_AGGREGATE         */
    MTCP_GPU_RCV_SEQ_AHEAD       = 11, /* tcp_in.c:164-165, ACK_NOW               */
    MTCP_GPU_RCV_ACK_ONLY        = 12, /* valid, payload_len == 0: tcp_in.c:854 not taken */
    MTCP_GPU_RCV_PUT_DROPPED     = 13, /* RBPut returns 0,  tcp_ring_buffer.c:294 */
    MTCP_GPU_RCV_PUT_NO_ROOM     = 14, /* RBPut returns -2, tcp_ring_buffer.c:299 */
    MTCP_GPU_RCV_PUT_STORED      = 15  /* RBPut copied,     tcp_ring_buffer.c:315-381 */
};

/*
 * The placement record of one packet, 16 B: d_place[n], indexed by packet like
 * d_sid.  Every one of the n records is written.  After each of the three
 * PUT_* verdicts tcp_in.c:588-593 run as in the reference: rcv_nxt and rcv_wnd
 * are recomputed from head_seq, merged_len and size, READ_EVENT and
 * ACK_AGGREGATE are set if rcv_nxt moved forward, ACK_NOW otherwise.
 */
typedef struct mtcp_gpu_rcv_place {
    uint32_t put_off;         /*  0 RBPut's putx (tcp_ring_buffer.c:297); meaningful with COPY */
    uint32_t rcv_nxt;         /*  4 the stream's after this packet                */
    uint32_t rcv_wnd;         /*  8 the stream's after this packet                */
    uint16_t put_len;         /* 12 the payload length, with COPY; else 0         */
    uint8_t  verdict;         /* 14 enum mtcp_gpu_rcv_verdict                     */
    uint8_t  flags;           /* 15 MTCP_GPU_RCV_*                                */
} mtcp_gpu_rcv_place;

/*
 * The contract.
 *
 * The comparisons are the reference's own, in the reference's order:
 * TCP_SEQ_* (tcp_in.h:37-41) in the validation; GetMinSeq / GetMaxSeq with
 * MAXSEQ/2 (tcp_ring_buffer.c:234-254) in RBPut (the two differ at a distance
 * of exactly 2^31).  CanMerge's + 1 (:259-260), the break at :352-357 and the
 * insert at :360-375 are restated literally, not replaced by an interval
 * union.  mtcp_gpu_result.verdict is not read: the lists name TCP_OK packets.
 *
 * A deferred packet changes nothing: the fifth fragment in particular is
 * found before any field is committed.  Records of streams absent from the
 * batch keep every byte.
 *
 * Every store is bounded by n, max_id and the segment table's m, clamped to
 * n, whatever d_state, d_res, d_opt and the group arrays hold: an index in
 * d_idx at or above n is skipped, a segment whose id is above max_id is not
 * walked.  The outputs are a pure function of the inputs for any bytes in
 * d_state, d_res and d_opt and for group arrays as mtcp_gpu_group[_dev] writes
 * them (every packet in one list, every stream in one segment); nothing
 * depends on what the workspace held.
 */

/* Bytes of workspace mtcp_gpu_rcvwalk_dev needs (the walk of tcp_in.c:101-179,
 * tcp_in.c:537-610 and tcp_ring_buffer.c:280-382 over n records).  Host only,
 * needs no GPU.  0 if n is above MTCP_GPU_GROUP_MAX_PKTS or max_id above
 * MTCP_GPU_FLOWTAB_MAX_ID, never 0 otherwise; non-decreasing in n and max_id. */
uint64_t mtcp_gpu_rcvwalk_work_bytes(uint32_t n, uint32_t max_id);

/* Packets of its own segment a lane walks per round; the lengths at which the
 * walker changes its path are multiples of it (sizing, tests) in the walk of
 * tcp_in.c:101-179, tcp_in.c:537-610 and tcp_ring_buffer.c:280-382. */
uint32_t mtcp_gpu_rcvwalk_short_len(void);

/*
 * Walk the streams of a grouped batch: ValidateSequence (tcp_in.c:101-179),
 * ProcessTCPPayload (tcp_in.c:537-610) and RBPut's bookkeeping
 * (tcp_ring_buffer.c:280-382) for every packet of every stream's list, in
 * list order.  d_res[n]: the 40 B records of the batch; d_opt[n]: its option
 * records, or NULL; d_idx, d_seg_sid, d_seg_start, d_nseg: what
 * mtcp_gpu_group_dev wrote for the batch with the same n and max_id.
 * d_state[max_id + 1] is read and updated, d_place[n] written, and
 * d_seg_stop[j] for j < m (the caller sizes it for n; entries past m are not
 * written): the position in d_idx of segment j's first deferred packet, or
 * the segment's end; for the MISS and NONE segments their start.
 *
 * Asynchronous on `stream` (NULL = the context's stream); allocates nothing,
 * waits for nothing and copies nothing to the host, so it can sit in a stream
 * capture behind the group launches.  MTCP_GPU_EINVAL: NULL arguments (d_opt
 * may be NULL), d_state not 64 B aligned, d_place, d_opt or d_work not 16 B
 * aligned, d_res not 8 B aligned, the others not 4 B aligned, work_bytes below
 * mtcp_gpu_rcvwalk_work_bytes(n, max_id), n above MTCP_GPU_GROUP_MAX_PKTS,
 * max_id above MTCP_GPU_FLOWTAB_MAX_ID, a context opened with
 * MTCP_GPU_F_COMPACT (16 B records carry no seq).  MTCP_GPU_EIO on an
 * abandoned context.  n == 0 is MTCP_GPU_OK without a launch.
 */
int mtcp_gpu_rcvwalk_dev(mtcp_gpu_ctx *ctx, const mtcp_gpu_result *d_res, const mtcp_gpu_tcpopt *d_opt,
                         uint32_t n, uint32_t max_id, const uint32_t *d_idx, const uint32_t *d_seg_sid,
                         const uint32_t *d_seg_start, const uint32_t *d_nseg, mtcp_gpu_rcv_state *d_state,
                         mtcp_gpu_rcv_place *d_place, uint32_t *d_seg_stop, void *d_work, uint64_t work_bytes,
                         void *stream);

/*
 * The same for host memory (tcp_in.c:101-179, tcp_in.c:537-610,
 * tcp_ring_buffer.c:280-382): res[n], opt[n] or NULL, the group arrays as
 * mtcp_gpu_group wrote them (idx[n], seg_sid[m], seg_start[m + 1], nseg[1]),
 * state[max_id + 1] read and written back, place[n] and seg_stop[m] written.
 * Synchronous, built like mtcp_gpu_group: the inputs go up on the context's
 * stream, the results come back; the workspace comes from the context's
 * staging.  Bounded by the context's wait limit (mtcp_gpu_set_wait_limit):
 * past it nothing of the caller's is written (the state array included),
 * MTCP_GPU_ETIMEDOUT is returned and the context is ABANDONED.
 */
int mtcp_gpu_rcvwalk(mtcp_gpu_ctx *ctx, const mtcp_gpu_result *res, const mtcp_gpu_tcpopt *opt, uint32_t n,
                     uint32_t max_id, const uint32_t *idx, const uint32_t *seg_sid, const uint32_t *seg_start,
                     const uint32_t *nseg, mtcp_gpu_rcv_state *state, mtcp_gpu_rcv_place *place,
                     uint32_t *seg_stop);

#ifdef __cplusplus
}
#endif

#endif /* MTCP_GPU_RCVWALK_H */
