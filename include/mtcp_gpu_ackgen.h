/*
 * mtcp_gpu_ackgen.h — pure-ACK tx segments from a walked rx batch (SURVEY §8
 * row f14): the piece between the walks and the frame builder.
 *
 * The receive walk (mtcp_gpu_rcvwalk.h) writes, per packet, which EnqueueACK
 * call the reference would have made (MTCP_GPU_RCV_ACK_NOW,
 * MTCP_GPU_RCV_ACK_AGGREGATE).  The reference then, once per main-loop
 * iteration, runs for every stream of its ack list:
 *
 *   EnqueueACK        mtcp/src/tcp_out.c:911-935: the count, a 6-bit bit-field
 *                     (mtcp/src/include/tcp_stream.h:117), and is_wack;
 *   WriteTCPACKList   mtcp/src/tcp_out.c:697-761: to_ack, ack_cnt plain ACKs,
 *                     then the window probe; the stream leaves the list or
 *                     stays with what no slot could be had for;
 *   SendTCPPacket     mtcp/src/tcp_out.c:220-354 with flags TCP_FLAG_ACK
 *                     [| TCP_FLAG_WACK], no payload: seq, ack_seq, the window,
 *                     need_wnd_adv, ts_lastack_sent; IPOutput's ip_id++
 *                     (mtcp/src/ip_out.c:139).
 *
 * The entry points here do that for every stream of a grouped, walked batch
 * against a device-resident array of per-stream tx records and write finished
 * mtcp_gpu_tx_seg records (mtcp_gpu_txbuild.h) with their descriptors, by the
 * conventions of mtcp_gpu_txseg.h (seg_cap, void records, d_total), ready for
 * mtcp_gpu_tx_build_dev behind them on the same stream: frames in, ACK frames
 * out, no per-packet record read back.
 *
 * Not done here: the piggy-back decrement of WriteTCPDataList
 * (tcp_out.c:642-648; WriteTCPACKList runs first, core.c, so it only ever sees
 * what a full tx ring left, and stays with the host), EnqueueACK(ACK_OPT_WACK)
 * (the sender's, tcp_out.c:430; is_wack comes in with the record),
 * UpdateTimeoutList and last_active_ts (tcp_out.c:291-292: the host's, for
 * every stream that emitted a frame), every state but ESTABLISHED.
 *
 * Plain C, as mtcp_gpu.h; MTCP_GPU_ABI_VERSION is unchanged (nothing that
 * exists changes): test for MTCP_GPU_HAS_ACKGEN.
 */
#ifndef MTCP_GPU_ACKGEN_H
#define MTCP_GPU_ACKGEN_H

#include "mtcp_gpu.h"
#include "mtcp_gpu_ackwalk.h"
#include "mtcp_gpu_group.h"
#include "mtcp_gpu_rcvwalk.h"
#include "mtcp_gpu_txbuild.h"
#include "mtcp_gpu_txseg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MTCP_GPU_HAS_ACKGEN         1
#define MTCP_GPU_ACKGEN_FRAME_LEN   66u  /* 54 + 12: MTCP_GPU_TX_SEG_FRAME_LEN(ACK, 0) */

/*
 * What SendTCPPacket and WriteTCPACKList read of one stream beyond the two
 * walks' states, 32 B: the caller's array d_tx[max_id + 1], 32 B aligned,
 * indexed by stream id like d_state and d_snd.  The caller fills and refreshes
 * it with plain copies; the host's tcp_stream stays the truth.
 *
 * A record is BAD if rsvd != 0, ack_cnt > 63 (tcp_stream.h:117), is_wack,
 * has_rcvbuf or need_wnd_adv > 1, wscale_mine > 31 (the shift at
 * tcp_out.c:301) or link >= n_links.  It is tested before anything of the
 * stream is folded: a BAD stream changes nothing and emits nothing.
 *
 * The call changes ip_id, ack_cnt, is_wack, has_rcvbuf, need_wnd_adv and
 * ts_lastack_sent.  Every other byte keeps its value.
 */
typedef struct mtcp_gpu_ackgen_state {
    uint32_t saddr, daddr;    /*  0, 4 network order, as mtcp_gpu_tx_seg                       */
    uint16_t sport, dport;    /*  8, 10 network order                                          */
    uint16_t ip_id;           /* 12 sndvar->ip_id; advanced by the frames emitted (ip_out.c:139) */
    uint8_t  ack_cnt;         /* 14 sndvar->ack_cnt, 0..63; folded and decremented             */
    uint8_t  is_wack;         /* 15 sndvar->is_wack, 0/1                                       */
    uint8_t  wscale_mine;     /* 16 sndvar->wscale_mine                                        */
    uint8_t  link;            /* 17 index into the builder's link table: nif_out / the ARP answer */
    uint8_t  has_rcvbuf;      /* 18 rcvvar->rcvbuf != NULL (tcp_in.c:555-566); set to 1 when a walked
                                    packet of the stream has verdict PUT_DROPPED, PUT_NO_ROOM or PUT_STORED */
    uint8_t  need_wnd_adv;    /* 19 cur_stream->need_wnd_adv; set as at tcp_out.c:304-306, never cleared here */
    uint32_t ts_lastack_sent; /* 20 sndvar->ts_lastack_sent: cur_ts when at least one frame was emitted */
    uint8_t  rsvd[8];         /* 24 must be 0                                                  */
} mtcp_gpu_ackgen_state;

/* status of a result; the first that applies, in this order */
enum mtcp_gpu_ackgen_status {
    MTCP_GPU_ACKGEN_NONE       = 0, /* a MISS or NONE segment, or an id above max_id: nothing of a stream is
                                       read or written */
    MTCP_GPU_ACKGEN_BAD        = 1, /* the tx record is bad */
    MTCP_GPU_ACKGEN_DEFERRED   = 2, /* the list has a host tail: d_seg_stop[j] is before the segment's end,
                                       d_ack_stop != NULL and d_ack_stop[j] is before it, or
                                       d_state[id].tcp_state != TCP_ST_ESTABLISHED.  The flags of
                                       [seg_start[j], d_seg_stop[j]) are folded into ack_cnt and has_rcvbuf
                                       is updated: the record holds what the reference holds in front of
                                       the first deferred packet.  Nothing is emitted, nothing else
                                       changes; the host finishes the list and runs its own
                                       WriteTCPACKList for the stream */
    MTCP_GPU_ACKGEN_IDLE       = 3, /* no ACK flag in the list, ack_cnt == 0 and is_wack == 0 on entry: the
                                       stream is not on the ack list.  Only has_rcvbuf may change */
    MTCP_GPU_ACKGEN_NOT_TO_ACK = 4, /* tcp_out.c:755-761: ack_cnt and is_wack are zeroed, nothing is sent */
    MTCP_GPU_ACKGEN_SENT       = 5, /* everything planned was emitted (that may be nothing: the 64th
                                       ACK_OPT_NOW of a round wraps the count to 0) */
    MTCP_GPU_ACKGEN_NO_ROOM    = 6  /* cut by the room rule: ack_cnt is what was not emitted, is_wack stays
                                       1 if the probe was not (tcp_out.c:732-735, :744-747); ip_id,
                                       ts_lastack_sent and need_wnd_adv reflect only the frames emitted */
};

/* flags of a result */
#define MTCP_GPU_ACKGEN_ON_LIST      0x1u /* the reference would have had the stream on its ack list: ack_cnt or
                                             is_wack not 0 on entry, or an EnqueueACK in the folded part */
#define MTCP_GPU_ACKGEN_NEED_WND_ADV 0x2u /* a frame of this call advertised a zero window: tcp_out.c:304-306
                                             set need_wnd_adv, whatever it was */

/* One per segment of the group's table, 16 B: d_ares[j] for j < m, m being
 * d_nseg[0] clamped to n.  The caller sizes the array for n; entries past m
 * are not written. */
typedef struct mtcp_gpu_ackgen_res {
    uint32_t first_seg;       /*  0 index of the stream's first record: the running total, also for a
                                    segment that emits nothing */
    uint8_t  n_ack;           /*  4 plain ACKs emitted */
    uint8_t  wack;            /*  5 1 if the probe was emitted */
    uint8_t  status;          /*  6 enum mtcp_gpu_ackgen_status */
    uint8_t  flags;           /*  7 MTCP_GPU_ACKGEN_* */
    uint32_t ack;             /*  8 the rcv_nxt acknowledged; 0 with NONE and BAD */
    uint16_t window;          /* 12 the wire value, MIN(rcv_wnd >> wscale_mine, 65535); 0 with NONE and BAD */
    uint16_t rsvd;            /* 14 0 */
} mtcp_gpu_ackgen_res;

/*
 * The contract.
 *
 * The fold runs over [seg_start[j], stop) in list order, stop being
 * d_seg_stop[j] clamped to the segment.  For each packet p = d_idx[position]
 * it reads d_place[p].flags and d_place[p].verdict: ACK_OPT_NOW is applied if
 * bit MTCP_GPU_RCV_ACK_NOW is set, ack_cnt = (ack_cnt + 1) & 63 (tcp_out.c:
 * 924-926: the guard is evaluated in int and always holds); then
 * ACK_OPT_AGGREGATE if bit MTCP_GPU_RCV_ACK_AGGREGATE is set, if (ack_cnt == 0)
 * ack_cnt = 1 (tcp_out.c:927-930).  The receive walk never sets both; the
 * order is fixed so that the output is a pure function of any input bytes.
 * ProcessACK enqueues nothing (only tcp_in.c:125, :157, :163, :165, :858, :860
 * do), so d_ack is not an input.
 *
 * to_ack (tcp_out.c:701-714) holds iff has_rcvbuf, after the fold, and
 * TCP_SEQ_LEQ(rcv_nxt, head_seq + merged_len).  A stream that only ever saw
 * SEQ_OLD / SEQ_AHEAD / PAWS_OLD / SEQ_WINPROBE packets has no receive buffer:
 * the reference sends no ACK for it and zeroes the count, and so does this.
 * With to_ack the plan is ack_cnt plain ACKs, then the probe if is_wack.
 *
 * Record k in global order (segments as the group's table has them; within a
 * stream the plain ACKs, then the probe) is a full mtcp_gpu_tx_seg:
 *   saddr, daddr, sport, dport, link    the tx record's
 *   seq          d_snd[id].snd_nxt as the ACK walk left it (tcp_out.c:284);
 *                snd_nxt - 1 for the probe (tcp_out.c:266)
 *   ack          d_state[id].rcv_nxt as the receive walk left it (tcp_out.c:289)
 *   ts_val       cur_ts, one value for the call; ts_ecr d_state[id].ts_recent,
 *                whatever saw_timestamp says (tcp_out.c:118-122)
 *   window       MIN(rcv_wnd >> wscale_mine, 65535) (tcp_out.c:301-302)
 *   ip_id        ip_id + i mod 2^16 for the stream's frame i (ip_out.c:139)
 *   flags 0x10 (TCP_FLAG_WACK, 0x80, never reaches the wire), form 1,
 *   payload_off, payload_len, mss, wscale 0.
 * Its descriptor is {(buf_off + k * slot) >> off_shift, 66, 0, 0}, slot being
 * slot_bytes, or ALIGN(66, A) when slot_bytes is 0, A = max(2, 1 << off_shift).
 *
 * Room, void records and totals are mtcp_gpu_txseg.h's: a record is emitted
 * iff k < seg_cap, its frame ends at or before buf_len and its offset fits 32
 * bits; the emitted records are a prefix of the planned ones; all seg_cap
 * records and descriptors are always written, the tail being 48 zero bytes
 * with form = MTCP_GPU_TXSEG_VOID_FORM and a zero descriptor; d_total[0] is
 * the records emitted, d_total[1] the bytes of the frame buffer used
 * (d_total[0] * slot).
 *
 * The commit of a stream with e frames emitted, n_ack = MIN(e, ack_cnt) of
 * them plain: ack_cnt -= n_ack (tcp_out.c:736); is_wack = 0 iff the probe was
 * emitted (tcp_out.c:741-747); ip_id += e; with e > 0, ts_lastack_sent = cur_ts
 * (tcp_out.c:290) and, where rcv_wnd >> wscale_mine is 0, need_wnd_adv = 1.
 * The payload length is 0: snd_nxt and the RTO list are not touched
 * (tcp_out.c:332-351).
 *
 * Every store is bounded by n, max_id, m and seg_cap whatever d_place,
 * d_state, d_snd, d_tx and the group arrays hold: an index in d_idx at or above
 * n is skipped, a segment whose id is above max_id is NONE.  The outputs are a
 * pure function of the inputs for any bytes in d_place, d_state, d_snd and d_tx
 * and for group arrays as mtcp_gpu_group[_dev] writes them (every stream in
 * one segment); nothing depends on what the workspace held.  Records of
 * streams absent from the batch keep every byte.
 */

/* Bytes of workspace mtcp_gpu_ackgen_dev needs (the plans of tcp_out.c:697-761
 * for n segments).  Host only, needs no GPU.  0 if n is above
 * MTCP_GPU_GROUP_MAX_PKTS or max_id above MTCP_GPU_FLOWTAB_MAX_ID, never 0
 * otherwise; non-decreasing in n and max_id. */
uint64_t mtcp_gpu_ackgen_work_bytes(uint32_t n, uint32_t max_id);

/* The longest list a lane folds by itself (the loop of tcp_out.c:911-935 over
 * one stream's packets); a longer one is folded by its wave, 64 packets a
 * step (sizing, tests). */
uint32_t mtcp_gpu_ackgen_lane_len(void);

/*
 * EnqueueACK's count, WriteTCPACKList and SendTCPPacket's records
 * (tcp_out.c:911-935, :697-761, :220-354) for every stream of a grouped,
 * walked batch.  d_place[n], d_seg_stop: what mtcp_gpu_rcvwalk_dev wrote;
 * d_ack_stop: what mtcp_gpu_ackwalk_dev wrote, or NULL; d_idx, d_seg_sid,
 * d_seg_start, d_nseg: what mtcp_gpu_group_dev wrote with the same n and
 * max_id; d_state[max_id + 1] and d_snd[max_id + 1] are read, d_tx[max_id + 1]
 * is read and updated; d_seg[seg_cap], d_desc[seg_cap], d_ares[j] for j < m
 * and d_total[2] are written.
 *
 * Asynchronous on `stream` (NULL = the context's stream); allocates nothing,
 * waits for nothing and copies nothing to the host, so it can sit in a stream
 * capture behind the walks.  No workgroup waits on another: the phases are
 * separate launches.  MTCP_GPU_EINVAL: NULL arguments (d_ack_stop may be
 * NULL; with n == 0 only d_seg, d_desc and d_total are needed), d_snd not
 * 128 B aligned, d_state not 64 B, d_tx not 32 B, d_place, d_ares or d_work
 * not 16 B, d_seg, d_desc or d_total not 8 B, the others not 4 B; work_bytes
 * below mtcp_gpu_ackgen_work_bytes(n, max_id); n above MTCP_GPU_GROUP_MAX_PKTS;
 * max_id above MTCP_GPU_FLOWTAB_MAX_ID; seg_cap 0 or above
 * MTCP_GPU_TXSEG_MAX_SEGS; off_shift above 16; n_links outside 1..256;
 * slot_bytes or buf_off not a multiple of A; slot_bytes not 0 and below 66; a
 * context opened with MTCP_GPU_F_COMPACT.  MTCP_GPU_EIO on an abandoned
 * context.  n == 0 writes seg_cap void records and zero totals.
 */
int mtcp_gpu_ackgen_dev(mtcp_gpu_ctx *ctx, const mtcp_gpu_rcv_place *d_place, uint32_t n, uint32_t max_id,
                        const uint32_t *d_idx, const uint32_t *d_seg_sid, const uint32_t *d_seg_start,
                        const uint32_t *d_nseg, const uint32_t *d_seg_stop, const uint32_t *d_ack_stop,
                        const mtcp_gpu_rcv_state *d_state, const mtcp_gpu_ack_state *d_snd, uint32_t cur_ts,
                        mtcp_gpu_ackgen_state *d_tx, uint32_t n_links, uint64_t buf_off, uint64_t buf_len,
                        uint32_t off_shift, uint32_t slot_bytes, mtcp_gpu_tx_seg *d_seg, mtcp_gpu_desc *d_desc,
                        uint32_t seg_cap, mtcp_gpu_ackgen_res *d_ares, uint64_t *d_total, void *d_work,
                        uint64_t work_bytes, void *stream);

/*
 * mtcp_gpu_ackgen_dev, then mtcp_gpu_tx_build_dev over all seg_cap records, on
 * one stream: WriteTCPACKList down to the finished frames (tcp_out.c:697-761,
 * :220-354, ip_out.c:100-167, eth_out.c:35-80).  d_status[seg_cap] is the
 * builder's; flags are its call flags (MTCP_GPU_TXB_NO_CSUM).  The builder
 * never dereferences its payload argument for payload_len == 0: it is given
 * the workspace pointer with payload_bytes = 0.  Every argument is checked
 * before anything is launched: the errors of both calls.
 */
int mtcp_gpu_ack_send_dev(mtcp_gpu_ctx *ctx, const mtcp_gpu_rcv_place *d_place, uint32_t n, uint32_t max_id,
                          const uint32_t *d_idx, const uint32_t *d_seg_sid, const uint32_t *d_seg_start,
                          const uint32_t *d_nseg, const uint32_t *d_seg_stop, const uint32_t *d_ack_stop,
                          const mtcp_gpu_rcv_state *d_state, const mtcp_gpu_ack_state *d_snd, uint32_t cur_ts,
                          mtcp_gpu_ackgen_state *d_tx, const mtcp_gpu_tx_link *d_links, uint32_t n_links,
                          void *d_buf, uint64_t buf_off, uint64_t buf_len, uint32_t off_shift,
                          uint32_t slot_bytes, uint32_t flags, mtcp_gpu_tx_seg *d_seg, mtcp_gpu_desc *d_desc,
                          uint32_t seg_cap, mtcp_gpu_ackgen_res *d_ares, uint64_t *d_total, uint8_t *d_status,
                          void *d_work, uint64_t work_bytes, void *stream);

/*
 * mtcp_gpu_ackgen_dev for host memory (tcp_out.c:911-935, :697-761, :220-354):
 * place[n], the group arrays as mtcp_gpu_group wrote them (idx[n], seg_sid[m],
 * seg_start[m + 1], nseg[1]), seg_stop[m], ack_stop[m] or NULL,
 * state[max_id + 1], snd[max_id + 1]; tx[max_id + 1] is read and written back,
 * seg[seg_cap], desc[seg_cap], ares[m] and total[2] are written.  Synchronous,
 * built like mtcp_gpu_ackwalk: the inputs go up on the context's stream, the
 * results come back; the workspace comes from the context's staging.  Bounded
 * by the context's wait limit (mtcp_gpu_set_wait_limit): past it nothing of
 * the caller's is written (tx[] included), MTCP_GPU_ETIMEDOUT is returned and
 * the context is ABANDONED.
 */
int mtcp_gpu_ackgen(mtcp_gpu_ctx *ctx, const mtcp_gpu_rcv_place *place, uint32_t n, uint32_t max_id,
                    const uint32_t *idx, const uint32_t *seg_sid, const uint32_t *seg_start, const uint32_t *nseg,
                    const uint32_t *seg_stop, const uint32_t *ack_stop, const mtcp_gpu_rcv_state *state,
                    const mtcp_gpu_ack_state *snd, uint32_t cur_ts, mtcp_gpu_ackgen_state *tx, uint32_t n_links,
                    uint64_t buf_off, uint64_t buf_len, uint32_t off_shift, uint32_t slot_bytes,
                    mtcp_gpu_tx_seg *seg, mtcp_gpu_desc *desc, uint32_t seg_cap, mtcp_gpu_ackgen_res *ares,
                    uint64_t total[2]);

#ifdef __cplusplus
}
#endif

#endif /* MTCP_GPU_ACKGEN_H */
