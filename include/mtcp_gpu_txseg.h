/*
 * mtcp_gpu_txseg.h — cutting send bursts into tx segments on the device
 * (SURVEY §8 row f8).
 *
 * In the reference FlushTCPSendingBuffer (mtcp/src/tcp_out.c:357-449) walks one
 * stream's send buffer: while bytes are buffered it takes the next
 * min(len, maxlen) of them (tcp_out.c:407-411), tests them against the window
 * (tcp_out.c:421) and hands them to SendTCPPacket (tcp_out.c:437), which
 * mtcp_gpu_tx_build* of mtcp_gpu_txbuild.h restates per segment.
 * WriteTCPDataList (tcp_out.c:587-674) runs that walk for every stream of the
 * send list.  Given a stream's snapshot the walk is arithmetic, and the entry
 * points here take it over: one 64 B burst record per stream in; the 48 B
 * segment records, their descriptors (the slot layout included) and one
 * result per burst out, on the device, ready for mtcp_gpu_tx_build_dev behind
 * them on the same stream.
 *
 * For a burst (timestamps on, SACK off, as everywhere in this tree):
 *   maxlen    = mss - 12: mss - CalculateOptionLength(TCP_FLAG_ACK)
 *               (tcp_out.c:21-60, :360)
 *   window    = MIN(cwnd, peer_wnd) (tcp_out.c:382), in_flight = snd_nxt -
 *               snd_una, len = buffered_len (tcp_out.c:395)
 *   segment j = 0, 1, ... carries p_j = min(len - sent, maxlen) bytes
 *               (tcp_out.c:407-411), sent being the bytes of segments 0 .. j-1;
 *               it is sent iff in_flight + sent + p_j <= window (tcp_out.c:421);
 *               otherwise the walk stops with -3 (tcp_out.c:433): stop bit
 *               WINDOW, and PEER_WINDOW as well where in_flight + sent + p_j >
 *               peer_wnd (tcp_out.c:423).  There the reference considers a
 *               window probe (EnqueueACK(..., ACK_OPT_WACK) after its 500 ms
 *               test, tcp_out.c:429-431): that test and the enqueue stay with
 *               the caller.
 *   every segment is SendTCPPacket(..., TCP_FLAG_ACK, data, len)
 *               (tcp_out.c:437): form 1, flags ACK alone, no PSH, with
 *                 seq          seq + sent mod 2^32 (tcp_out.c:284, :332)
 *                 ip_id        ip_id + j mod 2^16 (ip_out.c:139)
 *                 payload_off  payload_off + sent (tcp_out.c:404-405; the send
 *                              buffer is linear)
 *                 payload_len  p_j; wscale 0; every other field the burst's.
 *   IPOutput returning NULL where get_wptr has no room (tcp_out.c:238-240,
 *               result -2, tcp_out.c:439-441) ends the walk with the burst part
 *               sent, and WriteTCPDataList stops (tcp_out.c:633-636): running
 *               out of room here (below) does the same, stop bit NO_ROOM.
 * The window test is 64-bit here.  The reference's u32 arithmetic differs only
 * where in_flight + len >= 2^32, which no send buffer reaches: such a burst is
 * refused (BAD_BURST).  Nor is the reference's behaviour for mss <= 12
 * reproduced (maxlen 0 or wrapped, len cut to u16, SendTCPPacket's ERROR):
 * BAD_BURST.
 *
 * Plain C, as mtcp_gpu.h; MTCP_GPU_ABI_VERSION is unchanged (nothing that
 * exists changes): test for MTCP_GPU_HAS_TXSEG.
 */
#ifndef MTCP_GPU_TXSEG_H
#define MTCP_GPU_TXSEG_H

#include "mtcp_gpu_txbuild.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MTCP_GPU_HAS_TXSEG              1
#define MTCP_GPU_TXSEG_MAX_BURSTS       (1u << 24)
#define MTCP_GPU_TXSEG_MAX_SEGS         (1u << 26)
#define MTCP_GPU_TXSEG_VOID_FORM        0xFFu   /* form of a void record: BAD_SEG to the builder */

/* per-burst status; the first that applies, in this order */
#define MTCP_GPU_TXS_OK                 0
#define MTCP_GPU_TXS_BAD_BURST          1   /* a reserved field not 0; mss < 13; mss - 12 > max_mss + 12 (the
                                               builder would refuse such a payload); a full frame 66 + (mss - 12)
                                               above 65 535 B, or above slot_bytes with fixed slots;
                                               link >= n_links; in_flight + len > 0xFFFFFFFF */
#define MTCP_GPU_TXS_BAD_PAYLOAD        2   /* payload_off + len > payload_bytes */

/* stop bits of a result */
#define MTCP_GPU_TXS_STOP_WINDOW        0x1u    /* the reference's -3 (tcp_out.c:433) */
#define MTCP_GPU_TXS_STOP_PEER_WINDOW   0x2u    /* with WINDOW: tcp_out.c:423 holds as well */
#define MTCP_GPU_TXS_STOP_NO_ROOM       0x4u    /* the reference's -2 (tcp_out.c:439-441) */

/* One stream of the send list: what FlushTCPSendingBuffer reads of it
 * (tcp_out.c:357-449) and what SendTCPPacket adds per segment (tcp_out.c:224-300). */
typedef struct mtcp_gpu_tx_burst {   /* 64 B, 8 B aligned */
    uint64_t payload_off;            /*  0 byte offset of snd_nxt's byte in the payload buffer, any alignment */
    uint32_t saddr, daddr;           /*  8, 12 network order */
    uint16_t sport, dport;           /* 16, 18 network order */
    uint32_t seq, ack;               /* 20, 24 host order: snd_nxt, rcv_nxt */
    uint32_t ts_val, ts_ecr;         /* 28, 32 */
    uint32_t len;                    /* 36 buffered_len (tcp_out.c:395) */
    uint32_t in_flight;              /* 40 snd_nxt - snd_una */
    uint32_t window;                 /* 44 MIN(cwnd, peer_wnd) (tcp_out.c:382) */
    uint32_t peer_wnd;               /* 48 */
    uint16_t tcp_window;             /* 52 the value for the wire, as mtcp_gpu_tx_seg.window */
    uint16_t ip_id;                  /* 54 sndvar->ip_id before the burst */
    uint16_t mss;                    /* 56 sndvar->mss */
    uint8_t  link;                   /* 58 */
    uint8_t  rsvd0;                  /* 59 must be 0 */
    uint32_t rsvd1;                  /* 60 must be 0 */
} mtcp_gpu_tx_burst;

typedef struct mtcp_gpu_tx_burst_result {  /* 16 B */
    uint32_t first_seg;   /* index of the burst's first record (the running total, also for a burst with none) */
    uint32_t n_seg;       /* records emitted: the caller's ip_id += n_seg */
    uint32_t bytes;       /* payload bytes in them: snd_nxt += bytes */
    uint8_t  status;      /* MTCP_GPU_TXS_OK, _BAD_BURST, _BAD_PAYLOAD */
    uint8_t  stop;        /* MTCP_GPU_TXS_STOP_* bits */
    uint16_t rsvd;        /* 0 */
} mtcp_gpu_tx_burst_result;

/*
 * Status.  A burst with a non-zero status emits nothing.  len == 0 is OK with
 * no segments (tcp_out.c:401).
 *
 * Slots.  The segment with global index k (bursts in order, a burst's segments
 * in order) gets the descriptor {offset, len = 66 + p_k, 0, 0}, offset being
 * its byte offset >> off_shift.  A = max(2, 1 << off_shift).  With slot_bytes
 * == 0 the slots are packed, byte offset buf_off + sum over j < k of
 * ALIGN(66 + p_j, A): the PSIO layout (pslib.c:146).  Otherwise the byte offset
 * is buf_off + k * slot_bytes.  slot_bytes and buf_off are multiples of A.
 *
 * Room.  A segment is emitted iff its index is below seg_cap, its frame ends
 * at or before buf_len (byte offset + 66 + p_k <= buf_len) and its offset fits
 * 32 bits.  All three are monotone in k: the emitted segments are a prefix of
 * the planned sequence.  The burst that is cut, and every burst after it that
 * had segments planned, gets NO_ROOM and no other stop bit (the reference
 * returns -2 before it reaches the window test that would have stopped the
 * burst); n_seg and bytes count only what was emitted.
 *
 * Void records.  All seg_cap records and descriptors are always written: the
 * first `total` hold segments, records [total, seg_cap) are 48 zero bytes but
 * for form = MTCP_GPU_TXSEG_VOID_FORM, with an all-zero descriptor, for which
 * mtcp_gpu_tx_build_dev answers MTCP_GPU_TXB_BAD_SEG without touching a slot.
 * So seg_cap may come from any upper bound, and the builder may run over
 * seg_cap records without anything read back.
 *
 * total[0]: segments emitted; total[1]: bytes of the frame buffer used beyond
 * buf_off: where the next slot would begin (sum of ALIGN(66 + p_k, A) over the
 * emitted segments, or total[0] * slot_bytes).
 */

/*
 * FlushTCPSendingBuffer's walk (tcp_out.c:357-449) over n_burst streams as
 * WriteTCPDataList runs it (tcp_out.c:587-674), on the host, in closed form
 * per burst: the results and totals mtcp_gpu_tx_segment_dev produces for the
 * same arguments, without a context or a GPU.  What a caller advances snd_nxt
 * and ip_id from without waiting for a copy back.  max_mss 0 means 1460.
 * MTCP_GPU_EINVAL: NULL arguments (burst, res with n_burst; total), off_shift
 * above 16, n_links outside 1..256, seg_cap 0 or above 2^26, n_burst above
 * 2^24, slot_bytes or buf_off not a multiple of A.
 */
int mtcp_gpu_tx_segment_plan(const mtcp_gpu_tx_burst *burst, uint32_t n_burst, uint64_t payload_bytes,
                             uint32_t n_links, uint64_t buf_off, uint64_t buf_len, uint32_t off_shift,
                             uint32_t slot_bytes, uint32_t seg_cap, uint16_t max_mss,
                             mtcp_gpu_tx_burst_result *res, uint64_t total[2]);

/* Bursts per workgroup of the plan pass (for sizing tests); a batch of at most
 * this many bursts and 4 096 records runs as one workgroup in one launch. */
uint32_t mtcp_gpu_tx_segment_tile(void);

/* Bytes of d_work that mtcp_gpu_tx_segment_dev needs for n_burst bursts
 * (0: n_burst above 2^24). */
uint64_t mtcp_gpu_tx_segment_work_bytes(uint32_t n_burst);

/*
 * The same walk (tcp_out.c:357-449, :587-674) on the device: d_seg[seg_cap],
 * d_desc[seg_cap], d_res[n_burst] and d_total[2] are written as stated above.
 * Asynchronous on `stream` (NULL = the context's stream); allocates nothing
 * and waits for nothing, so it can sit in a stream capture.  No workgroup
 * waits on another: the passes are separate launches.
 * MTCP_GPU_EINVAL: NULL arguments; misaligned arguments (d_burst, d_seg,
 * d_desc, d_res, d_total 8 B, d_work 16 B); off_shift above 16; n_links
 * outside 1..256; seg_cap 0 or above 2^26; n_burst above 2^24; slot_bytes or
 * buf_off not a multiple of A; work_bytes below mtcp_gpu_tx_segment_work_bytes.
 * MTCP_GPU_EIO on an abandoned context.  n_burst == 0 writes seg_cap void
 * records and zero totals.
 */
int mtcp_gpu_tx_segment_dev(mtcp_gpu_ctx *ctx, const mtcp_gpu_tx_burst *d_burst, uint32_t n_burst,
                            uint64_t payload_bytes, uint32_t n_links, uint64_t buf_off, uint64_t buf_len,
                            uint32_t off_shift, uint32_t slot_bytes, uint16_t max_mss,
                            mtcp_gpu_tx_seg *d_seg, mtcp_gpu_desc *d_desc, uint32_t seg_cap,
                            mtcp_gpu_tx_burst_result *d_res, uint64_t *d_total,
                            void *d_work, uint64_t work_bytes, void *stream);

/*
 * mtcp_gpu_tx_segment_dev, then mtcp_gpu_tx_build_dev over all seg_cap
 * records, on one stream: WriteTCPDataList's walk down to the finished frames
 * (tcp_out.c:587-674, :357-449, :224-354).  d_status[seg_cap] is the
 * builder's; flags are its call flags (MTCP_GPU_TXB_NO_CSUM).  Every argument
 * is checked before anything is launched: the errors of both calls.
 */
int mtcp_gpu_tx_send_dev(mtcp_gpu_ctx *ctx, const mtcp_gpu_tx_burst *d_burst, uint32_t n_burst,
                         const void *d_payload, uint64_t payload_bytes,
                         const mtcp_gpu_tx_link *d_links, uint32_t n_links,
                         void *d_buf, uint64_t buf_off, uint64_t buf_len, uint32_t off_shift,
                         uint32_t slot_bytes, uint16_t max_mss, uint32_t flags,
                         mtcp_gpu_tx_seg *d_seg, mtcp_gpu_desc *d_desc, uint32_t seg_cap,
                         mtcp_gpu_tx_burst_result *d_res, uint64_t *d_total, uint8_t *d_status,
                         void *d_work, uint64_t work_bytes, void *stream);

/*
 * The same for host memory (tcp_out.c:587-674, :357-449, :224-354).
 * Synchronous, built like mtcp_gpu_tx_build: bursts, payload and links go up
 * on the context's stream; the frames come back into pinned staging, and the
 * calling thread copies the bytes of the built frames, and no others, into
 * buf.  desc[seg_cap], status[seg_cap], res[n_burst] and total[2] are written.
 * Bounded by the context's wait limit (mtcp_gpu_set_wait_limit): past it
 * nothing of the caller's memory is written, MTCP_GPU_ETIMEDOUT is returned and
 * the context is ABANDONED.
 */
int mtcp_gpu_tx_send(mtcp_gpu_ctx *ctx, const mtcp_gpu_tx_burst *burst, uint32_t n_burst,
                     const void *payload, uint64_t payload_bytes,
                     const mtcp_gpu_tx_link *links, uint32_t n_links,
                     void *buf, uint64_t buf_off, uint64_t buf_len, uint32_t off_shift,
                     uint32_t slot_bytes, uint16_t max_mss, uint32_t flags,
                     mtcp_gpu_desc *desc, uint32_t seg_cap, mtcp_gpu_tx_burst_result *res,
                     uint64_t total[2], uint8_t *status);

#ifdef __cplusplus
}
#endif

#endif /* MTCP_GPU_TXSEG_H */
