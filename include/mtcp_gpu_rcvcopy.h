/*
 * mtcp_gpu_rcvcopy.h — the payload copy behind the per-stream receive walk
 * (SURVEY §8 row f12): the consumer of mtcp_gpu_rcvwalk.h's placement records.
 *
 * RBPut's byte work (mtcp/src/tcp_ring_buffer.c:304-319) for every packet the
 * walk marked MTCP_GPU_RCV_COPY: the compaction of the buffer (:304-309), the
 * memcpy of the payload to head + putx (:315) and the tail_offset / last_len
 * update (:317-319).  The payload moves once, from an arbitrary byte offset in
 * a frame of the batch's chunk to an arbitrary byte offset in the stream's
 * receive buffer, for receive buffers that live in device-accessible memory.
 *
 * There is no host-memory form: the arena is device-resident state, and a
 * synchronous form would have to move the whole arena both ways for one
 * batch.  No call of this header waits, so none joins the wait-limit list.
 *
 * Plain C, as mtcp_gpu.h; MTCP_GPU_ABI_VERSION is unchanged (nothing that
 * exists changes): test for MTCP_GPU_HAS_RCVCOPY.
 */
#ifndef MTCP_GPU_RCVCOPY_H
#define MTCP_GPU_RCVCOPY_H

#include "mtcp_gpu.h"
#include "mtcp_gpu_group.h"
#include "mtcp_gpu_rcvwalk.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MTCP_GPU_HAS_RCVCOPY       1
/* A list with more copy candidates than this is planned by its whole wave, 64
 * packets a step; a shorter one by one lane. */
#define MTCP_GPU_RCVCOPY_WAVE_LEN  64

/*
 * The receive buffer of one stream, 32 B: the caller's array
 * d_rbuf[max_id + 1], 32 B aligned, indexed by stream id like d_state.  All
 * buffers of a context's streams sit in one caller-owned arena (device memory,
 * or registered host memory passed as a device-accessible address).  The
 * host's tcp_ring_buffer stays the truth: the caller fills the record after
 * RBInit and refreshes head_offset, tail_offset and last_len after RBRemove.
 *
 * A record is BAD if rsvd != 0, size == 0 or size > MTCP_GPU_RCV_MAX_SIZE,
 * data_off + size > arena_bytes, head_offset > tail_offset, tail_offset > size
 * or last_len != tail_offset - head_offset.  Nothing is copied for a BAD
 * stream and its record keeps every byte.
 */
typedef struct mtcp_gpu_rcv_buf {
    uint64_t data_off;        /*  0 rcvbuf->data, as a byte offset into the arena */
    uint32_t size;            /*  8 rcvbuf->size                                  */
    uint32_t head_offset;     /* 12 rcvbuf->head_offset                           */
    uint32_t tail_offset;     /* 16 rcvbuf->tail_offset                           */
    uint32_t last_len;        /* 20 rcvbuf->last_len                              */
    uint32_t rsvd[2];         /* 24 must be 0                                     */
} mtcp_gpu_rcv_buf;

/* d_cstat[n], one byte per packet, every one written. */
enum mtcp_gpu_rcv_cstat {
    MTCP_GPU_RCVCOPY_NONE      = 0,  /* no MTCP_GPU_RCV_COPY, or at or past its segment's seg_stop */
    MTCP_GPU_RCVCOPY_FRONT     = 1,  /* copied; put_off at or above every earlier end             */
    MTCP_GPU_RCVCOPY_ORDERED   = 2,  /* copied in list order behind the FRONT packets             */
    MTCP_GPU_RCVCOPY_BAD_BUF   = 3,  /* the stream's record is BAD                                */
    MTCP_GPU_RCVCOPY_BAD_SRC   = 4,  /* payload_len != put_len, the payload outside the
                                        descriptor's len, or the descriptor outside buf_len      */
    MTCP_GPU_RCVCOPY_BAD_RANGE = 5   /* put_off + put_len > size                                  */
};

/*
 * The contract.
 *
 * Copyable.  A packet with MTCP_GPU_RCV_COPY at a list position before its
 * segment's seg_stop is copyable if, tested in this order, its stream's record
 * is not BAD (else BAD_BUF), put_off + put_len <= size (else BAD_RANGE),
 * res.payload_len == put_len, the payload [14 + 4 * (ihl + doff), + put_len)
 * of the frame lies inside the descriptor's len and the descriptor inside
 * buf_len (else BAD_SRC).  A packet that is not copyable is skipped and takes
 * no part in anything below; the host copies it itself.
 *
 * Reference.  For a stream's list the reference runs tcp_ring_buffer.c:304-319
 * once per copyable packet in list order: the memmove of last_len bytes to the
 * chunk's start when size <= head_offset + put_off + put_len, the memcpy to
 * head + put_off, the tail_offset / last_len update.  After the call
 *
 *  1. head_offset, tail_offset and last_len of every stream equal the
 *     reference's;
 *  2. every live byte equals the reference's byte at head + x; here it is at
 *     data_off + head_offset' + x.  A byte is live if it is inside a payload
 *     copied in this batch or inside the stream's window before the batch
 *     (x < last_len before the batch);
 *  3. for a stream that did not compact in this batch the whole chunk
 *     [data_off, data_off + size) is byte-equal to the reference's data[];
 *  4. for a stream that did compact, bytes that are not live (holes, stale
 *     bytes past the window) are unspecified but stay inside the chunk.
 *
 * How the order is kept.  The reference's "last writer in list order wins" on
 * overlapping payloads (retransmissions) holds exactly.  Walking a stream's
 * copyable packets in list order, M is the largest put_off + put_len seen so
 * far (0 at the start).  A packet with put_off >= M is FRONT, any other is
 * ORDERED.  FRONT packets are pairwise disjoint: the later of two starts at or
 * above the earlier one's end.  No earlier packet covers a byte of a FRONT
 * packet, since every earlier end is at most M.  So all FRONT packets of all
 * streams are copied in parallel, in any order.  An ORDERED packet may overlap
 * earlier packets of either class, and only a later ORDERED packet can overlap
 * it (a later FRONT one starts at or above its end): the ORDERED packets are
 * copied afterwards one after another in list order within their stream,
 * streams in parallel, and every byte ends with its last writer's value.
 *
 * Compaction.  :304 fires when size <= head_offset + put_off + put_len.  After
 * it head_offset is 0, and a later trigger (put_off + put_len == size) moves
 * last_len bytes onto themselves: a stream compacts at most once per batch,
 * and at head_offset 0 not at all.  last_len' = max(last_len, M) with or
 * without it, because :306 takes head_offset from both ends.  The move is
 * therefore done first: the last_len bytes of before the batch go from
 * data_off + head_offset to data_off before any packet of the batch is
 * written, and every packet is written at the final head_offset'.  What the
 * reference's move carries beyond those bytes are payloads of this batch,
 * which are written at their final place anyway, and holes (4).
 *
 * Bounds.  Every store lands inside [data_off, data_off + size) of a non-BAD
 * record, hence inside the arena, whatever bytes d_rbuf, d_place, d_res and
 * d_desc hold.  Every load of frame bytes stays inside the aligned 16 B pieces
 * that hold bytes of the payload, which is rx's own rule.  An index in d_idx
 * at or above n is skipped, a segment whose id is above max_id is not
 * processed.  The outputs are a pure function of the inputs for group arrays
 * as mtcp_gpu_group[_dev] writes them and buffer regions that do not overlap;
 * otherwise the stores only stay bounded.
 */

/* Bytes of workspace mtcp_gpu_rcvcopy_dev needs (the copies of
 * tcp_ring_buffer.c:304-319 over n records).  Host only, needs no GPU.  0 if n
 * is above MTCP_GPU_GROUP_MAX_PKTS or max_id above MTCP_GPU_FLOWTAB_MAX_ID,
 * never 0 otherwise; non-decreasing in n and max_id. */
uint64_t mtcp_gpu_rcvcopy_work_bytes(uint32_t n, uint32_t max_id);

/*
 * Copy the payloads of a walked batch into the streams' receive buffers:
 * tcp_ring_buffer.c:304-319 for every copyable packet.  d_buf, buf_len, d_desc,
 * off_shift: the batch's chunk as mtcp_gpu_rx_chunk_dev saw it, with its
 * alignment rules; d_res[n]: the 40 B records; d_place[n] and d_seg_stop: what
 * mtcp_gpu_rcvwalk_dev wrote; d_idx, d_seg_sid, d_seg_start, d_nseg: what
 * mtcp_gpu_group_dev wrote, with the same n and max_id.  d_rbuf[max_id + 1]
 * is read, and updated for the streams that had a copyable packet; the arena
 * bytes and d_cstat[n] are written.
 *
 * Asynchronous on `stream` (NULL = the context's stream); allocates nothing,
 * waits for nothing and copies nothing to the host, so it can sit in a stream
 * capture behind the walk.  MTCP_GPU_EINVAL: NULL arguments, off_shift above
 * 16, buf_len not a multiple of 16, d_buf, d_arena or d_work not 16 B aligned,
 * d_rbuf not 32 B aligned, d_place not 16 B aligned, d_res or d_desc not 8 B
 * aligned, the u32 arrays not 4 B aligned, work_bytes below
 * mtcp_gpu_rcvcopy_work_bytes(n, max_id), n above MTCP_GPU_GROUP_MAX_PKTS,
 * max_id above MTCP_GPU_FLOWTAB_MAX_ID, a context opened with
 * MTCP_GPU_F_COMPACT (16 B records carry no ihl_doff).  MTCP_GPU_EIO on an
 * abandoned context.  n == 0 is MTCP_GPU_OK without a launch.
 */
int mtcp_gpu_rcvcopy_dev(mtcp_gpu_ctx *ctx, const void *d_buf, uint64_t buf_len, const mtcp_gpu_desc *d_desc,
                         uint32_t off_shift, const mtcp_gpu_result *d_res, const mtcp_gpu_rcv_place *d_place,
                         uint32_t n, uint32_t max_id, const uint32_t *d_idx, const uint32_t *d_seg_sid,
                         const uint32_t *d_seg_start, const uint32_t *d_nseg, const uint32_t *d_seg_stop,
                         mtcp_gpu_rcv_buf *d_rbuf, void *d_arena, uint64_t arena_bytes, uint8_t *d_cstat,
                         void *d_work, uint64_t work_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MTCP_GPU_RCVCOPY_H */
