/*
 * mtcp_gpu_tcpopt.h — per-packet TCP option records.
 *
 * After TCPCalcChecksum and the flow lookup the reference walks each
 * segment's option bytes in two places of its rx path:
 *
 *   ParseTCPTimestamp (mtcp/src/tcp_util.c:61-92)
 *       on every non-RST segment of a flow that negotiated timestamps
 *       (ValidateSequence, mtcp/src/tcp_in.c:106-139: the PAWS check, :109);
 *   ParseTCPOptions (mtcp/src/tcp_util.c:14-59)
 *       on every SYN (mtcp/src/tcp_in.c:72, :88).
 *
 * Both walk tcpopt = tcph + 20, len = 4*doff - 20.  The entry points here
 * run both walks for every TCP_OK frame of an rx batch and write one 16 B
 * record per packet, so that a caller gets ts_val / ts_ref / mss / wscale
 * without reading the headers again on the CPU.  ParseSACKOption is compiled
 * out in the reference (TCP_OPT_SACK_ENABLED FALSE, mtcp/src/include/mtcp.h:48)
 * and has no counterpart here.
 *
 * Plain C, as mtcp_gpu.h; MTCP_GPU_ABI_VERSION is unchanged (nothing that
 * exists changes): test for MTCP_GPU_HAS_TCPOPT.
 */
#ifndef MTCP_GPU_TCPOPT_H
#define MTCP_GPU_TCPOPT_H

#include "mtcp_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MTCP_GPU_HAS_TCPOPT 1

/* flags of mtcp_gpu_tcpopt */
#define MTCP_GPU_TCPOPT_TS_FOUND      0x01u  /* ParseTCPTimestamp returned TRUE  tcp_util.c:84 */
#define MTCP_GPU_TCPOPT_MSS           0x02u  /* TCP_OPT_FLAG_MSS          tcp_in.h:21, tcp_util.c:35 */
#define MTCP_GPU_TCPOPT_WSCALE        0x04u  /* TCP_OPT_FLAG_WSCALE       tcp_in.h:22, tcp_util.c:42 */
#define MTCP_GPU_TCPOPT_SACK_PERMIT   0x08u  /* TCP_OPT_FLAG_SACK_PERMIT  tcp_in.h:23, tcp_util.c:45 */
#define MTCP_GPU_TCPOPT_SACK          0x10u  /* TCP_OPT_FLAG_SACK         tcp_in.h:24: always 0 */
#define MTCP_GPU_TCPOPT_SAW_TIMESTAMP 0x20u  /* cur_stream->saw_timestamp tcp_util.c:49 */
#define MTCP_GPU_TCPOPT_TS_UNPINNED   0x40u  /* the ParseTCPTimestamp walk is unpinned (below) */
#define MTCP_GPU_TCPOPT_SYN_UNPINNED  0x80u  /* the ParseTCPOptions walk is unpinned (below) */

/*
 * Per-packet option record, 16 B.  As in mtcp_gpu_result, a field is written
 * only once the reference's chain has read it; everything else is 0:
 *   - the record is all zero unless the packet's verdict is MTCP_GPU_V_TCP_OK;
 *   - the ParseTCPTimestamp walk (ts_val, ts_ref, TS_FOUND) runs when RST is
 *     clear (tcp_in.c:108-109);
 *   - the ParseTCPOptions walk (ts_recent, mss, wscale, MSS, WSCALE,
 *     SACK_PERMIT, SAW_TIMESTAMP) runs when SYN is set (tcp_in.c:72, :88); the
 *     last occurrence of each option wins, as in the reference;
 *   - doff < 5 (len < 0) runs no walk.
 * eff_mss (tcp_util.c:38-41) is mss - 12 in 16 bits and is not stored.
 *
 * A walk is UNPINNED where the reference's result is not defined:
 *   - it would not terminate: a skipped option whose length byte is 0 does
 *     `i += optlen - 2` (tcp_util.c:55, :87) and lands on the same byte again
 *     (every kind but 0, 1, 8 in ParseTCPTimestamp; every kind but 0, 1, 2,
 *     3, 4, 8 in ParseTCPOptions);
 *   - or a byte it reads lies at or past the frame's end (the descriptor's
 *     len): the length byte may sit at index len, the two MSS bytes may end
 *     at len + 2, the timestamps at len + 8.  Bytes past 14 + ip_len but
 *     inside the frame are read as the reference reads them.
 * An unpinned walk writes only its UNPINNED bit: its fields and found bits
 * stay 0, and no byte at or past the frame's end is ever read.
 */
typedef struct mtcp_gpu_tcpopt {
    uint32_t ts_val;    /*  0 ParseTCPTimestamp ts->ts_val      tcp_util.c:82 */
    uint32_t ts_ref;    /*  4 ParseTCPTimestamp ts->ts_ref      tcp_util.c:83 */
    uint32_t ts_recent; /*  8 ParseTCPOptions rcvvar->ts_recent tcp_util.c:50 */
    uint16_t mss;       /* 12 ParseTCPOptions sndvar->mss       tcp_util.c:36-37 */
    uint8_t  wscale;    /* 14 ParseTCPOptions wscale_peer       tcp_util.c:43 */
    uint8_t  flags;     /* 15 MTCP_GPU_TCPOPT_* */
} mtcp_gpu_tcpopt;

/*
 * Device-resident option records of an rx batch: ParseTCPTimestamp
 * (tcp_util.c:61-92, called at tcp_in.c:109) and ParseTCPOptions
 * (tcp_util.c:14-59, called at tcp_in.c:72 and :88) for every frame.
 * Asynchronous on `stream` (NULL = the context's stream), with the frame
 * arguments and rules of mtcp_gpu_rx_chunk_dev.  d_res holds the records the
 * context's rx call wrote for these frames (40 B, or 16 B on an
 * MTCP_GPU_F_COMPACT context: verdict, ihl_doff and tcp_flags are read);
 * d_opt[n] is 16 B aligned.  A frame whose record is not TCP_OK is never
 * read; descriptors get the bounds check of rx (a frame rx would give
 * MTCP_GPU_V_BAD_DESC is not touched, whatever d_res says).
 * MTCP_GPU_EINVAL on NULL or misaligned arguments, MTCP_GPU_EIO on an
 * abandoned context; n == 0 is MTCP_GPU_OK without a launch.
 */
int mtcp_gpu_rx_tcpopt_chunk_dev(mtcp_gpu_ctx *ctx, const void *d_buf, uint64_t buf_len,
                                 const mtcp_gpu_desc *d_desc, uint32_t n, uint32_t off_shift,
                                 const mtcp_gpu_result *d_res, mtcp_gpu_tcpopt *d_opt,
                                 void *stream);

/* The same over a pointer burst (the rules of mtcp_gpu_rx_ptrs_dev: a NULL
 * or odd pointer is not read). */
int mtcp_gpu_rx_tcpopt_ptrs_dev(mtcp_gpu_ctx *ctx, const uint8_t *const *d_pkts,
                                const uint16_t *d_lens, uint32_t n,
                                const mtcp_gpu_result *d_res, mtcp_gpu_tcpopt *d_opt,
                                void *stream);

/*
 * mtcp_gpu_rx_chunk plus the option records (ParseTCPTimestamp
 * tcp_util.c:61-92, ParseTCPOptions tcp_util.c:14-59): host memory in, out[n]
 * and opts[n] written to host memory; synchronous, bounded by the context's
 * wait limit exactly as mtcp_gpu_rx_chunk (past the limit neither out nor
 * opts is written, MTCP_GPU_ETIMEDOUT, the context abandoned).  The option
 * kernel runs behind each stage's rx launch on that stage's stream: one more
 * device-to-host copy of 16 B per packet per batch.
 */
int mtcp_gpu_rx_chunk_opts(mtcp_gpu_ctx *ctx, const uint8_t *buf, uint64_t buf_len,
                           const mtcp_gpu_desc *desc, uint32_t n, uint32_t off_shift,
                           mtcp_gpu_result *out, mtcp_gpu_tcpopt *opts);

#ifdef __cplusplus
}
#endif

#endif /* MTCP_GPU_TCPOPT_H */
