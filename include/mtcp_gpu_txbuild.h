/*
 * mtcp_gpu_txbuild.h — building tx frames on the device from segment records
 * (SURVEY §8 row f7).
 *
 * In the reference FlushTCPSendingBuffer (mtcp/src/tcp_out.c:357-449) cuts a
 * send buffer into segments and SendTCPPacket / SendTCPPacketStandalone
 * (tcp_out.c:135-354) runs, per segment, IPOutput* (mtcp/src/ip_out.c:35-167)
 * and EthernetOutput (mtcp/src/eth_out.c:35-80), writes 54 B of headers and
 * 12 or 20 B of options, memcpys the payload (tcp_out.c:195, :314) and sums
 * every byte it just copied (tcp_out.c:208, :327).  mtcp_gpu_tx_fill* of
 * mtcp_gpu.h takes over only that sum, over frames a CPU has assembled.  The
 * entry points here take the whole chain: one record per segment in, the
 * finished frame out, each payload byte read once and each frame byte written
 * once.  The caller still runs FlushTCPSendingBuffer's window logic
 * (tcp_out.c:384-444) and the route / ARP lookups; it emits one record per
 * segment and one link-table index per record.
 *
 * Plain C, as mtcp_gpu.h; MTCP_GPU_ABI_VERSION is unchanged (nothing that
 * exists changes): test for MTCP_GPU_HAS_TXBUILD.
 */
#ifndef MTCP_GPU_TXBUILD_H
#define MTCP_GPU_TXBUILD_H

#include "mtcp_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MTCP_GPU_HAS_TXBUILD        1
#define MTCP_GPU_TXB_NO_CSUM        0x1u    /* call flag: both check fields stay 0, as when
                                               dev_ioctl answers 0 (ip_out.c:145-161, tcp_out.c:320-330) */
#define MTCP_GPU_TXB_MAX_LINKS      256u
#define MTCP_GPU_TXB_DEFAULT_MSS    1460u   /* TCP_DEFAULT_MSS */

/* per-segment status; the first that applies, in this order */
#define MTCP_GPU_TXB_BUILT          0
#define MTCP_GPU_TXB_BAD_SEG        1       /* unknown flag bits, form > 1, link >= n_links,
                                               payload_len > max_mss + optlen (the reference's ERROR,
                                               tcp_out.c:149, :231), a frame above 65 535 B */
#define MTCP_GPU_TXB_BAD_DESC       2       /* len is not the frame's length, an odd byte offset,
                                               a slot that reaches past buf_len */
#define MTCP_GPU_TXB_BAD_PAYLOAD    3       /* payload_off + payload_len > payload_bytes */

/* TCP_FLAG_* of the reference (mtcp/src/include/tcp_in.h) */
#define MTCP_GPU_TXB_FLAG_FIN       0x01u
#define MTCP_GPU_TXB_FLAG_SYN       0x02u
#define MTCP_GPU_TXB_FLAG_RST       0x04u
#define MTCP_GPU_TXB_FLAG_PSH       0x08u
#define MTCP_GPU_TXB_FLAG_ACK       0x10u

/* One segment: the arguments of SendTCPPacketStandalone (tcp_out.c:135-140),
 * or what SendTCPPacket reads from its stream (tcp_out.c:224-300). */
typedef struct mtcp_gpu_tx_seg {   /* 48 B, 8 B aligned */
    uint64_t payload_off;  /*  0 byte offset into the payload buffer; ANY alignment, odd included */
    uint32_t saddr, daddr; /*  8, 12  as stream->saddr/daddr (network order, as in memory) */
    uint16_t sport, dport; /* 16, 18  network order */
    uint32_t seq, ack;     /* 20, 24  host order; ack reaches the wire only with TCP_FLAG_ACK */
    uint32_t ts_val, ts_ecr; /* 28, 32 host order: cur_ts, echo_ts / rcvvar->ts_recent */
    uint16_t window;       /* 36 host order, the value for the wire (caller did >> wscale, MIN) */
    uint16_t ip_id;        /* 38 host order (0 standalone; sndvar->ip_id++ for a stream) */
    uint16_t payload_len;  /* 40 */
    uint16_t mss;          /* 42 read only by a SYN of form 1 */
    uint8_t  flags;        /* 44 TCP_FLAG_FIN|SYN|RST|PSH|ACK (0x1F); any other bit: BAD_SEG */
    uint8_t  form;         /* 45 0 = SendTCPPacketStandalone, 1 = SendTCPPacket; other: BAD_SEG */
    uint8_t  wscale;       /* 46 read only by a SYN of form 1 */
    uint8_t  link;         /* 47 index into the link table */
} mtcp_gpu_tx_seg;

/* One next hop: the ARP answer and CONFIG.eths[].haddr (eth_out.c:72-77) */
typedef struct mtcp_gpu_tx_link { uint8_t dst[6], src[6]; } mtcp_gpu_tx_link;

/* Option bytes (CalculateOptionLength, tcp_out.c:21-60, with
 * TCP_OPT_TIMESTAMP_ENABLED TRUE and TCP_OPT_SACK_ENABLED FALSE) and the
 * frame's length: what the caller asks get_wptr for (eth_out.c:58). */
#define MTCP_GPU_TX_SEG_OPTLEN(flags)   (((flags) & MTCP_GPU_TXB_FLAG_SYN) ? 20u : 12u)
#define MTCP_GPU_TX_SEG_FRAME_LEN(flags, payload_len) \
    (54u + MTCP_GPU_TX_SEG_OPTLEN(flags) + (uint32_t)(payload_len))

/*
 * The frame of one segment, bit for bit (optlen as above):
 *   Ethernet   link.dst, link.src, 08 00                          (eth_out.c:72-77)
 *   IPv4       45 00, tot_len = 40 + optlen + payload_len, ip_id, 40 00, ttl 64,
 *              protocol 6, ip_fast_csum, saddr, daddr              (ip_out.c:66-76, :135-145)
 *   TCP        ports, htonl(seq), htonl(ack) with ACK else 0, doff = (20 + optlen) / 4,
 *              flags & 0x1F, htons(window), TCPCalcChecksum over 20 + optlen +
 *              payload_len bytes, urg 0                            (tcp_out.c:160-192, :208-210)
 *   options    form 0, or form 1 without SYN: 01 01 08 0a ts_val ts_ecr
 *              (tcp_out.c:185-190, :118-122); a form-0 SYN's option bytes 12-19
 *              are zero (the memset of tcp_out.c:160 covers them and nothing
 *              writes them); form 1 with SYN: 02 04 mss | 01 01 08 0a ts_val
 *              ts_ecr | 01 03 03 wscale                            (tcp_out.c:79-114)
 *   payload    at frame byte 54 + optlen                           (tcp_out.c:195, :314)
 */

/*
 * Build n frames on the device: SendTCPPacketStandalone / SendTCPPacket
 * (tcp_out.c:135-354) with IPOutput* (ip_out.c:35-167) and EthernetOutput
 * (eth_out.c:35-80).  d_desc[i] is what get_wptr is to the reference
 * (eth_out.c:58): the slot's offset (bytes = offset << off_shift, even) and
 * the length asked for, which must equal MTCP_GPU_TX_SEG_FRAME_LEN; the same
 * array then feeds mtcp_gpu_rx_chunk_dev or mtcp_gpu_tx_fill_dev unchanged.
 * d_status[i] gets the segment's status; a segment with a non-zero status has
 * no byte of its slot written.  Bytes outside [start, start + len) of a slot
 * are never written and d_buf is never read: slots may be packed back to back
 * at even offsets.  max_mss 0 means TCP_DEFAULT_MSS (1460).
 * Asynchronous on `stream` (NULL = the context's stream); allocates nothing
 * and waits for nothing, so it can sit in a stream capture.
 * MTCP_GPU_EINVAL: NULL arguments, misaligned arguments (d_seg or d_desc not
 * 8 B aligned, d_links not 4 B), n_links outside 1..256, off_shift above 16,
 * unknown call flags, a payload range that overlaps d_buf's range.
 * MTCP_GPU_EIO on an abandoned context.  n == 0 is MTCP_GPU_OK without a launch.
 */
int mtcp_gpu_tx_build_dev(mtcp_gpu_ctx *ctx, const mtcp_gpu_tx_seg *d_seg, uint32_t n,
                          const void *d_payload, uint64_t payload_bytes,
                          const mtcp_gpu_tx_link *d_links, uint32_t n_links,
                          void *d_buf, uint64_t buf_len, const mtcp_gpu_desc *d_desc, uint32_t off_shift,
                          uint16_t max_mss, uint32_t flags, uint8_t *d_status, void *stream);

/*
 * The same for host memory (tcp_out.c:135-354, ip_out.c:35-167,
 * eth_out.c:35-80).  Synchronous, built like mtcp_gpu_tx_fill: records,
 * payload, links and descriptors go up on the context's stream, the frames
 * come back into pinned staging, and the calling thread copies the bytes of
 * the built frames, and no others, into buf; *n_built (may be NULL) counts
 * them.  Bounded by the context's wait limit (mtcp_gpu_set_wait_limit): past
 * it neither buf nor status is written, MTCP_GPU_ETIMEDOUT is returned and the
 * context is ABANDONED.
 */
int mtcp_gpu_tx_build(mtcp_gpu_ctx *ctx, const mtcp_gpu_tx_seg *seg, uint32_t n,
                      const void *payload, uint64_t payload_bytes,
                      const mtcp_gpu_tx_link *links, uint32_t n_links,
                      void *buf, uint64_t buf_len, const mtcp_gpu_desc *desc, uint32_t off_shift,
                      uint16_t max_mss, uint32_t flags, uint8_t *status, uint32_t *n_built);

#ifdef __cplusplus
}
#endif

#endif /* MTCP_GPU_TXBUILD_H */
