"""numpy views of the C ABI records (include/mtcp_gpu.h)."""
import numpy as np

# struct mtcp_gpu_desc: layout-compatible with PSIO's ps_pkt_info (ps.h:181-185)
DESC_DTYPE = np.dtype([("offset", "<u4"), ("len", "<u2"), ("flags", "u1"), ("rsvd", "u1")])

# struct mtcp_gpu_result (40 B)
RESULT_DTYPE = np.dtype([
    ("saddr", "<u4"), ("daddr", "<u4"), ("sport", "<u2"), ("dport", "<u2"),
    ("seq", "<u4"), ("ack_seq", "<u4"), ("window", "<u2"), ("ip_len", "<u2"),
    ("ip_csum", "<u2"), ("tcp_csum", "<u2"), ("rss_hash", "<u4"),
    ("payload_len", "<u2"), ("ihl_doff", "u1"), ("tcp_flags", "u1"),
    ("verdict", "u1"), ("rss_queue", "u1"), ("eth_type", "<u2"),
])
assert DESC_DTYPE.itemsize == 8 and RESULT_DTYPE.itemsize == 40

# struct mtcp_gpu_result16 (16 B, MTCP_GPU_F_COMPACT): the same fields as the
# 40 B record's, for callers that act on the verdict
RESULT16_DTYPE = np.dtype([
    ("rss_hash", "<u4"), ("ip_csum", "<u2"), ("tcp_csum", "<u2"), ("payload_len", "<u2"),
    ("ip_len", "<u2"), ("ihl_doff", "u1"), ("tcp_flags", "u1"), ("verdict", "u1"),
    ("rss_queue", "u1"),
])
assert RESULT16_DTYPE.itemsize == 16


def compact_of(res: np.ndarray) -> np.ndarray:
    """The 16 B records a compact context writes, from 40 B records."""
    out = np.zeros(len(res), dtype=RESULT16_DTYPE)
    for f in RESULT16_DTYPE.names:
        out[f] = res[f]
    return out

VERDICTS = ("TCP_OK", "ETH_OTHER", "ARP", "IP_SHORT", "IP_CSUM_BAD", "IP_VERSION", "ICMP",
            "IP_PROTO_OTHER", "TCP_LEN_BAD", "TCP_CSUM_BAD", "TRUNCATED", "BAD_DESC")
RX_ERROR_VERDICTS = (3, 4, 8, 9)   # ProcessPacket ret < 0 (eth_in.c:49-53)

# struct mtcp_gpu_addr_entry: sockaddr_in address and port, network order
ADDR_ENTRY_DTYPE = np.dtype([("saddr", "<u4"), ("sport", "<u2"), ("rsvd", "<u2")])
assert ADDR_ENTRY_DTYPE.itemsize == 8

# struct mtcp_gpu_tcpopt (include/mtcp_gpu_tcpopt.h): ParseTCPTimestamp's and
# ParseTCPOptions' outputs per packet (mtcp/src/tcp_util.c:14-92)
TCPOPT_DTYPE = np.dtype([("ts_val", "<u4"), ("ts_ref", "<u4"), ("ts_recent", "<u4"), ("mss", "<u2"),
                         ("wscale", "u1"), ("flags", "u1")])
assert TCPOPT_DTYPE.itemsize == 16
# its flags
TCPOPT_TS_FOUND, TCPOPT_MSS, TCPOPT_WSCALE, TCPOPT_SACK_PERMIT = 0x01, 0x02, 0x04, 0x08
TCPOPT_SAW_TIMESTAMP, TCPOPT_TS_UNPINNED, TCPOPT_SYN_UNPINNED = 0x20, 0x40, 0x80

# include/mtcp_gpu_steer.h
STEER_MAX_QUEUES = 128
STEER_MAX_PKTS = 1 << 26
STEER_DROP_BAD = 0x1

# include/mtcp_gpu_txbuild.h: struct mtcp_gpu_tx_seg (one segment: the arguments
# of SendTCPPacketStandalone, tcp_out.c:135-140, or what SendTCPPacket reads
# from its stream) and struct mtcp_gpu_tx_link (eth_out.c:72-77)
TX_SEG_DTYPE = np.dtype([
    ("payload_off", "<u8"), ("saddr", "<u4"), ("daddr", "<u4"), ("sport", "<u2"), ("dport", "<u2"),
    ("seq", "<u4"), ("ack", "<u4"), ("ts_val", "<u4"), ("ts_ecr", "<u4"), ("window", "<u2"),
    ("ip_id", "<u2"), ("payload_len", "<u2"), ("mss", "<u2"), ("flags", "u1"), ("form", "u1"),
    ("wscale", "u1"), ("link", "u1"),
])
TX_LINK_DTYPE = np.dtype([("dst", "u1", (6,)), ("src", "u1", (6,))])
assert TX_SEG_DTYPE.itemsize == 48 and TX_LINK_DTYPE.itemsize == 12
assert [TX_SEG_DTYPE.fields[f][1] for f in TX_SEG_DTYPE.names] == [0, 8, 12, 16, 18, 20, 24, 28, 32, 36, 38, 40,
                                                                   42, 44, 45, 46, 47]
TXB_NO_CSUM = 0x1
TXB_BUILT, TXB_BAD_SEG, TXB_BAD_DESC, TXB_BAD_PAYLOAD = 0, 1, 2, 3
TXB_FLAG_FIN, TXB_FLAG_SYN, TXB_FLAG_RST, TXB_FLAG_PSH, TXB_FLAG_ACK = 0x01, 0x02, 0x04, 0x08, 0x10


def tx_seg_frame_len(flags, payload_len):
    """MTCP_GPU_TX_SEG_FRAME_LEN: 54 + optlen + payload_len (scalars or arrays)."""
    return 54 + np.where(np.asarray(flags) & TXB_FLAG_SYN, 20, 12) + np.asarray(payload_len, dtype=np.int64)


# include/mtcp_gpu_txseg.h: struct mtcp_gpu_tx_burst (one stream of the send
# list: what FlushTCPSendingBuffer reads of it, tcp_out.c:357-449) and struct
# mtcp_gpu_tx_burst_result
TX_BURST_DTYPE = np.dtype([
    ("payload_off", "<u8"), ("saddr", "<u4"), ("daddr", "<u4"), ("sport", "<u2"), ("dport", "<u2"),
    ("seq", "<u4"), ("ack", "<u4"), ("ts_val", "<u4"), ("ts_ecr", "<u4"), ("len", "<u4"),
    ("in_flight", "<u4"), ("window", "<u4"), ("peer_wnd", "<u4"), ("tcp_window", "<u2"), ("ip_id", "<u2"),
    ("mss", "<u2"), ("link", "u1"), ("rsvd0", "u1"), ("rsvd1", "<u4"),
])
TX_BURST_RESULT_DTYPE = np.dtype([("first_seg", "<u4"), ("n_seg", "<u4"), ("bytes", "<u4"), ("status", "u1"),
                                  ("stop", "u1"), ("rsvd", "<u2")])
assert TX_BURST_DTYPE.itemsize == 64 and TX_BURST_RESULT_DTYPE.itemsize == 16
assert [TX_BURST_DTYPE.fields[f][1] for f in TX_BURST_DTYPE.names] == [0, 8, 12, 16, 18, 20, 24, 28, 32, 36, 40, 44,
                                                                       48, 52, 54, 56, 58, 59, 60]
TXS_OK, TXS_BAD_BURST, TXS_BAD_PAYLOAD = 0, 1, 2
TXS_STOP_WINDOW, TXS_STOP_PEER_WINDOW, TXS_STOP_NO_ROOM = 0x1, 0x2, 0x4
TXSEG_MAX_BURSTS, TXSEG_MAX_SEGS, TXSEG_VOID_FORM = 1 << 24, 1 << 26, 0xFF

NUM_BINS_FLOWS = 131072     # mtcp/src/include/fhash.h:7
FLOW_NONE = 0xFFFFFFFF

# include/mtcp_gpu_flowtab.h: struct mtcp_gpu_flow_entry (the 12 key bytes
# HashFlow reads, tcp_stream.c:56-90, in the stream's orientation, and the
# caller's stream number) and struct mtcp_gpu_flowtab_counters
FLOW_ENTRY_DTYPE = np.dtype([("saddr", "<u4"), ("daddr", "<u4"), ("sport", "<u2"), ("dport", "<u2"), ("id", "<u4")])
FLOWTAB_COUNTERS_DTYPE = np.dtype([("live", "<u4"), ("tombs", "<u4"), ("insert_failed", "<u4"),
                                   ("remove_missed", "<u4")])
assert FLOW_ENTRY_DTYPE.itemsize == 16 and FLOWTAB_COUNTERS_DTYPE.itemsize == 16
FLOW_MISS = 0xFFFFFFFE
FLOWTAB_MAX_ID = 0xFFFFFFEF
FLOWTAB_MIN_CAP_LOG2, FLOWTAB_MAX_CAP_LOG2, FLOWTAB_MAX_BATCH = 4, 26, 1 << 26
MIN_PORT, MAX_PORT = 1025, 65536   # mtcp/src/include/addr_pool.h:7-8

# include/mtcp_gpu_rcvwalk.h: struct mtcp_gpu_rcv_state (one stream's receive
# state: what ValidateSequence, ProcessTCPPayload and RBPut read and write of it,
# tcp_in.c:101-179, :537-610, tcp_ring_buffer.c:280-382) and struct
# mtcp_gpu_rcv_place (one packet's placement record)
RCV_STATE_DTYPE = np.dtype([
    ("rcv_nxt", "<u4"), ("rcv_wnd", "<u4"), ("head_seq", "<u4"), ("merged_len", "<u4"), ("size", "<u4"),
    ("ts_recent", "<u4"), ("ts_lastack_rcvd", "<u4"), ("tcp_state", "u1"), ("saw_timestamp", "u1"), ("nfrag", "u1"),
    ("rsvd", "u1"), ("frag", [("seq", "<u4"), ("len", "<u4")], (4,)),
])
RCV_PLACE_DTYPE = np.dtype([("put_off", "<u4"), ("rcv_nxt", "<u4"), ("rcv_wnd", "<u4"), ("put_len", "<u2"),
                            ("verdict", "u1"), ("flags", "u1")])
assert RCV_STATE_DTYPE.itemsize == 64 and RCV_PLACE_DTYPE.itemsize == 16
assert [RCV_STATE_DTYPE.fields[f][1] for f in RCV_STATE_DTYPE.names] == [0, 4, 8, 12, 16, 20, 24, 28, 29, 30, 31, 32]
RCV_COPY, RCV_ACK_NOW, RCV_ACK_AGGREGATE, RCV_READ_EVENT, RCV_TS_NEWER = 0x01, 0x02, 0x04, 0x08, 0x10
RCV_VERDICTS = ("NONE", "DEFER_STATE", "DEFER_BAD_STATE", "DEFER_FLAGS", "DEFER_TS", "DEFER_FRAG_FULL", "DEFER_BEHIND",
                "PAWS_NO_TS", "PAWS_OLD", "SEQ_WINPROBE", "SEQ_OLD", "SEQ_AHEAD", "ACK_ONLY", "PUT_DROPPED",
                "PUT_NO_ROOM", "PUT_STORED")
RCV_MAX_FRAGS, RCV_MAX_SIZE, RCV_ST_ESTABLISHED = 4, 1 << 30, 4

# include/mtcp_gpu_ackwalk.h: struct mtcp_gpu_ack_state (one stream's send
# state, 128 B: d_snd[max_id + 1] indexed by stream id; bytes 88-127 are the
# caller's) and struct mtcp_gpu_ack_rec (one packet's ACK record)
ACK_STATE_DTYPE = np.dtype([
    ("snd_nxt", "<u4"), ("snd_una", "<u4"), ("snd_wnd", "<u4"), ("peer_wnd", "<u4"), ("snd_wl1", "<u4"),
    ("snd_wl2", "<u4"), ("last_ack_seq", "<u4"), ("cwnd", "<u4"), ("ssthresh", "<u4"), ("rto", "<u4"),
    ("ts_rto", "<u4"), ("srtt", "<u4"), ("mdev", "<u4"), ("mdev_max", "<u4"), ("rttvar", "<u4"), ("rtt_seq", "<u4"),
    ("sb_head_seq", "<u4"), ("sb_len", "<u4"), ("sb_size", "<u4"), ("mss", "<u2"), ("eff_mss", "<u2"),
    ("tcp_state", "u1"), ("saw_timestamp", "u1"), ("wscale_peer", "u1"), ("dup_acks", "u1"), ("nrtx", "u1"),
    ("on_rto", "u1"), ("has_sndbuf", "u1"), ("rsvd", "u1"), ("user", "u1", (40,))])
ACK_REC_DTYPE = np.dtype([("rmlen", "<u4"), ("snd_nxt", "<u4"), ("cwnd", "<u4"), ("flags", "<u2"), ("verdict", "u1"),
                          ("dup_acks", "u1")])
assert ACK_STATE_DTYPE.itemsize == 128 and ACK_REC_DTYPE.itemsize == 16
assert [ACK_STATE_DTYPE.fields[f][1] for f in ACK_STATE_DTYPE.names] == \
    list(range(0, 76, 4)) + [76, 78, 80, 81, 82, 83, 84, 85, 86, 87, 88]
(ACK_WND_UPDATE, ACK_WRITE_EVENT_WND, ACK_DUP, ACK_FAST_RTX, ACK_SND_NXT_RECOVERED, ACK_SEND_LIST_REMOVE,
 ACK_WRITE_EVENT_ROOM, ACK_RTO_REMOVE, ACK_RTO_ADD) = (1 << k for k in range(9))
ACK_FLAGS = ("WND_UPDATE", "WRITE_EVENT_WND", "DUP", "FAST_RTX", "SND_NXT_RECOVERED", "SEND_LIST_REMOVE",
             "WRITE_EVENT_ROOM", "RTO_REMOVE", "RTO_ADD")
ACK_VERDICTS = ("NONE", "DEFER_RCV", "DEFER_STATE", "DEFER_BAD_STATE", "DEFER_FLAGS", "DEFER_ARITH", "DEFER_BEHIND",
                "NOT_VALID", "NO_ACK_FLAG", "NO_SNDBUF", "ACK_BEYOND", "ACK_OLD", "ACK_NEW")
ACK_MAX_SIZE, ACK_ST_ESTABLISHED, ACK_MAX_RTX = 1 << 30, 4, 16

# include/mtcp_gpu_ackgen.h: struct mtcp_gpu_ackgen_state (what WriteTCPACKList
# and SendTCPPacket read of one stream beyond the walks' states, 32 B:
# d_tx[max_id + 1] indexed by stream id) and struct mtcp_gpu_ackgen_res (one
# segment's result)
ACKGEN_STATE_DTYPE = np.dtype([("saddr", "<u4"), ("daddr", "<u4"), ("sport", "<u2"), ("dport", "<u2"),
                               ("ip_id", "<u2"), ("ack_cnt", "u1"), ("is_wack", "u1"), ("wscale_mine", "u1"),
                               ("link", "u1"), ("has_rcvbuf", "u1"), ("need_wnd_adv", "u1"),
                               ("ts_lastack_sent", "<u4"), ("rsvd", "u1", (8,))])
ACKGEN_RES_DTYPE = np.dtype([("first_seg", "<u4"), ("n_ack", "u1"), ("wack", "u1"), ("status", "u1"), ("flags", "u1"),
                             ("ack", "<u4"), ("window", "<u2"), ("rsvd", "<u2")])
assert ACKGEN_STATE_DTYPE.itemsize == 32 and ACKGEN_RES_DTYPE.itemsize == 16
assert [ACKGEN_STATE_DTYPE.fields[f][1] for f in ACKGEN_STATE_DTYPE.names] == \
    [0, 4, 8, 10, 12, 14, 15, 16, 17, 18, 19, 20, 24]
ACKGEN_STATUS = ("NONE", "BAD", "DEFERRED", "IDLE", "NOT_TO_ACK", "SENT", "NO_ROOM")
ACKGEN_ON_LIST, ACKGEN_NEED_WND_ADV, ACKGEN_FRAME_LEN = 0x1, 0x2, 66

# include/mtcp_gpu_datagen.h: struct mtcp_gpu_datagen_state (where one stream's
# send buffer lies in the payload arena and its list membership, 16 B:
# d_dtx[max_id + 1] indexed by stream id) and struct mtcp_gpu_datagen_res (one
# segment's result)
DATAGEN_STATE_DTYPE = np.dtype([("sb_off", "<u8"), ("sb_base_seq", "<u4"), ("on_send_list", "u1"),
                                ("on_control_list", "u1"), ("rsvd", "u1", (2,))])
DATAGEN_RES_DTYPE = np.dtype([("first_seg", "<u4"), ("n_seg", "<u4"), ("bytes", "<u4"), ("status", "u1"),
                              ("stop", "u1"), ("flags", "u1"), ("rsvd", "u1")])
assert DATAGEN_STATE_DTYPE.itemsize == 16 and DATAGEN_RES_DTYPE.itemsize == 16
DATAGEN_STATUS = ("NONE", "BAD", "DEFERRED", "IDLE", "CONTROL_WAIT", "NO_SNDBUF", "EMPTY", "BEHIND_HEAD", "BAD_BURST",
                  "SENT", "WINDOW", "NO_ROOM")
(DATAGEN_ON_LIST_BEFORE, DATAGEN_ON_LIST_AFTER, DATAGEN_RTO_ADD, DATAGEN_WACK_ENQUEUED,
 DATAGEN_NEED_WND_ADV) = (1 << k for k in range(5))
DATAGEN_MAX_DIST = 1 << 30

# include/mtcp_gpu_rtosweep.h: struct mtcp_gpu_rto_rec (one handled stream of a
# retransmission-timeout sweep, 16 B: d_rto[j] for j < handled, in ascending id)
RTO_REC_DTYPE = np.dtype([("sid", "<u4"), ("rto", "<u4"), ("nrtx", "u1"), ("verdict", "u1"), ("flags", "u1"),
                          ("rsvd0", "u1"), ("rsvd1", "<u4")])
assert RTO_REC_DTYPE.itemsize == 16
RTO_VERDICTS = ("NONE", "BAD", "DEFER_STATE", "LOST", "RETRANSMIT")
RTO_SEND_LIST_ADD, RTO_MAX_BACKOFF, RTO_ST_CLOSED = 0x01, 7, 0

# include/mtcp_gpu_rcvcopy.h: struct mtcp_gpu_rcv_buf (one stream's receive
# buffer in the arena: what RBPut's byte work reads and writes of it,
# tcp_ring_buffer.c:304-319) and the status bytes of d_cstat
RCV_BUF_DTYPE = np.dtype([("data_off", "<u8"), ("size", "<u4"), ("head_offset", "<u4"), ("tail_offset", "<u4"),
                          ("last_len", "<u4"), ("rsvd", "<u4", (2,))])
assert RCV_BUF_DTYPE.itemsize == 32
assert [RCV_BUF_DTYPE.fields[f][1] for f in RCV_BUF_DTYPE.names] == [0, 8, 12, 16, 20, 24]
RCVCOPY_STATS = ("NONE", "FRONT", "ORDERED", "BAD_BUF", "BAD_SRC", "BAD_RANGE")
RCVCOPY_WAVE_LEN = 64

# include/mtcp_gpu_rcvread.h: struct mtcp_gpu_rcvread_req (one application read:
# CopyToUser's stream, len and user buffer, api.c:1114-1149) and struct
# mtcp_gpu_rcvread_res (what the read returned and what the host replays)
RCVREAD_REQ_DTYPE = np.dtype([("sid", "<u4"), ("len", "<u4"), ("dst_off", "<u8"), ("flags", "<u4"),
                              ("rsvd", "<u4", (3,))])
RCVREAD_RES_DTYPE = np.dtype([("sid", "<u4"), ("copylen", "<u4"), ("rcv_wnd", "<u4"), ("verdict", "u1"),
                              ("flags", "u1"), ("rsvd", "<u2")])
assert RCVREAD_REQ_DTYPE.itemsize == 32 and RCVREAD_RES_DTYPE.itemsize == 16
assert [RCVREAD_REQ_DTYPE.fields[f][1] for f in RCVREAD_REQ_DTYPE.names] == [0, 4, 8, 16, 20]
assert [RCVREAD_RES_DTYPE.fields[f][1] for f in RCVREAD_RES_DTYPE.names] == [0, 4, 8, 12, 13, 14]
RCVREAD_VERDICTS = ("NONE", "BAD_REQ", "DUP", "BAD_STATE", "DEFER_STATE", "EAGAIN", "PEEKED", "READ")
RCVREAD_PEEK, RCVREAD_ON_ACKQ = 0x1, 0x2
RCVREAD_MORE, RCVREAD_WND_ADV, RCVREAD_FRAG_FREED = 0x1, 0x2, 0x4
RCVREAD_HOST_MAX_BYTES = 32 << 20

# include/mtcp_gpu_sndwrite.h: struct mtcp_gpu_sndwrite_req (one application
# write: CopyFromUser's stream, len and user buffer, api.c:1416-1456) and struct
# mtcp_gpu_sndwrite_res (what the write returned and what the host replays)
SNDWRITE_REQ_DTYPE = np.dtype([("sid", "<u4"), ("len", "<u4"), ("src_off", "<u8"), ("flags", "<u4"),
                               ("rsvd", "<u4", (3,))])
SNDWRITE_RES_DTYPE = np.dtype([("sid", "<u4"), ("written", "<u4"), ("snd_wnd", "<u4"), ("verdict", "u1"),
                               ("flags", "u1"), ("rsvd", "<u2")])
assert SNDWRITE_REQ_DTYPE.itemsize == 32 and SNDWRITE_RES_DTYPE.itemsize == 16
assert [SNDWRITE_REQ_DTYPE.fields[f][1] for f in SNDWRITE_REQ_DTYPE.names] == [0, 4, 8, 16, 20]
assert [SNDWRITE_RES_DTYPE.fields[f][1] for f in SNDWRITE_RES_DTYPE.names] == [0, 4, 8, 12, 13, 14]
SNDWRITE_VERDICTS = ("NONE", "BAD_REQ", "DUP", "BAD_STATE", "DEFER_STATE", "ZERO", "EAGAIN", "NO_SNDBUF", "FULL",
                     "WRITTEN")
SNDWRITE_ROOM, SNDWRITE_SEND_LIST_ADD, SNDWRITE_COMPACTED = 0x1, 0x2, 0x4
SNDWRITE_HOST_MAX_BYTES = 32 << 20
