"""A literal Python restatement of the reference's ProcessACK for one
ESTABLISHED stream, with the deferral rules of include/mtcp_gpu_ackwalk.h on top:

  Handle_TCP_ST_ESTABLISHED   its ACK branch, mtcp/src/tcp_in.c:864-869
  ProcessACK                  tcp_in.c:302-531
  EstimateRTT                 tcp_in.c:249-300
  SBRemove                    mtcp/src/tcp_send_buffer.c:149-173 (its bookkeeping)
  UpdateRetransmissionTimer   mtcp/src/timer.c:149-173

The reference's statements in the reference's order, with C's conversions
spelled out (a uint32_t store masks, `long m` is a Python int inside 64 bits,
uint8_t and uint16_t truncate).  Every expected value of
tests/test_ackwalk_model.py and tests/test_gpu_ackwalk.py comes from here, never
from the kernels.
"""
import numpy as np

from mtcp_amd._types import (ACK_DUP, ACK_FAST_RTX, ACK_MAX_RTX, ACK_MAX_SIZE, ACK_REC_DTYPE, ACK_RTO_ADD,
                             ACK_RTO_REMOVE, ACK_SEND_LIST_REMOVE, ACK_SND_NXT_RECOVERED, ACK_ST_ESTABLISHED,
                             ACK_VERDICTS, ACK_WND_UPDATE, ACK_WRITE_EVENT_ROOM, ACK_WRITE_EVENT_WND, FLOW_MISS,
                             FLOW_NONE, TCPOPT_TS_FOUND)

M32 = 0xFFFFFFFF
INT_MAX = 0x7FFFFFFF
(NONE, DEFER_RCV, DEFER_STATE, DEFER_BAD_STATE, DEFER_FLAGS, DEFER_ARITH, DEFER_BEHIND, NOT_VALID, NO_ACK_FLAG,
 NO_SNDBUF, ACK_BEYOND, ACK_OLD, ACK_NEW) = range(13)
assert ACK_VERDICTS[ACK_NEW] == "ACK_NEW" and ACK_VERDICTS[DEFER_BEHIND] == "DEFER_BEHIND"
WALKED = tuple(range(NOT_VALID, ACK_NEW + 1))
DEFERS = tuple(range(DEFER_RCV, DEFER_BEHIND + 1))
TCP_FIN, TCP_SYN, TCP_RST, TCP_ACK = 0x01, 0x02, 0x04, 0x10
RCV_FIRST_WALKED, RCV_FIRST_VALID, RCV_LAST = 7, 12, 15          # enum mtcp_gpu_rcv_verdict
WORDS = ("snd_nxt", "snd_una", "snd_wnd", "peer_wnd", "snd_wl1", "snd_wl2", "last_ack_seq", "cwnd", "ssthresh", "rto",
         "ts_rto", "srtt", "mdev", "mdev_max", "rttvar", "rtt_seq", "sb_head_seq", "sb_len")
CHANGED = WORDS + ("dup_acks", "nrtx", "on_rto")                 # what the walk may write
FIXED = ("sb_size", "mss", "eff_mss", "tcp_state", "saw_timestamp", "wscale_peer", "has_sndbuf", "rsvd")


def _s32(x):
    x &= M32
    return x - (1 << 32) if x & 0x80000000 else x


def TCP_SEQ_LT(a, b):                                # tcp_in.h:37-41
    return _s32(a - b) < 0


def TCP_SEQ_GT(a, b):
    return _s32(a - b) > 0


def TCP_SEQ_GEQ(a, b):
    return _s32(a - b) >= 0


class Snd:
    """What ProcessACK reads and writes of one tcp_stream, its tcp_send_vars,
    tcp_recv_vars and tcp_send_buffer: the fields of mtcp_gpu_ack_state."""
    __slots__ = CHANGED + FIXED

    def __init__(self, **kw):
        for f in self.__slots__:
            setattr(self, f, 0)
        self.tcp_state, self.has_sndbuf, self.mss, self.eff_mss, self.sb_size = ACK_ST_ESTABLISHED, 1, 1460, 1448, 8192
        for k, v in kw.items():
            setattr(self, k, v)

    @classmethod
    def from_record(cls, r):
        return cls(**{f: int(r[f]) for f in cls.__slots__})

    def to_record(self, a, i):
        """The bytes the walk changes, into element i of the ACK_STATE_DTYPE array a."""
        for f in CHANGED:
            a[f][i] = getattr(self, f)

    def copy(self):
        return Snd(**{f: getattr(self, f) for f in self.__slots__})

    def words(self):
        return tuple(getattr(self, f) for f in CHANGED)

    def bad(self):
        return (self.rsvd != 0 or self.eff_mss == 0 or self.wscale_peer > 31 or self.sb_size > ACK_MAX_SIZE or
                self.sb_len > self.sb_size)


class Arith(Exception):
    """The reference's int arithmetic would overflow or divide by zero."""


def EstimateRTT(st, mrtt):                           # tcp_in.c:249-300
    m = mrtt                                         # long m = mrtt
    if m == 0:
        m = 1
    if st.srtt != 0:
        m -= st.srtt >> 3
        st.srtt = (st.srtt + m) & M32
        if m < 0:
            m = -m
            m -= st.mdev >> 2
            if m > 0:
                m >>= 3
        else:
            m -= st.mdev >> 2
        st.mdev = (st.mdev + m) & M32
        if st.mdev > st.mdev_max:
            st.mdev_max = st.mdev
            if st.mdev_max > st.rttvar:
                st.rttvar = st.mdev_max
        if TCP_SEQ_GT(st.snd_una, st.rtt_seq):
            if st.mdev_max < st.rttvar:
                st.rttvar = (st.rttvar - ((st.rttvar - st.mdev_max) >> 2)) & M32
            st.rtt_seq = st.snd_nxt
            st.mdev_max = 0                          # tcp_rto_min
    else:
        st.srtt = (m << 3) & M32
        st.mdev = (m << 1) & M32
        st.mdev_max = st.rttvar = max(st.mdev, 0)
        st.rtt_seq = st.snd_nxt


def UpdateRetransmissionTimer(st, cur_ts):           # timer.c:149-173; returns the flags
    flags = 0
    st.nrtx = 0
    if st.on_rto:                                    # :157-159, RemoveFromRTOList
        st.on_rto = 0
        flags |= ACK_RTO_REMOVE
    if TCP_SEQ_GT(st.snd_nxt, st.snd_una):           # :162-166, AddtoRTOList
        st.ts_rto = (cur_ts + st.rto) & M32
        st.on_rto = 1
        flags |= ACK_RTO_ADD
    return flags


def ProcessACK(st, cur_ts, seq, ack_seq, window, payloadlen, ts_lastack_rcvd):
    """tcp_in.c:302-531 on st (tcph->syn clear, ESTABLISHED).  Returns (verdict,
    flags, rmlen).  Raises Arith where C's int arithmetic is undefined; st may
    be half changed then (the caller walks a copy)."""
    flags = 0
    cwindow = (window << st.wscale_peer) & M32                   # :315-318
    right_wnd_edge = (st.peer_wnd + st.snd_wl2) & M32            # :319
    if TCP_SEQ_GT(ack_seq, (st.sb_head_seq + st.sb_len) & M32):  # :332-338
        return ACK_BEYOND, 0, 0
    if (TCP_SEQ_LT(st.snd_wl1, seq) or (st.snd_wl1 == seq and TCP_SEQ_LT(st.snd_wl2, ack_seq)) or
            (st.snd_wl2 == ack_seq and cwindow > st.peer_wnd)):  # :341-349
        cwindow_prev = st.peer_wnd
        st.peer_wnd = cwindow
        st.snd_wl1 = seq
        st.snd_wl2 = ack_seq
        flags |= ACK_WND_UPDATE
        outstanding = (st.snd_nxt - st.snd_una) & M32
        if cwindow_prev < outstanding and st.peer_wnd >= outstanding:   # :355-363
            flags |= ACK_WRITE_EVENT_WND
    dup = False                                                  # :375-389
    if TCP_SEQ_LT(ack_seq, st.snd_nxt):
        if ack_seq == st.last_ack_seq and payloadlen == 0:
            if (st.snd_wl2 + st.peer_wnd) & M32 == right_wnd_edge:
                if st.dup_acks + 1 > st.dup_acks:                # in int: always
                    st.dup_acks = (st.dup_acks + 1) & 0xFF       # a uint8_t
                dup = True
                flags |= ACK_DUP
    if not dup:
        st.dup_acks = 0
        st.last_ack_seq = ack_seq
    if dup and st.dup_acks == 3:                                 # :392-426
        if TCP_SEQ_LT(ack_seq, st.snd_nxt):
            st.snd_nxt = ack_seq
        st.ssthresh = min(st.cwnd, st.peer_wnd) // 2
        if st.ssthresh < 2 * st.mss:
            st.ssthresh = 2 * st.mss
        st.cwnd = (st.ssthresh + 3 * st.mss) & M32
        if st.nrtx < ACK_MAX_RTX:
            st.nrtx += 1
        flags |= ACK_FAST_RTX
    elif st.dup_acks > 3:                                        # :428-435
        if (st.cwnd + st.mss) & M32 > st.cwnd:
            st.cwnd += st.mss
    if TCP_SEQ_GT(ack_seq, st.snd_nxt):                          # :444-455
        st.snd_nxt = ack_seq
        flags |= ACK_SND_NXT_RECOVERED
        if st.sb_len == 0:
            flags |= ACK_SEND_LIST_REMOVE
    if TCP_SEQ_GEQ(st.sb_head_seq, ack_seq):                     # :459-461
        return ACK_OLD, flags, 0
    rmlen = (ack_seq - st.sb_head_seq) & M32                     # :464
    removed = 0
    if rmlen > 0:
        packets = (rmlen // st.eff_mss) & 0xFFFF                 # :467-473, a uint16_t
        if ((rmlen // st.eff_mss) * st.eff_mss) & M32 > rmlen:
            packets = (packets + 1) & 0xFFFF
        if st.saw_timestamp:                                     # :476-480
            EstimateRTT(st, (cur_ts - ts_lastack_rcvd) & M32)
            st.rto = ((st.srtt >> 3) + st.rttvar) & M32
        if st.cwnd < st.ssthresh:                                # :487-504
            if (st.cwnd + st.mss) & M32 > st.cwnd:
                if st.mss * packets > INT_MAX:
                    raise Arith()
                st.cwnd = (st.cwnd + st.mss * packets) & M32
        else:
            if packets * st.mss > INT_MAX or packets * st.mss * st.mss > INT_MAX or st.cwnd == 0:
                raise Arith()
            new_cwnd = (st.cwnd + packets * st.mss * st.mss // st.cwnd) & M32
            if new_cwnd > st.cwnd:
                st.cwnd = new_cwnd
        to_remove = min(rmlen, st.sb_len)                        # SBRemove, tcp_send_buffer.c:149-173
        if to_remove > 0:
            st.sb_head_seq = (st.sb_head_seq + to_remove) & M32
            st.sb_len -= to_remove
            removed = to_remove
        st.snd_una = ack_seq                                     # :512-514
        snd_wnd_prev = st.snd_wnd
        st.snd_wnd = (st.sb_size - st.sb_len) & M32
        if snd_wnd_prev <= 0:                                    # :519-523
            flags |= ACK_WRITE_EVENT_ROOM
        flags |= UpdateRetransmissionTimer(st, cur_ts)           # :527
    return ACK_NEW, flags, removed


def rec(rmlen=0, snd_nxt=0, cwnd=0, flags=0, verdict=0, dup_acks=0):
    return (rmlen, snd_nxt, cwnd, flags, verdict, dup_acks)


def step(st, pkt, cur_ts, deferral=True):
    """One packet of one stream: pkt = (seq, ack_seq, ts_ref, window,
    payload_len, tcp_flags, rcv_verdict, has_ts).  rcv_verdict: the placement
    record's; has_ts: an option record with TS_FOUND.  Returns the record
    tuple; a DEFER_* verdict leaves st as it was.  deferral=False: the plain
    reference walk of a valid packet (no tests in front of tcp_in.c:864)."""
    seq, ack_seq, ts_ref, window, payloadlen, tcp_flags, rcv_verdict, has_ts = pkt
    if deferral:
        if st.bad():
            return rec(verdict=DEFER_BAD_STATE)
        if st.tcp_state != ACK_ST_ESTABLISHED:
            return rec(verdict=DEFER_STATE)
        if tcp_flags & (TCP_FIN | TCP_SYN | TCP_RST):
            return rec(verdict=DEFER_FLAGS)
        valid = RCV_FIRST_VALID <= rcv_verdict <= RCV_LAST
        if not RCV_FIRST_WALKED <= rcv_verdict <= RCV_LAST or (valid and st.saw_timestamp and not has_ts):
            return rec(verdict=DEFER_RCV)
        if not valid:
            return rec(0, st.snd_nxt, st.cwnd, 0, NOT_VALID, st.dup_acks)
    if not tcp_flags & TCP_ACK:                                  # :864
        return rec(0, st.snd_nxt, st.cwnd, 0, NO_ACK_FLAG, st.dup_acks)
    if not st.has_sndbuf:                                        # :865
        return rec(0, st.snd_nxt, st.cwnd, 0, NO_SNDBUF, st.dup_acks)
    work = st.copy()
    try:
        verdict, flags, rmlen = ProcessACK(work, cur_ts, seq, ack_seq, window, payloadlen, ts_ref)
    except Arith:
        if not deferral:
            raise
        return rec(verdict=DEFER_ARITH)
    for f in CHANGED:
        setattr(st, f, getattr(work, f))
    return rec(rmlen, st.snd_nxt, st.cwnd, flags, verdict, st.dup_acks)


def packets_of(res, opt, place):
    """The walk's per-packet inputs as Python tuples."""
    n = len(res)
    z = [0] * n
    cols = [res["seq"].tolist(), res["ack_seq"].tolist(), opt["ts_ref"].tolist() if opt is not None else z,
            res["window"].tolist(), res["payload_len"].tolist(), res["tcp_flags"].tolist(), place["verdict"].tolist(),
            [bool(f & TCPOPT_TS_FOUND) for f in opt["flags"].tolist()] if opt is not None else z]
    return list(zip(*cols))


def walk(res, opt, place, max_id, idx, seg_sid, seg_start, cur_ts, snd):
    """The whole call: returns (ack[n], snd', ack_stop[m]); `snd` is not changed."""
    n, m = len(res), len(seg_sid)
    pk = packets_of(res, opt, place)
    out = np.zeros(n, ACK_REC_DTYPE)
    rows = [None] * n
    new_snd = snd.copy()
    ack_stop = np.zeros(m, np.uint32)
    idx_l, start_l = [int(x) for x in idx], [int(x) for x in seg_start]
    for j, sid in enumerate(int(x) for x in seg_sid):
        a, b = start_l[j], start_l[j + 1]
        if sid > max_id:
            assert sid in (FLOW_MISS, FLOW_NONE)
            ack_stop[j] = a
            continue
        st = Snd.from_record(snd[sid])
        stop, walked = b, False
        for k in range(a, b):
            p = idx_l[k]
            if stop != b:
                rows[p] = rec(verdict=DEFER_BEHIND)
                continue
            rows[p] = step(st, pk[p], cur_ts)
            if rows[p][4] in DEFERS:
                stop = k
            else:
                walked = True
        ack_stop[j] = stop
        if walked:
            st.to_record(new_snd, sid)
    got = [r for r in rows if r is not None]
    if got:
        sel = np.array([i for i, r in enumerate(rows) if r is not None])
        arr = np.array(got, dtype=np.int64)
        for c, f in enumerate(("rmlen", "snd_nxt", "cwnd", "flags", "verdict", "dup_acks")):
            out[f][sel] = arr[:, c]
    return out, new_snd, ack_stop
