"""A literal Python restatement of the reference's receive walk for one
ESTABLISHED stream, with the deferral rules of include/mtcp_gpu_rcvwalk.h on top:

  ValidateSequence            mtcp/src/tcp_in.c:101-179
  Handle_TCP_ST_ESTABLISHED   its payload branch, tcp_in.c:854-862
  ProcessTCPPayload           tcp_in.c:537-610
  RBPut                       mtcp/src/tcp_ring_buffer.c:280-382 (its bookkeeping;
                              the copy at :315 and the compaction at :304-308
                              move no state this model keeps)

The reference's statements in the reference's order, over a Python list of
fragments of any length.  Every expected value of tests/test_rcvwalk_model.py
and tests/test_gpu_rcvwalk.py comes from here, never from the kernels.
"""
import numpy as np

from mtcp_amd._types import (FLOW_MISS, FLOW_NONE, RCV_ACK_AGGREGATE, RCV_ACK_NOW, RCV_COPY, RCV_MAX_FRAGS,
                             RCV_MAX_SIZE, RCV_PLACE_DTYPE, RCV_READ_EVENT, RCV_ST_ESTABLISHED, RCV_STATE_DTYPE,
                             RCV_TS_NEWER, RCV_VERDICTS, RESULT_DTYPE, TCPOPT_DTYPE, TCPOPT_TS_FOUND,
                             TCPOPT_TS_UNPINNED)

M32 = 0xFFFFFFFF
MAXSEQ = 0xFFFFFFFF                                   # tcp_ring_buffer.c:234
(NONE, DEFER_STATE, DEFER_BAD_STATE, DEFER_FLAGS, DEFER_TS, DEFER_FRAG_FULL, DEFER_BEHIND, PAWS_NO_TS, PAWS_OLD,
 SEQ_WINPROBE, SEQ_OLD, SEQ_AHEAD, ACK_ONLY, PUT_DROPPED, PUT_NO_ROOM, PUT_STORED) = range(16)
assert RCV_VERDICTS[PUT_STORED] == "PUT_STORED" and RCV_VERDICTS[DEFER_BEHIND] == "DEFER_BEHIND"
WALKED = tuple(range(PAWS_NO_TS, PUT_STORED + 1))
DEFERS = tuple(range(DEFER_STATE, DEFER_BEHIND + 1))
TCP_FIN, TCP_SYN, TCP_RST = 0x01, 0x02, 0x04


# ---- tcp_in.h:37-41 -----------------------------------------------------------------------------
def _s32(x):
    x &= M32
    return x - (1 << 32) if x & 0x80000000 else x


def TCP_SEQ_LT(a, b):
    return _s32(a - b) < 0


def TCP_SEQ_LEQ(a, b):
    return _s32(a - b) <= 0


def TCP_SEQ_GT(a, b):
    return _s32(a - b) > 0


def TCP_SEQ_GEQ(a, b):
    return _s32(a - b) >= 0


def TCP_SEQ_BETWEEN(a, b, c):
    return TCP_SEQ_GEQ(a, b) and TCP_SEQ_LEQ(a, c)


# ---- tcp_ring_buffer.c:234-254 ------------------------------------------------------------------
def GetMinSeq(a, b):
    if a == b:
        return a
    if a < b:
        return a if (b - a) <= MAXSEQ // 2 else b
    return b if (a - b) <= MAXSEQ // 2 else a


def GetMaxSeq(a, b):
    if a == b:
        return a
    if a < b:
        return b if (b - a) <= MAXSEQ // 2 else a
    return a if (a - b) <= MAXSEQ // 2 else b


class NullPrev(Exception):
    """RBPut's insert at tcp_ring_buffer.c:370-372 would follow a NULL prev."""


class Stream:
    """What the walk reads and writes of one tcp_stream, its tcp_recv_vars and
    its tcp_ring_buffer; frags: [seq, len] lists in list order."""
    __slots__ = ("rcv_nxt", "rcv_wnd", "head_seq", "merged_len", "size", "ts_recent", "ts_lastack_rcvd", "tcp_state",
                 "saw_timestamp", "rsvd", "nfrag_field", "frags", "stored")

    def __init__(self, rcv_nxt=0, rcv_wnd=0, head_seq=0, merged_len=0, size=0, ts_recent=0, ts_lastack_rcvd=0,
                 tcp_state=RCV_ST_ESTABLISHED, saw_timestamp=0, frags=(), rsvd=0, nfrag_field=None):
        self.rcv_nxt, self.rcv_wnd, self.head_seq, self.merged_len, self.size = rcv_nxt, rcv_wnd, head_seq, merged_len, size
        self.ts_recent, self.ts_lastack_rcvd, self.tcp_state = ts_recent, ts_lastack_rcvd, tcp_state
        self.saw_timestamp, self.rsvd = saw_timestamp, rsvd
        self.frags = [list(f) for f in frags]
        self.nfrag_field = len(self.frags) if nfrag_field is None else nfrag_field
        self.stored = False                          # a PUT_STORED rewrote the fragment slots

    @classmethod
    def fresh(cls, irs, size, saw_timestamp=0, ts_recent=0):
        """Behind the handshake: rcv_nxt = irs + 1, the whole buffer free, no ring buffer yet (tcp_in.c:555-566)."""
        return cls((irs + 1) & M32, size, (irs + 1) & M32, 0, size, ts_recent, 0, RCV_ST_ESTABLISHED, saw_timestamp)

    @classmethod
    def from_record(cls, r):
        nf = int(r["nfrag"])
        frags = [[int(r["frag"]["seq"][k]), int(r["frag"]["len"][k])] for k in range(min(nf, RCV_MAX_FRAGS))]
        return cls(int(r["rcv_nxt"]), int(r["rcv_wnd"]), int(r["head_seq"]), int(r["merged_len"]), int(r["size"]),
                   int(r["ts_recent"]), int(r["ts_lastack_rcvd"]), int(r["tcp_state"]), int(r["saw_timestamp"]),
                   frags, int(r["rsvd"]), nf)

    def to_record(self, a, i):
        """The bytes the walk changes, into element i of the RCV_STATE_DTYPE array a."""
        a["rcv_nxt"][i], a["rcv_wnd"][i], a["merged_len"][i] = self.rcv_nxt, self.rcv_wnd, self.merged_len
        a["ts_recent"][i], a["ts_lastack_rcvd"][i] = self.ts_recent, self.ts_lastack_rcvd
        if self.stored:
            assert len(self.frags) <= RCV_MAX_FRAGS
            a["nfrag"][i] = len(self.frags)
            a["frag"][i] = 0
            for k, (s, l) in enumerate(self.frags):
                a["frag"]["seq"][i, k], a["frag"]["len"][i, k] = s, l

    def bad(self):
        return (self.rsvd != 0 or self.nfrag_field > RCV_MAX_FRAGS or self.size > RCV_MAX_SIZE or
                self.merged_len > self.size or any(l >= 1 << 31 for _, l in self.frags))


# ---- RBPut, tcp_ring_buffer.c:280-382 -----------------------------------------------------------
def CanMerge(a, b):                                  # :256-266
    a_end = (a[0] + a[1] + 1) & M32
    b_end = (b[0] + b[1] + 1) & M32
    if GetMinSeq(a_end, b[0]) == a_end or GetMinSeq(b_end, a[0]) == b_end:
        return 0
    return 1


def MergeFragments(a, b):                            # :268-278, merge a into b
    min_seq = GetMinSeq(a[0], b[0])
    max_seq = GetMaxSeq((a[0] + a[1]) & M32, (b[0] + b[1]) & M32)
    b[0] = min_seq
    b[1] = ((max_seq - min_seq) & M32) & 0x7FFFFFFF  # uint32_t len : 31, tcp_ring_buffer.h:36


def RBPut(st, length, cur_seq, max_frags=None):
    """Returns (ret, putx).  The fragment list is a Python list; `next` is the
    list order, so prev / pprev are indices.  max_frags: a list that would grow
    past it raises FragFull before anything is changed."""
    if length <= 0:                                  # :290
        return 0, 0
    if GetMinSeq(st.head_seq, cur_seq) != st.head_seq:   # :294
        return 0, 0
    putx = (cur_seq - st.head_seq) & M32             # :297
    end_off = putx + length
    if st.size < end_off:                            # :299
        return -2, 0
    # :303-319 move bytes only
    frags = [list(f) for f in st.frags]              # walk on a copy: a deferral changes nothing
    new_ctx = [cur_seq, length]                      # :322-329
    in_list = -1                                     # where new_ctx sits in frags once it is an element of it
    merged = 0
    i, prev = 0, -1
    while i < len(frags):                            # :332-358
        it = frags[i]
        if CanMerge(new_ctx, it):
            MergeFragments(new_ctx, it)
            if prev >= 0 and prev == in_list:        # prev == new_ctx, :341-347
                del frags[prev]
                i -= 1
                prev = i - 1                         # prev = pprev
            new_ctx = frags[i]
            in_list = i
            merged = 1
        elif merged or GetMaxSeq((cur_seq + length) & M32, it[0]) == it[0]:
            break                                    # :352-357
        prev = i
        i += 1
    if not merged:                                   # :360-375
        if max_frags is not None and len(frags) >= max_frags:
            raise FragFull()
        if not frags:
            frags.append(new_ctx)
        elif GetMinSeq(cur_seq, frags[0][0]) == cur_seq:
            frags.insert(0, new_ctx)
        else:
            if prev < 0:
                raise NullPrev()
            frags.insert(prev + 1, new_ctx)          # prev->next = new_ctx; new_ctx->next = iter
    st.frags = frags
    st.stored = True
    if st.head_seq == frags[0][0]:                   # :376-379
        st.merged_len = frags[0][1]
    return length, putx


def RBRemove(st, length):                            # tcp_ring_buffer.c:384-421
    if st.merged_len < length:
        length = st.merged_len
    if length == 0:
        return 0
    st.head_seq = (st.head_seq + length) & M32
    st.merged_len -= length
    if length == st.frags[0][1]:
        del st.frags[0]
    elif length < st.frags[0][1]:
        st.frags[0][0] = (st.frags[0][0] + length) & M32
        st.frags[0][1] -= length
    else:
        assert 0
    st.stored = True
    return length


def app_read(st, length):
    """What mtcp_read does to the receive state between two bursts (api.c:1130-1131)."""
    RBRemove(st, length)
    st.rcv_wnd = (st.size - st.merged_len) & M32


class FragFull(Exception):
    """RBPut would end with more fragments than the caller's record has slots."""


# ---- ValidateSequence, tcp_in.c:101-179 (tcph->rst clear, state ESTABLISHED) --------------------
def ValidateSequence(st, seq, payloadlen, ts_found, ts_val, ts_ref):
    """Returns (TRUE/FALSE, verdict or None, flags, (ts_recent, ts_lastack_rcvd) to commit)."""
    flags = 0
    ts = (st.ts_recent, st.ts_lastack_rcvd)
    if st.saw_timestamp:                             # :106
        if not ts_found:                             # :109-115
            return False, PAWS_NO_TS, 0, ts
        if TCP_SEQ_LT(ts_val, st.ts_recent):         # :119-126
            return False, PAWS_OLD, RCV_ACK_NOW, ts
        if TCP_SEQ_GT(ts_val, st.ts_recent):         # :129-135
            flags |= RCV_TS_NEWER
        ts = (ts_val, ts_ref)                        # :137-138
    if not TCP_SEQ_BETWEEN((seq + payloadlen) & M32, st.rcv_nxt, (st.rcv_nxt + st.rcv_wnd) & M32):   # :143-144
        if (seq + 1) & M32 == st.rcv_nxt:            # :152-158
            return False, SEQ_WINPROBE, flags | RCV_ACK_AGGREGATE, ts
        if TCP_SEQ_LEQ(seq, st.rcv_nxt):             # :162-163
            return False, SEQ_OLD, flags | RCV_ACK_AGGREGATE, ts
        return False, SEQ_AHEAD, flags | RCV_ACK_NOW, ts   # :164-165
    return True, None, flags, ts


def place(put_off=0, rcv_nxt=0, rcv_wnd=0, put_len=0, verdict=0, flags=0):
    return (put_off, rcv_nxt, rcv_wnd, put_len, verdict, flags)


def step(st, pkt, has_opt=True, max_frags=RCV_MAX_FRAGS, deferral=True):
    """One packet of one stream: pkt = (seq, ts_val, ts_ref, payload_len,
    tcp_flags, opt_flags).  Returns the placement tuple; a DEFER_* verdict
    leaves st as it was.  deferral=False: the plain reference walk (no bad-state
    test, no fragment limit; the caller feeds it no SYN / RST / FIN)."""
    seq, ts_val, ts_ref, payloadlen, tcp_flags, opt_flags = pkt
    if deferral:
        if st.bad():
            return place(verdict=DEFER_BAD_STATE)
        if st.tcp_state != RCV_ST_ESTABLISHED:
            return place(verdict=DEFER_STATE)
        if tcp_flags & (TCP_FIN | TCP_SYN | TCP_RST):
            return place(verdict=DEFER_FLAGS)
        if st.saw_timestamp and (not has_opt or opt_flags & TCPOPT_TS_UNPINNED):
            return place(verdict=DEFER_TS)
    else:
        max_frags = None
    ok, verdict, flags, ts = ValidateSequence(st, seq, payloadlen, bool(opt_flags & TCPOPT_TS_FOUND), ts_val, ts_ref)
    if verdict in (PAWS_NO_TS, PAWS_OLD):
        return place(0, st.rcv_nxt, st.rcv_wnd, 0, verdict, flags)
    if not ok:
        st.ts_recent, st.ts_lastack_rcvd = ts
        return place(0, st.rcv_nxt, st.rcv_wnd, 0, verdict, flags)
    if not payloadlen > 0:                           # tcp_in.c:854
        st.ts_recent, st.ts_lastack_rcvd = ts
        return place(0, st.rcv_nxt, st.rcv_wnd, 0, ACK_ONLY, flags)
    # ProcessTCPPayload, tcp_in.c:537-610.  :546 and :550 test the two values ValidateSequence just passed
    assert not TCP_SEQ_LT((seq + payloadlen) & M32, st.rcv_nxt)
    assert not TCP_SEQ_GT((seq + payloadlen) & M32, (st.rcv_nxt + st.rcv_wnd) & M32)
    prev_rcv_nxt = st.rcv_nxt                        # :574
    try:
        ret, putx = RBPut(st, payloadlen, seq, max_frags)    # :575
    except FragFull:
        return place(verdict=DEFER_FRAG_FULL)
    except NullPrev:
        if not deferral:
            raise
        return place(verdict=DEFER_BAD_STATE)
    st.ts_recent, st.ts_lastack_rcvd = ts
    st.rcv_nxt = (st.head_seq + st.merged_len) & M32         # :588
    st.rcv_wnd = (st.size - st.merged_len) & M32             # :589
    if ret > 0:
        verdict, flags, put_len = PUT_STORED, flags | RCV_COPY, payloadlen
    else:
        verdict, put_len = (PUT_DROPPED if ret == 0 else PUT_NO_ROOM), 0
    if TCP_SEQ_LEQ(st.rcv_nxt, prev_rcv_nxt):        # :593 -> FALSE -> tcp_in.c:860
        flags |= RCV_ACK_NOW
    else:                                            # :606, TRUE -> tcp_in.c:858
        flags |= RCV_READ_EVENT | RCV_ACK_AGGREGATE
    return place(putx, st.rcv_nxt, st.rcv_wnd, put_len, verdict, flags)


def packets_of(res, opt):
    """The walk's per-packet inputs as Python tuples, from RESULT_DTYPE and TCPOPT_DTYPE (or None) arrays."""
    n = len(res)
    z = [0] * n
    cols = [res["seq"].tolist(), opt["ts_val"].tolist() if opt is not None else z,
            opt["ts_ref"].tolist() if opt is not None else z, res["payload_len"].tolist(), res["tcp_flags"].tolist(),
            opt["flags"].tolist() if opt is not None else z]
    return list(zip(*cols))


def walk(res, opt, max_id, idx, seg_sid, seg_start, state):
    """The whole call: returns (place[n], state', seg_stop[m]); `state` is not changed."""
    n, m = len(res), len(seg_sid)
    pk = packets_of(res, opt)
    out = np.zeros(n, RCV_PLACE_DTYPE)
    rows = [None] * n
    new_state = state.copy()
    seg_stop = np.zeros(m, np.uint32)
    idx_l, start_l = [int(x) for x in idx], [int(x) for x in seg_start]
    for j, sid in enumerate(int(x) for x in seg_sid):
        a, b = start_l[j], start_l[j + 1]
        if sid > max_id:
            assert sid in (FLOW_MISS, FLOW_NONE)
            seg_stop[j] = a
            continue
        st = Stream.from_record(state[sid])
        stop, walked = b, False
        for k in range(a, b):
            p = idx_l[k]
            if stop != b:
                rows[p] = place(verdict=DEFER_BEHIND)
                continue
            rows[p] = step(st, pk[p], opt is not None)
            if rows[p][4] in DEFERS:
                stop = k
            else:
                walked = True
        seg_stop[j] = stop
        if walked:
            st.to_record(new_state, sid)
    got = [r for r in rows if r is not None]
    if got:
        sel = np.array([i for i, r in enumerate(rows) if r is not None])
        arr = np.array(got, dtype=np.int64)
        for c, f in enumerate(("put_off", "rcv_nxt", "rcv_wnd", "put_len", "verdict", "flags")):
            out[f][sel] = arr[:, c]
    return out, new_state, seg_stop
