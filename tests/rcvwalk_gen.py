"""Batches for the receive walk's tests (tests/test_rcvwalk_model.py asserts the
family's statistics on the CPU, tests/test_gpu_rcvwalk.py runs it on the GPU).

A batch is what mtcp_gpu_rcvwalk[_dev] reads: rx records, option records, the
stream id of every packet and the state array.  Streams send in-order
segments of 1-1460 B; a segment in eight is delayed by 1-8 places, after every
segment an earlier one is sent again with probability 1/16.  On top, packets
aimed at the verdicts that ordinary reordering does not reach: each is built
from the model's state of its stream at that point (a stale or missing
timestamp, a window probe, a segment beyond the window, an ACK, a segment that
starts before the buffer's head, one that passes the buffer's end while the
initial window is still advertised).  Deferrals (FIN, another state, an
unpinned timestamp walk, a bad record) are rare.
"""
import numpy as np

from mtcp_amd._types import (RCV_STATE_DTYPE, RESULT_DTYPE, TCPOPT_DTYPE, TCPOPT_TS_FOUND, TCPOPT_TS_UNPINNED)
from tests import rcvwalk_model as rm

M32 = 0xFFFFFFFF
ACK, PSH, FIN = 0x10, 0x08, 0x01
TCP_INITIAL_WINDOW = 14600            # tcp_in.h:35: rcv_wnd before the first payload


def record_of(st):
    """One RCV_STATE_DTYPE record of a model stream (at most four fragments)."""
    r = np.zeros(1, RCV_STATE_DTYPE)
    r["head_seq"], r["size"], r["tcp_state"], r["saw_timestamp"] = st.head_seq, st.size, st.tcp_state, st.saw_timestamp
    r["rsvd"] = st.rsvd
    st.stored = True
    st.to_record(r, 0)
    return r[0]


def initial_stream(rng, wrap=False):
    """A stream somewhere in its life: fresh behind the handshake (three in ten
    with a 4 096 B buffer and the initial window still advertised), or after
    some in-order and out-of-order data and an application read."""
    saw_ts = int(rng.integers(0, 2))
    irs = int(M32 - rng.integers(0, 2000)) if wrap or rng.random() < 0.2 else int(rng.integers(0, 1 << 32))
    ts = int(rng.integers(0, 1 << 32))
    if rng.random() < 0.3:
        st = rm.Stream.fresh(irs, 4096, saw_ts, ts)
        st.rcv_wnd = TCP_INITIAL_WINDOW
        return st
    st = rm.Stream.fresh(irs, 4096 if rng.random() < 0.3 else 65536, saw_ts, ts)
    nxt = st.rcv_nxt
    for _ in range(int(rng.integers(0, 4))):              # what earlier bursts left
        ln = int(rng.integers(1, 600))
        hole = int(rng.integers(0, 2)) * int(rng.integers(1, 300))
        rm.step(st, ((nxt + hole) & M32, ts, 0, ln, ACK, TCPOPT_TS_FOUND), deferral=False)
        nxt = (nxt + hole + ln) & M32 if not hole else nxt
    if rng.random() < 0.5:
        rm.app_read(st, int(rng.integers(0, 2000)))
    if len(st.frags) > 4:
        return initial_stream(rng, wrap)
    return st


def stream_packets(rng, st, k, defers=True):
    """k packets for a stream whose state is `st` (a copy is walked along), as
    (seq, ts_val, ts_ref, payload_len, tcp_flags, opt_flags) tuples.  defers:
    with the rare FIN and unpinned option record."""
    st = rm.Stream.from_record(record_of(st))
    ts = st.ts_recent
    nxt = st.rcv_nxt                                       # send from rcv_nxt, or behind the last fragment
    if len(st.frags) > 1 and rng.random() < 0.3:
        nxt = (st.frags[-1][0] + st.frags[-1][1]) & M32
    sent, queue, out = [], [], []
    max_len = max(1, min(1460, (st.size - st.merged_len) // (k + 1)))     # the batch fits the buffer: nobody reads meanwhile
    while len(out) < k:
        r = rng.random()
        ts = (ts + int(rng.integers(0, 3))) & M32
        of = TCPOPT_TS_FOUND
        tf = ACK | (PSH if rng.random() < 0.3 else 0)
        tv = ts
        seq = None
        if queue and queue[0][0] <= len(out):              # a delayed segment's turn
            _, seq, ln = queue.pop(0)
        elif st.rcv_wnd > st.size - st.merged_len and st.size <= 65536 and rng.random() < 0.8:
            seq, ln = (st.head_seq + st.size - int(rng.integers(0, 100))) & M32, int(rng.integers(101, 1400))
        elif r < 0.020:
            seq, ln = (st.rcv_nxt - 1) & M32, int(rng.integers(0, 2))            # a window probe
        elif r < 0.040:
            seq, ln = (st.rcv_nxt + st.rcv_wnd + int(rng.integers(1, 3000))) & M32, int(rng.integers(1, 1461))
        elif r < 0.060:
            seq, ln = st.rcv_nxt, 0                        # an ACK
        elif r < 0.080:
            if st.saw_timestamp:
                of = 0                                     # no timestamp option
                seq, ln = st.rcv_nxt, int(rng.integers(1, max_len + 1))
        elif r < 0.100:
            if st.saw_timestamp:
                tv = (st.ts_recent - int(rng.integers(1, 1000))) & M32           # a stale one
                seq, ln = st.rcv_nxt, int(rng.integers(1, max_len + 1))
        elif r < 0.130:
            if st.merged_len < 8000:
                back = int(rng.integers(1, 400))           # starts before the buffer's head, ends inside the window
                seq, ln = (st.head_seq - back) & M32, back + st.merged_len + int(rng.integers(0, 50))
        elif r < 0.132:
            if defers:
                seq, ln, tf = nxt, int(rng.integers(0, 100)), tf | FIN               # deferred: FIN
        elif r < 0.133:
            if st.saw_timestamp and defers:
                seq, ln, of = nxt, int(rng.integers(1, 100)), TCPOPT_TS_UNPINNED     # deferred: the walk is unpinned
        elif sent and r < 0.133 + 1 / 16:
            seq, ln = sent[int(rng.integers(0, len(sent)))]                      # an earlier one again
        if seq is None:
            seq, ln = nxt, int(rng.integers(1, max_len + 1))
            nxt = (nxt + ln) & M32
            sent.append((seq, ln))
            if rng.random() < 1 / 8:                       # delayed by 1-8 places
                queue.append((len(out) + int(rng.integers(1, 9)), seq, ln))
                queue.sort()
                continue
        pkt = (seq, tv if of & TCPOPT_TS_FOUND else 0, int(rng.integers(0, 1 << 32)) if of & TCPOPT_TS_FOUND else 0,
               ln, tf, of)
        rm.step(st, pkt)                                   # deferred packets leave st alone
        out.append(pkt)
    return out


def batch(rng, lens, max_id=None, extra=0, wrap=False, with_opt=True, special=None, defers=True):
    """A batch of sum(lens) + extra packets: len(lens) streams with lens[s]
    packets each, interleaved at random (a stream's packets keep their order),
    and `extra` packets of the MISS and NONE classes.  special(rng, s, st):
    optional, changes stream s's initial state.  Returns a dict: res, opt, sid,
    state, max_id (the ids are spread over 0..max_id; the other records hold
    streams of their own, which the walk must leave alone)."""
    ns = len(lens)
    max_id = max(2 * ns, 8) if max_id is None else max_id
    ids = np.sort(rng.choice(max_id + 1, ns, replace=False)) if ns else np.zeros(0, np.int64)
    state = np.zeros(max_id + 1, RCV_STATE_DTYPE)
    for i in range(max_id + 1):
        state[i] = record_of(initial_stream(rng, wrap))
    n = int(sum(lens)) + extra
    owner = np.concatenate([np.repeat(np.arange(ns), lens), np.full(extra, -1)]).astype(np.int64)
    rng.shuffle(owner)
    res, opt = np.zeros(n, RESULT_DTYPE), np.zeros(n, TCPOPT_DTYPE)
    raw = rng.integers(0, 256, n * 40, dtype=np.uint8).view(RESULT_DTYPE)       # the fields the walk does not read
    for f in ("saddr", "daddr", "sport", "dport", "ack_seq", "window", "rss_hash", "ihl_doff"):
        res[f] = raw[f]
    sid = np.zeros(n, np.uint32)
    cols = {f: np.zeros(n, np.int64) for f in ("seq", "tv", "tr", "ln", "tf", "of")}
    for s in range(ns):
        st = rm.Stream.from_record(state[ids[s]])
        if special is not None:                            # a Stream, or a raw record
            alt = special(rng, s, st)
            if alt is not None:
                state[ids[s]] = alt if isinstance(alt, np.void) else record_of(alt)
                st = rm.Stream.from_record(state[ids[s]])
        pk = stream_packets(rng, st, int(lens[s]), defers) if not st.bad() else \
            [(int(rng.integers(0, 1 << 32)), 0, 0, 100, ACK, 0)] * int(lens[s])
        at = np.nonzero(owner == s)[0]
        sid[at] = ids[s]
        for c, f in enumerate(("seq", "tv", "tr", "ln", "tf", "of")):
            cols[f][at] = [p[c] for p in pk]
    rest = np.nonzero(owner < 0)[0]
    sid[rest] = np.where(rng.random(len(rest)) < 0.5, rm.FLOW_MISS, rm.FLOW_NONE)
    for f in ("seq", "tv", "tr"):
        cols[f][rest] = rng.integers(0, 1 << 32, len(rest))
    cols["ln"][rest], cols["tf"][rest] = rng.integers(0, 1461, len(rest)), ACK
    res["seq"], res["payload_len"], res["tcp_flags"] = cols["seq"], cols["ln"], cols["tf"]
    res["ip_len"] = 40 + cols["ln"]
    opt["ts_val"], opt["ts_ref"], opt["flags"] = cols["tv"], cols["tr"], cols["of"]
    return {"res": res, "opt": opt if with_opt else None, "sid": sid, "state": state, "max_id": max_id}


def family_lens(rng, ns):
    """Packets per stream of the random family: 1-40, a few long ones."""
    lens = rng.integers(1, 41, ns)
    lens[rng.random(ns) < 0.02] = rng.integers(65, 200)
    return lens


def family_special(rng, s, st):
    """One stream in a hundred each: another state, a bad record."""
    r = rng.random()
    if r < 0.01:
        st.tcp_state = int(rng.choice([3, 5, 7, 10]))
        return st
    if r < 0.02:
        st.rsvd = 1
        return st
    return None


def garbage_batch(rng, ns, per):
    """ns streams of `per` packets over states of 64 random bytes.  Every
    other record gets sane small fields (so that it passes the bad test and is
    walked), every fourth fragments and a window near the packets' sequence
    numbers; seven packets in ten land near their stream's head_seq."""
    raw = lambda r, s, st: rng.integers(0, 256, 64, dtype=np.uint8).view(RCV_STATE_DTYPE)[0]
    b = batch(rng, [per] * ns, special=raw)
    S, n = b["state"], len(b["res"])
    ev = np.arange(0, len(S), 2)
    S["rsvd"][ev], S["tcp_state"][ev] = 0, 4
    S["saw_timestamp"][ev] = rng.integers(0, 2, len(ev)) * rng.integers(1, 256, len(ev))
    b["opt"]["flags"] = np.where(rng.random(n) < 0.9, TCPOPT_TS_FOUND, 0)
    b["opt"]["ts_val"] = rng.integers(0, 1 << 32, n)
    S["nfrag"][ev] = rng.integers(0, 5, len(ev))
    S["size"][ev] = 1 << rng.integers(10, 31, len(ev))
    S["merged_len"][ev] = (rng.random(len(ev)) * (S["size"][ev] + 1)).astype(np.uint32)
    S["frag"]["len"][ev] &= 0x7FFFFFFF
    q = np.arange(0, len(S), 4)
    S["frag"]["seq"][q] = S["head_seq"][q, None] + rng.integers(0, 3000, (len(q), 4)).astype(np.uint32)
    S["frag"]["len"][q] = rng.integers(0, 3000, (len(q), 4))
    S["rcv_nxt"][q] = S["head_seq"][q] + S["merged_len"][q]
    S["rcv_wnd"][q] = S["size"][q] - S["merged_len"][q]
    near = S["head_seq"][np.minimum(b["sid"], b["max_id"])] + rng.integers(0, 5000, n).astype(np.uint32)
    b["res"]["seq"] = np.where(rng.random(n) < 0.7, near, b["res"]["seq"])
    return b
