"""Batches for the ProcessACK walk's tests (tests/test_ackwalk_model.py asserts
the family's statistics on the CPU, tests/test_gpu_ackwalk.py runs it on the
GPU), on top of tests/rcvwalk_gen.py's: one batch feeds both walks.

A batch is rcvwalk_gen's (rx records, option records, the stream id of every
packet, the receive states) with runs of pure ACKs put between a stream's data
segments (a duplicate ACK has no payload, tcp_in.c:377), the grouping, the
receive model's placement records, and the send side: a send state per stream
id and, written into the rx records, the ack_seq and window of every packet.
The ACKs of a stream are made from the ACK model's state of that stream at
that point: new data (through slow start and congestion avoidance), runs of
duplicates into a fast retransmit and the ACK above snd_nxt behind it, old
ACKs, ACKs beyond the buffer, window changes of all three kinds, a full send
buffer.  Deferrals (FIN, another state, a bad record) are rare.
"""
import numpy as np

from mtcp_amd._types import ACK_STATE_DTYPE, TCPOPT_TS_FOUND
from tests import ackwalk_model as am
from tests import group_model as gm
from tests import rcvwalk_gen as rg
from tests import rcvwalk_model as rm

M32 = 0xFFFFFFFF
ACK, FIN = 0x10, 0x01
CUR_TS = 0x00F00000


def record_of(s, user=None):
    """One ACK_STATE_DTYPE record of a model stream."""
    r = np.zeros(1, ACK_STATE_DTYPE)
    for f in am.Snd.__slots__:
        r[f] = getattr(s, f)
    if user is not None:
        r["user"] = user
    return r[0]


def initial_snd(rng, saw_timestamp, wrap=False):
    """A send side somewhere in its life: data queued, most of it sent, a
    window, a congestion window in slow start or past it, an RTT estimate or
    none, some already two duplicates into a loss."""
    s = am.Snd()
    s.saw_timestamp = saw_timestamp
    s.mss = 536 if rng.random() < 0.2 else 1460
    s.eff_mss = s.mss - 12 if saw_timestamp else s.mss
    s.wscale_peer = 0 if rng.random() < 0.3 else int(rng.integers(0, 8))
    s.sb_size = 8192 if rng.random() < 0.2 else 65536
    iss = int(M32 - rng.integers(0, 20000)) if wrap or rng.random() < 0.2 else int(rng.integers(0, 1 << 32))
    full = rng.random() < 0.1
    s.sb_len = s.sb_size if full else int(rng.integers(0, s.sb_size + 1)) if rng.random() < 0.9 else 0
    s.sb_head_seq = s.snd_una = s.last_ack_seq = s.snd_wl2 = iss
    sent = s.sb_len if rng.random() < 0.7 else int(rng.integers(0, s.sb_len + 1))
    s.snd_nxt = (iss + sent) & M32
    s.snd_wnd = s.sb_size - s.sb_len
    s.peer_wnd = int(rng.integers(100, 60000)) << s.wscale_peer
    if rng.random() < 0.15:
        s.peer_wnd = int(rng.integers(0, sent + 1))
    s.snd_wl1 = int(rng.integers(0, 1 << 32))
    slow = rng.random() < 0.5
    s.cwnd = s.mss * int(rng.integers(1, 4) if slow else rng.integers(2, 60))
    s.ssthresh = s.mss * int(rng.integers(4, 12)) if slow else s.mss * int(rng.integers(2, 30))
    s.rto, s.ts_rto = int(rng.integers(1, 300)), int(rng.integers(0, 1 << 32))
    if rng.random() < 0.6:
        s.srtt, s.mdev = int(rng.integers(8, 2000)), int(rng.integers(0, 300))
        s.mdev_max = s.mdev + int(rng.integers(0, 50))
        s.rttvar = s.mdev_max + int(rng.integers(0, 50))
    s.rtt_seq = (iss - 1 - int(rng.integers(0, 1000))) & M32 if rng.random() < 0.5 else \
        (iss + int(rng.integers(0, s.sb_len + 1000))) & M32
    s.dup_acks = int(rng.choice([0, 0, 1, 2, 2, 2, 3, 5, 254, 255])) if sent else 0
    s.nrtx = int(rng.integers(0, 17)) if rng.random() < 0.2 else 0
    s.on_rto = int(rng.integers(0, 2))
    s.has_sndbuf = 0 if rng.random() < 0.01 else 1
    return s


def stream_acks(rng, s, pkts, cur_ts):
    """(ack_seq, window) for the packets of one stream, in list order.  pkts:
    (seq, ts_ref, payload_len, tcp_flags, rcv_verdict, has_ts) per packet; a
    copy of s is walked along."""
    s = s.copy()
    window = min(0xFFFF, s.peer_wnd >> min(s.wscale_peer, 31))
    out = []
    for seq, ts_ref, ln, tf, rv, has_ts in pkts:
        r = rng.random()
        head, can_dup = s.sb_head_seq, am.TCP_SEQ_LT(s.last_ack_seq, s.snd_nxt)
        new = (head + int(rng.integers(1, min(s.sb_len, 3 * s.mss) + 1))) & M32 if s.sb_len else head
        if ln == 0 and can_dup and r < 0.85:
            ack = s.last_ack_seq                           # a duplicate
        elif r < 0.04:
            ack = (head - int(rng.integers(0, 3000))) & M32    # old
        elif r < 0.06:
            ack = (head + s.sb_len + int(rng.integers(1, 3000))) & M32   # beyond the buffer
        elif r < 0.10 and s.sb_len <= 65536:
            ack = (head + s.sb_len) & M32                  # all of it (a long stream keeps its larger buffer)
        elif r < 0.20:
            ack = s.snd_wl2                                # the same ACK, another window
            window = int(rng.integers(0, 0x10000)) if rng.random() < 0.5 else min(0xFFFF, window + int(rng.integers(1, 300)))
        else:
            ack = new
            if r > 0.95:
                window = int(rng.integers(0, 0x10000))
        out.append((ack, window))
        am.step(s, (seq, ack, ts_ref, window, ln, tf, rv, has_ts), cur_ts)
    return out


def _with_pure_acks(inner):
    """rcvwalk_gen.stream_packets with runs of 1-5 pure ACKs (seq = rcv_nxt, the
    timestamp the stream last saw) between the data segments: they leave the
    receive state alone, so the segments behind them stay what rcvwalk_gen made."""
    def packets(rng, st, k, defers=True):
        n_ack = int(rng.binomial(k, 0.3))
        data = inner(rng, st, k - n_ack, defers)
        st = rm.Stream.from_record(rg.record_of(st))
        runs = []
        left = n_ack
        while left:
            run = min(left, int(rng.integers(1, 6)))
            runs.append((int(rng.integers(0, len(data) + 1)), run))
            left -= run
        runs.sort()
        out, at = [], 0
        for pos, run in runs + [(len(data), 0)]:
            for p in data[at:pos]:
                rm.step(st, p)
                out.append(p)
            at = pos
            for _ in range(run):
                of = TCPOPT_TS_FOUND
                out.append((st.rcv_nxt, st.ts_recent, int(rng.integers(0, 1 << 32)), 0, ACK, of))
        assert len(out) == k
        return out
    return packets


def batch(rng, lens, max_id=None, extra=0, wrap=False, with_opt=True, special=None, snd_special=None, fin=0.0003,
          noack=0.005, cur_ts=CUR_TS):
    """rcvwalk_gen.batch(rng, lens, ...) with pure ACKs, then the send side.
    special(rng, s, st): changes stream s's receive state; snd_special(rng, s,
    snd): its send state (a Snd, or a raw record).  fin: the share of packets
    that get a FIN (deferred by both walks); noack: of packets without the
    ACK flag (tcp_in.c:864).  Returns rcvwalk_gen's dict plus
    group, place (the receive model's), rcv_want (its whole answer), snd and
    cur_ts."""
    inner = rg.stream_packets
    rg.stream_packets = _with_pure_acks(inner)
    try:
        b = rg.batch(rng, lens, max_id, extra, wrap, True, special, defers=False)
    finally:
        rg.stream_packets = inner
    n, max_id = len(b["res"]), b["max_id"]
    res, opt, sid = b["res"], b["opt"], b["sid"]
    res["tcp_flags"] = np.where((rng.random(n) < fin) & (sid <= max_id), res["tcp_flags"] | FIN, res["tcp_flags"])
    res["tcp_flags"] = np.where(rng.random(n) < noack, res["tcp_flags"] & ~np.uint8(ACK), res["tcp_flags"])
    b["group"] = gm.group(sid, max_id)
    b["rcv_want"] = rm.walk(res, opt, max_id, *b["group"], b["state"])
    place = b["place"] = b["rcv_want"][0]
    snd = np.zeros(max_id + 1, ACK_STATE_DTYPE)
    user = rng.integers(0, 256, (max_id + 1, 40), dtype=np.uint8)
    for i in range(max_id + 1):
        snd[i] = record_of(initial_snd(rng, int(b["state"]["saw_timestamp"][i]), wrap), user[i])
    ids = np.unique(sid[sid <= max_id])
    order = np.argsort(sid, kind="stable")
    bounds = np.searchsorted(sid[order], ids, side="left").tolist() + [int((sid <= max_id).sum())]
    cols = [res["seq"].tolist(), opt["ts_ref"].tolist(), res["payload_len"].tolist(), res["tcp_flags"].tolist(),
            place["verdict"].tolist(), [bool(f & TCPOPT_TS_FOUND) for f in opt["flags"].tolist()]]
    for s, i in enumerate(int(x) for x in ids):
        at = order[bounds[s]:bounds[s + 1]]
        if snd_special is not None:
            alt = snd_special(rng, s, am.Snd.from_record(snd[i]))
            if alt is not None:
                snd[i] = alt if isinstance(alt, np.void) else record_of(alt, user[i])
        st = am.Snd.from_record(snd[i])
        if st.bad():
            continue                                       # res keeps rcvwalk_gen's random ack_seq and window
        acks = stream_acks(rng, st, [tuple(c[p] for c in cols) for p in at.tolist()], cur_ts)
        res["ack_seq"][at] = [a for a, _ in acks]
        res["window"][at] = [w for _, w in acks]
    b["snd"], b["cur_ts"] = snd, cur_ts
    if not with_opt:
        drop_options(b)
    return b


def drop_options(b):
    """The same batch without option records: the receive answer changes with it."""
    b["opt"] = None
    b["rcv_want"] = rm.walk(b["res"], None, b["max_id"], *b["group"], b["state"])
    b["place"] = b["rcv_want"][0]
    b.pop("want", None)
    return b


def expect(b):
    """The ACK model's whole answer for batch b: (ack, snd', ack_stop)."""
    if "want" not in b:
        b["want"] = am.walk(b["res"], b["opt"], b["place"], b["max_id"], *b["group"], b["cur_ts"], b["snd"])
    return b["want"]


def family_lens(rng, ns):
    """Packets per stream of the random family: 1-40, a few long ones."""
    lens = rng.integers(1, 41, ns)
    lens[rng.random(ns) < 0.02] = rng.integers(65, 200)
    return lens


def family_special(rng, s, st):
    """One stream in three hundred: another receive state."""
    if rng.random() < 0.003:
        st.tcp_state = int(rng.choice([3, 5, 7, 10]))
        return st
    return None


def family_snd_special(rng, s, snd):
    """One stream in three hundred each: another state, a bad record."""
    r = rng.random()
    if r < 0.003:
        snd.tcp_state = int(rng.choice([3, 5, 7, 10]))
        return snd
    if r < 0.006:
        snd.rsvd = 1
        return snd
    return None


def family(seed=2025, ns=500, extra=150):
    """The random family the CPU statistics test and the GPU tests share."""
    rng = np.random.default_rng(seed)
    return batch(rng, family_lens(rng, ns), extra=extra, special=family_special, snd_special=family_snd_special)


def garbage_batch(rng, ns, per):
    """ns streams of `per` packets over send states of 128 random bytes.
    Every other record gets sane small fields (so that it passes the bad test
    and is walked) around the random words; the ACKs land near their stream's
    buffer; the placement records are random bytes too, half of them with a
    walked verdict."""
    b = batch(rng, [per] * ns, fin=0.0)
    S, n = b["snd"], len(b["res"])
    S[:] = rng.integers(0, 256, 128 * len(S), dtype=np.uint8).view(ACK_STATE_DTYPE)
    ev = np.arange(0, len(S), 2)
    S["rsvd"][ev], S["tcp_state"][ev], S["wscale_peer"][ev] = 0, 4, rng.integers(0, 32, len(ev))
    S["eff_mss"][ev] = np.maximum(S["eff_mss"][ev], 1)
    S["sb_size"][ev] = 1 << rng.integers(10, 31, len(ev))
    S["sb_len"][ev] = (rng.random(len(ev)) * (S["sb_size"][ev] + 1)).astype(np.uint32)
    q = np.arange(0, len(S), 4)                            # and every fourth a consistent small one: ACK_NEW is reached
    S["sb_size"][q], S["sb_len"][q] = 65536, rng.integers(0, 65537, len(q))
    S["snd_nxt"][q] = S["sb_head_seq"][q] + S["sb_len"][q]
    S["snd_una"][q] = S["last_ack_seq"][q] = S["sb_head_seq"][q]
    owner = np.minimum(b["sid"], b["max_id"])
    near = S["sb_head_seq"][owner] + rng.integers(-2000, 70000, n).astype(np.uint32)
    b["res"]["ack_seq"] = np.where(rng.random(n) < 0.8, near, b["res"]["ack_seq"])
    place = rng.integers(0, 256, 16 * n, dtype=np.uint8).view(b["place"].dtype).copy()
    place["verdict"] = np.where(rng.random(n) < 0.5, rng.integers(7, 16, n), place["verdict"])
    b["place"] = place
    b.pop("want", None)
    return b
