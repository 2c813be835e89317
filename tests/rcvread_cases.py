"""Inputs shared by tests/test_rcvread_model.py and tests/test_gpu_rcvread.py:
streams built with the model's own RBPut and reads (tests/rcvread_model.py), laid
out in an arena, and request lists over them.  Nothing here is an expectation."""
import numpy as np

from mtcp_amd._types import (ACK_STATE_DTYPE, ACKGEN_STATE_DTYPE, RCV_BUF_DTYPE, RCV_STATE_DTYPE, RCVREAD_ON_ACKQ,
                             RCVREAD_PEEK, RCVREAD_REQ_DTYPE)
from tests import rcvread_model as rm

GUARD = 64                                           # bytes kept free around every destination range


class Batch:
    """The mirrors of some streams, their arena, a request list and a
    destination region with GUARD bytes of 0x5A around every range."""

    def __init__(self, state, rbuf, tx, snd, arena):
        self.state, self.rbuf, self.tx, self.snd, self.arena = state, rbuf, tx, snd, arena
        self.max_id = len(state) - 1
        self.req = np.zeros(0, dtype=RCVREAD_REQ_DTYPE)
        self.dst = np.zeros(0, dtype=np.uint8)

    def requests(self, sids, lens, flags=None, dst_align=None, room=None):
        """One request per entry; range i begins GUARD bytes behind the end of
        range i - 1 at a 16 B phase of dst_align[i] and has room[i] bytes
        (default MIN(len, size) of the stream, 0 for a sid above max_id)."""
        n = len(sids)
        self.req = np.zeros(n, dtype=RCVREAD_REQ_DTYPE)
        self.req["sid"], self.req["len"] = sids, lens
        self.req["flags"] = 0 if flags is None else flags
        at = 0
        for i in range(n):
            sid = int(sids[i])
            size = int(self.rbuf["size"][sid]) if sid <= self.max_id else 0
            need = min(int(lens[i]), size) if room is None else int(room[i])
            at += GUARD
            if dst_align is not None:
                at += (int(dst_align[i]) - at) % 16
            self.req["dst_off"][i] = at
            at += need
        self.dst = np.full((at + GUARD + 15) & ~15, 0x5A, dtype=np.uint8)
        return self

    def copies(self):
        return (self.state.copy(), self.rbuf.copy(), None if self.tx is None else self.tx.copy(), self.snd,
                self.arena, self.dst.copy())

    def expect(self):
        """(state, rbuf, tx, dst, rres, total) by the model."""
        state, rbuf, tx, snd, arena, dst = self.copies()
        rres, total = rm.read(self.req, self.max_id, state, rbuf, tx, snd, arena, dst)
        return state, rbuf, tx, dst, rres, total


def lay_out(apps, rng=None, src_align=None, tcp_states=None):
    """The mirrors of a list of rcvread_model.App and an arena that holds their
    chunks one behind the other, chunk i at a 16 B phase of src_align[i]
    (default: random) with 32 bytes of 0xC3 in between."""
    n = len(apps)
    state, rbuf = np.zeros(n, dtype=RCV_STATE_DTYPE), np.zeros(n, dtype=RCV_BUF_DTYPE)
    tx, snd = np.zeros(n, dtype=ACKGEN_STATE_DTYPE), np.zeros(n, dtype=ACK_STATE_DTYPE)
    offs, at = [], 0
    for i, a in enumerate(apps):
        at += 32
        phase = int(src_align[i]) if src_align is not None else (int(rng.integers(16)) if rng is not None else 0)
        at += (phase - at) % 16
        offs.append(at)
        at += a.st.size
    arena = np.full((at + 32 + 15) & ~15, 0xC3, dtype=np.uint8)
    for i, a in enumerate(apps):
        s, b, t, d = rm.records_of(a, offs[i], 4 if tcp_states is None else int(tcp_states[i]))
        state[i], rbuf[i], tx[i], snd[i] = s[0], b[0], t[0], d[0]
        arena[offs[i]:offs[i] + a.st.size] = a.rb.data
        # fields the read must leave alone
        state["ts_recent"][i], state["ts_lastack_rcvd"][i], state["saw_timestamp"][i] = 0x11110000 + i, 0x22220000 + i, i & 1
        tx["saddr"][i], tx["ip_id"][i], tx["ts_lastack_sent"][i], tx["has_rcvbuf"][i] = 0x0A000001 + i, i & 0xFFFF, i, 1
        snd["mss"][i], snd["snd_nxt"][i], snd["tcp_state"][i] = 1460, 7 * i, 4
    return Batch(state, rbuf, tx, snd, arena)


def stream(rng, size, merged, head=0, extra_frags=0, eff_mss=64, need_wnd_adv=0, init_seq=None, serial=0):
    """An App with `merged` in-order bytes at head_offset `head`, and extra_frags
    further fragments behind holes."""
    init_seq = int(rng.integers(1 << 32)) if init_seq is None else init_seq
    a = rm.App(size, init_seq, eff_mss)
    nxt = init_seq
    total = head + merged
    assert total <= size
    if total:
        a.put(nxt, rm.payload_bytes(int(rng.integers(1 << 16)), serial, total))
        nxt = (nxt + total) & rm.M32
    if head:
        rm.RBRemove(a, head)
    for k in range(extra_frags):
        room = size - ((nxt - a.st.head_seq) & rm.M32)
        if room < 8:
            break
        gap, ln = 1 + int(rng.integers(3)), 1 + int(rng.integers(4))
        a.put((nxt + gap) & rm.M32, rm.payload_bytes(k, serial + 1 + k, ln))
        nxt = (nxt + gap + ln) & rm.M32
    a.st.rcv_wnd = a.st.size - a.st.merged_len
    a.need_wnd_adv = need_wnd_adv
    return a


def random_batch(rng, n_streams, n_req, sizes=(256, 512, 1024, 2048), dup=0.2, with_tx=True):
    """Streams of every shape the verdict chain distinguishes and a request list with duplicates."""
    apps, states = [], []
    for i in range(n_streams):
        size = int(rng.choice(sizes))
        merged = int(rng.integers(size + 1)) if rng.integers(8) else 0
        head = int(rng.integers(size - merged + 1)) if rng.integers(2) else 0
        apps.append(stream(rng, size, merged, head, int(rng.integers(4)), eff_mss=int(rng.integers(1, size)),
                           need_wnd_adv=int(rng.integers(2))))
        states.append(4 if rng.integers(10) else int(rng.integers(11)))
    b = lay_out(apps, rng, tcp_states=states)
    for i in range(n_streams):                       # one record in ten is broken in one of the BAD_STATE ways
        kind = int(rng.integers(80))
        if kind == 0:
            b.state["rsvd"][i] = 1
        elif kind == 1:
            b.state["size"][i] += 1
        elif kind == 2:
            b.rbuf["rsvd"][i, 1] = 1
        elif kind == 3:
            b.rbuf["last_len"][i] += 1
        elif kind == 4:
            b.state["frag"]["seq"][i, 0] += 1
        elif kind == 5:
            b.state["nfrag"][i] = 0
        elif kind == 6:
            b.state["frag"]["len"][i, 0] = int(b.state["merged_len"][i]) // 2
        elif kind == 7:
            b.rbuf["data_off"][i] = len(b.arena)
    if not with_tx:
        b.tx = b.snd = None
    sids = rng.integers(n_streams, size=n_req).astype(np.uint32)
    for i in range(1, n_req):
        if rng.random() < dup:
            sids[i] = sids[rng.integers(i)]
    if n_req > 4:
        sids[rng.integers(n_req)] = n_streams + int(rng.integers(1, 5))            # above max_id
    lens = np.where(rng.integers(4, size=n_req) == 0, rng.integers(1, 9, size=n_req),
                    rng.integers(0, 3000, size=n_req)).astype(np.uint32)
    flags = np.where(rng.integers(4, size=n_req) == 0, RCVREAD_PEEK, 0) | np.where(rng.integers(3, size=n_req) == 0,
                                                                                   RCVREAD_ON_ACKQ, 0)
    b.requests(sids, lens, flags.astype(np.uint32), dst_align=rng.integers(16, size=n_req))
    return b


def random_records(rng, n_streams, n_req, arena_bytes=4096, dst_bytes=4096):
    """Random bytes in every record array; every second record with the fields
    of the BAD tests made sane, so that the later rules are reached too."""
    raw = lambda dt, k: np.frombuffer(rng.bytes(dt.itemsize * k), dtype=dt).copy()
    state, rbuf = raw(RCV_STATE_DTYPE, n_streams), raw(RCV_BUF_DTYPE, n_streams)
    tx, snd = raw(ACKGEN_STATE_DTYPE, n_streams), raw(ACK_STATE_DTYPE, n_streams)
    for i in range(0, n_streams, 2):
        size = int(rng.integers(1, 1024))
        head = int(rng.integers(size))
        last = int(rng.integers(size - head + 1))
        merged = int(rng.integers(last + 1))
        rbuf[i] = (int(rng.integers(arena_bytes - size)), size, head, head + last, last, (0, 0))
        s = state[i]
        s["rsvd"], s["size"], s["merged_len"], s["nfrag"] = 0, size, merged, int(rng.integers(1, 5))
        s["frag"]["len"] &= 0x7FFFFFFF
        s["tcp_state"] = 4 if rng.integers(4) else int(rng.integers(11))
        if rng.integers(8):
            s["frag"]["seq"][0] = s["head_seq"]
            s["frag"]["len"][0] = merged + int(rng.integers(3)) if rng.integers(2) else merged
        tx["need_wnd_adv"][i], snd["eff_mss"][i] = int(rng.integers(3)), int(rng.integers(size))
    b = Batch(state, rbuf, tx, snd, np.frombuffer(rng.bytes(arena_bytes), dtype=np.uint8).copy())
    req = raw(RCVREAD_REQ_DTYPE, n_req)
    for i in range(n_req):
        if rng.integers(8):
            req["rsvd"][i] = 0
            req["flags"][i] &= 3
            req["sid"][i] = int(rng.integers(n_streams + 1))
            req["len"][i] = int(rng.integers(600))
            req["dst_off"][i] = int(rng.integers(dst_bytes - 512))
    b.req, b.dst = req, np.full(dst_bytes, 0x5A, dtype=np.uint8)
    # overlapping ranges are outside the purity clause: keep the accepted ones apart
    rres = b.expect()[4]
    at = 0
    for i in np.nonzero(rres["copylen"])[0]:
        b.req["dst_off"][i] = at + int(rng.integers(16))
        at += 16 + int(rres["copylen"][i]) + 15
    assert at <= dst_bytes
    return b


def direct(rng, sizes, merged, heads, src_align=None, eff_mss=64, need_wnd_adv=1):
    """Streams written as records at once (no RBPut): stream i has merged[i]
    in-order bytes at head_offset heads[i] as its one fragment; the arena holds
    random bytes."""
    n = len(sizes)
    state, rbuf = np.zeros(n, dtype=RCV_STATE_DTYPE), np.zeros(n, dtype=RCV_BUF_DTYPE)
    tx, snd = np.zeros(n, dtype=ACKGEN_STATE_DTYPE), np.zeros(n, dtype=ACK_STATE_DTYPE)
    sizes, merged, heads = (np.asarray(a, dtype=np.int64) for a in (sizes, merged, heads))
    phase = rng.integers(16, size=n) if src_align is None else np.asarray(src_align, dtype=np.int64)
    offs, at = np.zeros(n, dtype=np.int64), 0
    for i in range(n):                               # the run, not the chunk, gets the phase
        at += 32
        at += (int(phase[i]) - (at + int(heads[i]))) % 16
        offs[i] = at
        at += int(sizes[i])
    arena = rng.integers(0, 256, (at + 32 + 15) & ~15, dtype=np.uint8)
    head_seq = rng.integers(1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    head_seq[:1] = 0xFFFFFFF0                        # the first stream's head_seq wraps with a read of 16 bytes or more
    state["head_seq"], state["merged_len"], state["size"], state["tcp_state"] = head_seq, merged, sizes, 4
    state["rcv_nxt"], state["rcv_wnd"] = head_seq + merged.astype(np.uint32), sizes - merged
    state["nfrag"] = merged > 0
    state["frag"]["seq"][:, 0], state["frag"]["len"][:, 0] = np.where(merged > 0, head_seq, 0), merged
    rbuf["data_off"], rbuf["size"], rbuf["head_offset"] = offs, sizes, heads
    rbuf["tail_offset"], rbuf["last_len"] = heads + merged, merged
    tx["need_wnd_adv"], snd["eff_mss"] = need_wnd_adv, eff_mss
    return Batch(state, rbuf, tx, snd, arena)
