"""A plain-Python model of include/mtcp_gpu_rcvread.h in two parts (line numbers
of mtcp/src/api.c and mtcp/src/tcp_ring_buffer.c):

  the reference   PeekForUser (api.c:1096-1112), CopyToUser (api.c:1114-1149) and
                  RBRemove (tcp_ring_buffer.c:384-421) restated per line on an
                  App object: what tests/c/ref_rcvread_gen.c ran with the
                  reference's own ring buffer.  The puts between the reads come
                  from tests/rcvwalk_model.py (RBPut's bookkeeping) and
                  tests/rcvcopy_model.py (its byte work);
  the batch       read(): the header's contract on the record arrays in the
                  shapes mtcp_gpu_rcvread[_dev] takes: the claim (lowest request
                  index of a sid), the verdict chain, the records after, the
                  destination bytes, the result records and the totals.

Every expected value of tests/test_rcvread_model.py and tests/test_gpu_rcvread.py
comes from here, never from the kernels.
"""
import os
import struct

import numpy as np

from mtcp_amd._types import (ACK_STATE_DTYPE, ACKGEN_STATE_DTYPE, RCV_BUF_DTYPE, RCV_MAX_FRAGS, RCV_MAX_SIZE,
                             RCV_ST_ESTABLISHED, RCV_STATE_DTYPE, RCVREAD_FRAG_FREED, RCVREAD_MORE, RCVREAD_ON_ACKQ,
                             RCVREAD_PEEK, RCVREAD_REQ_DTYPE, RCVREAD_RES_DTYPE, RCVREAD_WND_ADV)
from tests import rcvcopy_model as cm
from tests import rcvwalk_model as wm

M32 = 0xFFFFFFFF
NONE, BAD_REQ, DUP, BAD_STATE, DEFER_STATE, EAGAIN, PEEKED, READ = range(8)
UNIT = 4096                                          # mtcp_gpu_rcvread_tile()
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rcvread_cases.bin")
FILL = 0xEE                                          # tests/c/ref_rcvread_gen.c fills the chunk behind RBInit


# ---- the reference ---------------------------------------------------------------------------------
class App:
    """One stream as the application's read sees it: the ring buffer (st: the
    bookkeeping, a rcvwalk_model.Stream; rb: the bytes, a rcvcopy_model.Ring)
    and the three fields of api.c:1134-1141."""

    def __init__(self, size, init_seq, eff_mss):
        self.st = wm.Stream(init_seq, size, init_seq, 0, size)
        self.rb = cm.Ring(np.full(size, FILL, dtype=np.uint8))
        self.eff_mss, self.need_wnd_adv, self.on_ackq = eff_mss, 0, 0

    def put(self, seq, payload):
        """RBPut (tcp_ring_buffer.c:280-382) and tcp_in.c:589."""
        ret, putx = wm.RBPut(self.st, len(payload), seq)
        if ret > 0:
            cm.put(self.rb, putx, payload)
        self.st.rcv_wnd = self.st.size - self.st.merged_len      # tcp_in.c:589
        return ret

    def snapshot(self):
        return (self.rb.head, self.rb.tail, self.rb.last, self.st.head_seq, self.st.merged_len, self.st.rcv_wnd,
                [tuple(f) for f in self.st.frags])


def RBRemove(app, length):
    """tcp_ring_buffer.c:384-421 with option AT_APP.  Returns (len, freed)."""
    st, rb = app.st, app.rb
    if st.merged_len < length:                       # :389-390
        length = st.merged_len
    if length == 0:                                  # :392-393
        return 0, False
    rb.head += length                                # :395-396
    st.head_seq = (st.head_seq + length) & M32       # :397
    st.merged_len -= length                          # :399
    rb.last -= length                                # :400
    freed = False
    if length == st.frags[0][1]:                     # :403-411
        del st.frags[0]
        freed = True
    elif length < st.frags[0][1]:                    # :412-415
        st.frags[0][0] = (st.frags[0][0] + length) & M32
        st.frags[0][1] -= length
    else:                                            # :416-418
        assert 0
    return length, freed


def PeekForUser(app, length):
    """api.c:1096-1112.  Returns (ret, bytes)."""
    copylen = min(app.st.merged_len, length)         # :1102 (len is positive here: both sides unsigned)
    if copylen <= 0:                                 # :1103-1106
        return -1, b""
    return copylen, app.rb.data[app.rb.head:app.rb.head + copylen].tobytes()   # :1109-1111


def CopyToUser(app, length):
    """api.c:1114-1149.  Returns (ret, bytes, freed)."""
    st = app.st
    copylen = min(st.merged_len, length)             # :1121
    if copylen <= 0:                                 # :1122-1125
        return -1, b"", False
    buf = app.rb.data[app.rb.head:app.rb.head + copylen].tobytes()   # :1129
    _, freed = RBRemove(app, copylen)                # :1130
    st.rcv_wnd = st.size - st.merged_len             # :1131
    if app.need_wnd_adv:                             # :1134
        if st.rcv_wnd > app.eff_mss:                 # :1135
            if not app.on_ackq:                      # :1136
                app.on_ackq = 1                      # :1138
                app.need_wnd_adv = 0                 # :1141
    return copylen, buf, freed


# ---- the fixture ------------------------------------------------------------------------------------
def payload_bytes(case, serial, n):
    i = np.arange(n, dtype=np.int64)
    return ((case * 113 + serial * 29 + i * 5 + (i >> 8)) & 0xFF).astype(np.uint8)


def load_fixture(path=FIXTURE):
    """The cases tests/c/ref_rcvread_gen.c wrote: dicts with family, size,
    init_seq, eff_mss and events; an event is a dict with kind ('put', 'read',
    'peek'), its fields and `after` = (head_offset, tail_offset, last_len,
    head_seq, merged_len, rcv_wnd, [(seq, len), ...])."""
    raw = open(path, "rb").read()
    pos = 0

    def u32(k=1):
        nonlocal pos
        v = struct.unpack_from(f"<{k}I", raw, pos)
        pos += 4 * k
        return v if k > 1 else v[0]

    magic, version, ncases = u32(3)
    assert magic == 0x52564352 and version == 1
    cases = []
    for _ in range(ncases):
        fam, size, init_seq, eff_mss, nev = u32(5)
        events = []
        for _ in range(nev):
            kind = u32()
            if kind == 0:
                seq, ln, ret = u32(3)
                ev = {"kind": "put", "seq": seq, "len": ln, "ret": ret - (1 << 32) if ret >> 31 else ret}
            else:
                ln, nwa, ackq, ret, nwa2, ackq2, freed = u32(7)
                ret = ret - (1 << 32) if ret >> 31 else ret
                ev = {"kind": "read" if kind == 1 else "peek", "len": ln, "need_wnd_adv": nwa, "on_ackq": ackq,
                      "ret": ret, "need_wnd_adv_after": nwa2, "on_ackq_after": ackq2, "freed": freed, "bytes": b""}
                if ret > 0:
                    ev["bytes"] = raw[pos:pos + ret]
                    pos += (ret + 3) & ~3
            snap = u32(7)
            frags = [u32(2) for _ in range(snap[6])]
            ev["after"] = (*snap[:6], frags)
            events.append(ev)
        cases.append({"family": fam, "size": size, "init_seq": init_seq, "eff_mss": eff_mss, "events": events})
    assert pos == len(raw)
    return cases


# ---- the records ------------------------------------------------------------------------------------
def records_of(app, data_off=0, tcp_state=RCV_ST_ESTABLISHED):
    """The mirrors of one App: (state, rbuf, tx, snd) records of one element each."""
    st, rb = app.st, app.rb
    state, rbuf = np.zeros(1, dtype=RCV_STATE_DTYPE), np.zeros(1, dtype=RCV_BUF_DTYPE)
    tx, snd = np.zeros(1, dtype=ACKGEN_STATE_DTYPE), np.zeros(1, dtype=ACK_STATE_DTYPE)
    state["rcv_nxt"], state["rcv_wnd"] = (st.head_seq + st.merged_len) & M32, st.rcv_wnd
    state["head_seq"], state["merged_len"], state["size"], state["tcp_state"] = st.head_seq, st.merged_len, st.size, tcp_state
    assert len(st.frags) <= RCV_MAX_FRAGS
    state["nfrag"] = len(st.frags)
    for k, (s, l) in enumerate(st.frags):
        state["frag"]["seq"][0, k], state["frag"]["len"][0, k] = s, l
    rbuf["data_off"], rbuf["size"] = data_off, st.size
    rbuf["head_offset"], rbuf["tail_offset"], rbuf["last_len"] = rb.head, rb.tail, rb.last
    tx["need_wnd_adv"], snd["eff_mss"] = app.need_wnd_adv, app.eff_mss
    return state, rbuf, tx, snd


def state_bad(s):
    """mtcp_gpu_rcvwalk.h's rule on one RCV_STATE_DTYPE record."""
    nf = int(s["nfrag"])
    return bool(s["rsvd"] != 0 or nf > RCV_MAX_FRAGS or s["size"] > RCV_MAX_SIZE or s["merged_len"] > s["size"] or
                any(int(s["frag"]["len"][k]) >= 1 << 31 for k in range(min(nf, RCV_MAX_FRAGS))))


def buf_bad(b, arena_bytes):
    """mtcp_gpu_rcvcopy.h's rule on one RCV_BUF_DTYPE record."""
    size, head, tail, last = int(b["size"]), int(b["head_offset"]), int(b["tail_offset"]), int(b["last_len"])
    return bool(b["rsvd"].any() or size == 0 or size > RCV_MAX_SIZE or int(b["data_off"]) + size > arena_bytes or
                head > tail or tail > size or last != tail - head)


def units(dst, copylen):
    """Copy units of copylen bytes to destination byte dst (mtcp_gpu_rcvread_tile())."""
    if copylen == 0:
        return 0
    nch = ((dst + copylen + 15) >> 4) - (dst >> 4)
    return (nch + UNIT // 16 - 1) // (UNIT // 16)


# ---- the batch --------------------------------------------------------------------------------------
def read(req, max_id, state, rbuf, tx, snd, arena, dst):
    """mtcp_gpu_rcvread[_dev]: state, rbuf, tx (byte 19) and dst are updated in
    place; returns (rres, total).  tx and snd may both be None."""
    assert (tx is None) == (snd is None)
    n = len(req)
    rres = np.zeros(n, dtype=RCVREAD_RES_DTYPE)
    total = np.zeros(2, dtype=np.uint64)
    arena_bytes, dst_bytes = len(arena), len(dst)
    # the claim: the lowest request index of every sid <= max_id
    first = {}
    for i in range(n):
        sid = int(req["sid"][i])
        if sid <= max_id:
            first.setdefault(sid, i)
    # every request sees the records as they were: a sid's records change under its winner only
    for i in range(n):
        r = req[i]
        sid, ln, dst_off, flags = int(r["sid"]), int(r["len"]), int(r["dst_off"]), int(r["flags"])
        rres["sid"][i] = sid
        # 1. BAD_REQ
        if sid > max_id or r["rsvd"].any() or flags & ~(RCVREAD_PEEK | RCVREAD_ON_ACKQ):
            rres["verdict"][i] = BAD_REQ
            continue
        s, b = state[sid], rbuf[sid]
        if dst_off + min(ln, int(b["size"])) > dst_bytes:
            rres["verdict"][i] = BAD_REQ
            continue
        # 2. DUP
        if first[sid] != i:
            rres["verdict"][i] = DUP
            continue
        # 3. BAD_STATE
        merged, size, nfrag = int(s["merged_len"]), int(s["size"]), int(s["nfrag"])
        copylen = min(merged, ln)                    # api.c:1102, :1121
        if (state_bad(s) or buf_bad(b, arena_bytes) or size != int(b["size"]) or merged > int(b["last_len"]) or
                (merged > 0 and (nfrag == 0 or int(s["frag"]["seq"][0]) != int(s["head_seq"]))) or
                copylen > int(s["frag"]["len"][0])):
            rres["verdict"][i] = BAD_STATE
            continue
        more = RCVREAD_MORE if merged > 0 else 0
        # 4. DEFER_STATE, 5. EAGAIN
        if int(s["tcp_state"]) != RCV_ST_ESTABLISHED or copylen == 0:
            rres["verdict"][i] = DEFER_STATE if int(s["tcp_state"]) != RCV_ST_ESTABLISHED else EAGAIN
            rres["rcv_wnd"][i], rres["flags"][i] = s["rcv_wnd"], more
            continue
        # the memcpy from rcvbuf->head (api.c:1109, :1129)
        src = int(b["data_off"]) + int(b["head_offset"])
        dst[dst_off:dst_off + copylen] = arena[src:src + copylen]
        total[0] += 1
        total[1] += copylen
        rres["copylen"][i] = copylen
        # 6. PEEKED
        if flags & RCVREAD_PEEK:
            rres["verdict"][i], rres["rcv_wnd"][i], rres["flags"][i] = PEEKED, s["rcv_wnd"], more
            continue
        # 7. READ: RBRemove, tcp_ring_buffer.c:395-415
        out = 0
        b["head_offset"] += copylen                  # :395
        s["head_seq"] = (int(s["head_seq"]) + copylen) & M32   # :397
        s["merged_len"] = merged - copylen           # :399
        b["last_len"] -= copylen                     # :400
        if copylen == int(s["frag"]["len"][0]):      # :403-411
            for k in range(nfrag - 1):
                s["frag"][k] = s["frag"][k + 1]
            s["frag"][nfrag - 1] = (0, 0)
            s["nfrag"] = nfrag - 1
            out |= RCVREAD_FRAG_FREED
        else:                                        # :412-415
            s["frag"]["seq"][0] = (int(s["frag"]["seq"][0]) + copylen) & M32
            s["frag"]["len"][0] -= copylen
        s["rcv_wnd"] = size - int(s["merged_len"])   # api.c:1131
        # api.c:1134-1145
        if (tx is not None and int(tx["need_wnd_adv"][sid]) == 1 and int(s["rcv_wnd"]) > int(snd["eff_mss"][sid]) and
                not flags & RCVREAD_ON_ACKQ):
            tx["need_wnd_adv"][sid] = 0
            out |= RCVREAD_WND_ADV
        if int(s["merged_len"]) > 0:
            out |= RCVREAD_MORE
        rres["verdict"][i], rres["rcv_wnd"][i], rres["flags"][i] = READ, s["rcv_wnd"], out
    return rres, total


def read_loop(req, max_id, state, rbuf, tx, snd, arena, dst):
    """The batch contract as a plain loop: one request after the other, each a
    batch of its own, with the sids already seen answered DUP."""
    rres = np.zeros(len(req), dtype=RCVREAD_RES_DTYPE)
    total = np.zeros(2, dtype=np.uint64)
    seen = set()
    for i in range(len(req)):
        sid = int(req["sid"][i])
        one, t = read(req[i:i + 1], max_id, state, rbuf, tx, snd, arena, dst) if sid not in seen else (None, None)
        if one is None:
            # only the tests in front of the DUP rule decide: ask them of a copy
            one, t = read(req[i:i + 1], max_id, state.copy(), rbuf.copy(), None if tx is None else tx.copy(), snd,
                          arena, dst.copy())
            if one["verdict"][0] != BAD_REQ:
                one[0] = (sid, 0, 0, DUP, 0, 0)
            t = np.zeros(2, dtype=np.uint64)
        rres[i] = one[0]
        total += t
        if sid <= max_id:
            seen.add(sid)
    return rres, total
