"""A plain-Python model of include/mtcp_gpu_sndwrite.h in two parts (line numbers
of mtcp/src/api.c and mtcp/src/tcp_send_buffer.c):

  the reference   SBPut (tcp_send_buffer.c:116-146), SBRemove (:149-173),
                  CopyFromUser (api.c:1416-1456) and the lines of mtcp_write
                  around it (api.c:1495-1563) restated per line on byte arrays:
                  what tests/c/ref_sndwrite_gen.c ran with the reference's own
                  send buffer;
  the batch       write(): the header's contract on the record arrays in the
                  shapes mtcp_gpu_sndwrite[_dev] takes: the claim (lowest
                  request index of a sid), the verdict chain, the anchored d_dtx,
                  the records after, the chunk bytes, the result records, the
                  table and the totals.

Every expected value of tests/test_sndwrite_model.py and
tests/test_gpu_sndwrite.py comes from here, never from the kernels.
"""
import os
import struct

import numpy as np

from mtcp_amd._types import (ACK_STATE_DTYPE, DATAGEN_STATE_DTYPE, FLOW_NONE, SNDWRITE_COMPACTED, SNDWRITE_RES_DTYPE,
                             SNDWRITE_ROOM, SNDWRITE_SEND_LIST_ADD)
from tests import datagen_model as dm

M32 = 0xFFFFFFFF
NONE, BAD_REQ, DUP, BAD_STATE, DEFER_STATE, ZERO, EAGAIN, NO_SNDBUF, FULL, WRITTEN = range(10)
UNIT = 4096                                          # mtcp_gpu_sndwrite_tile()
ST_ESTABLISHED = 4
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sndwrite_cases.bin")
FILL = 0xEE                                          # tests/c/ref_sndwrite_gen.c fills the chunk behind SBInit


def to_int(v):
    """(int) of a uint32_t."""
    return v - (1 << 32) if v >> 31 else v


# ---- the reference ---------------------------------------------------------------------------------
class SendBuf:
    """struct tcp_send_buffer behind SBInit (tcp_send_buffer.c:59-88); head is data + head_off."""

    def __init__(self, size, init_seq, fill=FILL):
        self.data = np.full(size, fill, dtype=np.uint8)
        self.head_off = self.tail_off = 0            # :82
        self.len = self.cum_len = 0                  # :83
        self.size = size                             # :84
        self.head_seq = init_seq                     # :86

    def snapshot(self):
        return self.head_off, self.tail_off, self.len, self.cum_len, self.head_seq


def SBPut(buf, data, length):
    """tcp_send_buffer.c:116-146.  Returns (ret, compacted)."""
    if length <= 0:                                  # :121-122
        return 0, False
    to_put = min(length, buf.size - buf.len)         # :125
    if to_put <= 0:                                  # :126-128
        return -2, False
    compacted = False
    if buf.tail_off + to_put < buf.size:             # :130
        buf.data[buf.tail_off:buf.tail_off + to_put] = data[:to_put]          # :132
        buf.tail_off += to_put                       # :133
    else:
        buf.data[:buf.len] = buf.data[buf.head_off:buf.head_off + buf.len].copy()   # :136 memmove
        buf.head_off = 0                             # :137-138
        buf.data[buf.len:buf.len + to_put] = data[:to_put]                    # :139
        buf.tail_off = buf.len + to_put              # :140
        compacted = True
    buf.len += to_put                                # :142
    buf.cum_len += to_put                            # :143
    return to_put, compacted


def SBRemove(buf, length):
    """tcp_send_buffer.c:149-173."""
    if length <= 0:                                  # :153-154
        return 0
    to_remove = min(length, buf.len)                 # :156
    if to_remove <= 0:                               # :157-159
        return -2
    buf.head_off += to_remove                        # :161-162
    buf.head_seq = (buf.head_seq + to_remove) & M32  # :163
    buf.len -= to_remove                             # :164
    if buf.len == 0 and buf.head_off > 0:            # :167-170
        buf.head_off = buf.tail_off = 0
    return to_remove


class Stream:
    """The fields of tcp_stream and tcp_send_vars mtcp_write touches."""

    def __init__(self, sndbuf, snd_wnd, state=ST_ESTABLISHED, on_send_list=0):
        self.sndbuf, self.snd_wnd, self.state = sndbuf, snd_wnd, state
        self.on_sendq, self.on_send_list = 0, on_send_list


def CopyFromUser(stream, data, length):
    """api.c:1416-1456 with a buffer present.  Returns (ret, compacted); -1 is EAGAIN."""
    sndlen = min(to_int(stream.snd_wnd), length)     # :1423
    if sndlen <= 0:                                  # :1424-1427
        return -1, False
    assert stream.sndbuf is not None                 # :1430-1438 stays with the host
    ret, compacted = SBPut(stream.sndbuf, data, sndlen)        # :1440
    stream.snd_wnd = stream.sndbuf.size - stream.sndbuf.len    # :1442
    if ret <= 0:                                     # :1443-1448
        return -1, False
    return ret, compacted


def mtcp_write(stream, data, length):
    """api.c:1495-1563 for an ESTABLISHED stream and len > 0, the sendq drained
    at once (core.c:479-483).  Returns (ret, compacted, send_list_add, write_event)."""
    ret, compacted = CopyFromUser(stream, data, length)        # :1526
    added = False
    if ret > 0 and not (stream.on_sendq or stream.on_send_list):   # :1535
        stream.on_send_list = 1                      # :1536-1540, core.c:479-483, tcp_out.c:850-851
        added = True
    return ret, compacted, added, stream.snd_wnd > 0             # :1549


# ---- the fixture ------------------------------------------------------------------------------------
def payload_bytes(case, serial, n):
    i = np.arange(n, dtype=np.int64)
    return ((case * 113 + serial * 29 + i * 5 + (i >> 8)) & 0xFF).astype(np.uint8)


def load_fixture(path=FIXTURE):
    """The cases tests/c/ref_sndwrite_gen.c wrote: dicts with family, size,
    init_seq and ops; an op is a dict with kind ('put', 'rem'), len, ret, `after`
    = (head_off, tail_off, len, cum_len, head_seq) and data (the whole chunk)."""
    raw = open(path, "rb").read()
    pos = 0

    def u32(k=1):
        nonlocal pos
        v = struct.unpack_from(f"<{k}I", raw, pos)
        pos += 4 * k
        return v if k > 1 else v[0]

    magic, version, ncases = u32(3)
    assert magic == 0x57444E53 and version == 1
    cases = []
    for _ in range(ncases):
        fam, size, init_seq, nops = u32(4)
        ops = []
        for _ in range(nops):
            kind, ln, ret, head_off, tail_off, blen, cum_lo, cum_hi, head_seq = u32(9)
            data = np.frombuffer(raw, dtype=np.uint8, count=size, offset=pos)
            pos += size
            ops.append({"kind": "put" if kind == 0 else "rem", "len": ln, "ret": to_int(ret),
                        "after": (head_off, tail_off, blen, cum_lo | cum_hi << 32, head_seq), "data": data})
        cases.append({"family": fam, "size": size, "init_seq": init_seq, "ops": ops})
    assert pos == len(raw)
    return cases


# ---- the records ------------------------------------------------------------------------------------
def records_of(buf, sb_off, snd_wnd=None, on_send_list=0, tcp_state=ST_ESTABLISHED, stale_base=None):
    """The mirrors of one SendBuf whose chunk lies at sb_off of the arena: (snd,
    dtx) of one element each, d_dtx anchored (sb_base_seq = head_seq - head_off).
    stale_base: another sb_base_seq for an empty buffer."""
    snd, dtx = np.zeros(1, dtype=ACK_STATE_DTYPE), np.zeros(1, dtype=DATAGEN_STATE_DTYPE)
    snd["snd_wnd"] = buf.size - buf.len if snd_wnd is None else snd_wnd
    snd["sb_head_seq"], snd["sb_len"], snd["sb_size"] = buf.head_seq, buf.len, buf.size
    snd["snd_una"] = snd["snd_nxt"] = buf.head_seq
    snd["mss"], snd["eff_mss"], snd["tcp_state"], snd["has_sndbuf"] = 1460, 1448, tcp_state, 1
    dtx["sb_off"], dtx["on_send_list"] = sb_off, on_send_list
    dtx["sb_base_seq"] = (buf.head_seq - buf.head_off) & M32 if stale_base is None else stale_base
    return snd, dtx


def offsets_of(s, d):
    """(head_off, tail_off) of an anchored pair: the header's rule."""
    head_off = 0 if int(s["sb_len"]) == 0 else (int(s["sb_head_seq"]) - int(d["sb_base_seq"])) & M32
    return head_off, head_off + int(s["sb_len"])


def units(dst, length):
    """Copy units of length bytes to destination byte dst (mtcp_gpu_sndwrite_tile())."""
    if length == 0:
        return 0
    nch = ((dst + length + 15) >> 4) - (dst >> 4)
    return (nch + UNIT // 16 - 1) // (UNIT // 16)


# ---- the batch --------------------------------------------------------------------------------------
def write(wreq, max_id, snd, dtx, src, payload, src_bytes=None):
    """mtcp_gpu_sndwrite[_dev]: snd, dtx and payload are updated in place;
    returns (wres, seg_sid, seg_start, seg_stop, nseg, total)."""
    n = len(wreq)
    wres = np.zeros(n, dtype=SNDWRITE_RES_DTYPE)
    total = np.zeros(2, dtype=np.uint64)
    seg_sid = np.full(n, FLOW_NONE, dtype=np.uint32)
    seg_start, seg_stop = np.zeros(n + 1, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    nseg = np.array([n], dtype=np.uint32)
    src_bytes = len(src) if src_bytes is None else src_bytes
    pbytes = len(payload)
    # the claim: the lowest request index of every sid <= max_id
    first = {}
    for i in range(n):
        sid = int(wreq["sid"][i])
        if sid <= max_id:
            first.setdefault(sid, i)
    moves, copies = [], []
    for i in range(n):
        r = wreq[i]
        sid, ln, src_off = int(r["sid"]), int(r["len"]), int(r["src_off"])
        wres["sid"][i] = sid
        # 1. BAD_REQ
        if sid > max_id or r["flags"] or r["rsvd"].any() or ln > 0x7FFFFFFF or src_off + ln > src_bytes:
            wres["verdict"][i] = BAD_REQ
            continue
        # 2. DUP
        if first[sid] != i:
            wres["verdict"][i] = DUP
            continue
        # 3. BAD_STATE
        s, d = snd[sid], dtx[sid]
        sb_len, sb_size, sb_off = int(s["sb_len"]), int(s["sb_size"]), int(d["sb_off"])
        head_off, tail_off = offsets_of(s, d)
        if dm.snd_is_bad(s) or dm.dtx_is_bad(d) or (s["has_sndbuf"] and (
                sb_size == 0 or sb_off + sb_size > pbytes or head_off > sb_size - sb_len)):
            wres["verdict"][i] = BAD_STATE
            continue
        wnd = int(s["snd_wnd"])

        def done(verdict, wnd, flags=0, written=0):
            wres["verdict"][i], wres["snd_wnd"][i], wres["written"][i] = verdict, wnd, written
            wres["flags"][i] = flags | (SNDWRITE_ROOM if wnd > 0 else 0)
        # 4. DEFER_STATE (api.c:1495-1501), 5. ZERO (:1503-1510)
        if int(s["tcp_state"]) != ST_ESTABLISHED:
            done(DEFER_STATE, wnd)
            continue
        if ln == 0:
            done(ZERO, wnd)
            continue
        # 6. EAGAIN: api.c:1423-1427
        sndlen = min(to_int(wnd), ln)
        if sndlen <= 0:
            done(EAGAIN, wnd)
            continue
        # 7. NO_SNDBUF: api.c:1430
        if not s["has_sndbuf"]:
            done(NO_SNDBUF, wnd)
            continue
        # 8. FULL: tcp_send_buffer.c:125-128, api.c:1442
        to_put = min(sndlen, sb_size - sb_len)
        if to_put == 0:
            s["snd_wnd"] = sb_size - sb_len
            done(FULL, sb_size - sb_len)
            continue
        # 9. WRITTEN
        flags = 0
        if tail_off + to_put < sb_size:              # :130-133
            dst = sb_off + tail_off
            if sb_len == 0:
                d["sb_base_seq"] = s["sb_head_seq"]
        else:                                        # :134-141
            if head_off and sb_len:
                moves.append((sb_off, sb_off + head_off, sb_len))
            dst = sb_off + sb_len
            d["sb_base_seq"] = s["sb_head_seq"]
            flags |= SNDWRITE_COMPACTED
        copies.append((dst, src_off, to_put))
        s["sb_len"] = sb_len + to_put                # :142
        s["snd_wnd"] = sb_size - sb_len - to_put     # api.c:1442
        if not d["on_send_list"]:
            flags |= SNDWRITE_SEND_LIST_ADD          # api.c:1535-1541
        d["on_send_list"] = 1
        seg_sid[i] = sid
        total[0] += 1
        total[1] += to_put
        done(WRITTEN, int(s["snd_wnd"]), flags, to_put)
    # every memmove of the batch before any memcpy (disjoint chunks: any order among themselves)
    for to, frm, ln in moves:
        payload[to:to + ln] = payload[frm:frm + ln].copy()
    for dst, src_off, ln in copies:
        payload[dst:dst + ln] = src[src_off:src_off + ln]
    return wres, seg_sid, seg_start, seg_stop, nseg, total


def write_loop(wreq, max_id, snd, dtx, src, payload):
    """The batch contract as a plain loop: one request after the other, each a
    batch of its own, with the sids already seen answered DUP."""
    n = len(wreq)
    wres = np.zeros(n, dtype=SNDWRITE_RES_DTYPE)
    seg_sid = np.full(n, FLOW_NONE, dtype=np.uint32)
    total = np.zeros(2, dtype=np.uint64)
    seen = set()
    for i in range(n):
        sid = int(wreq["sid"][i])
        if sid in seen:
            # only the tests in front of the DUP rule decide: ask them of copies
            one = write(wreq[i:i + 1], max_id, snd.copy(), dtx.copy(), src, payload.copy())[0]
            if one["verdict"][0] != BAD_REQ:
                one[0] = (sid, 0, 0, DUP, 0, 0)
            wres[i] = one[0]
        else:
            one, sids, _, _, _, t = write(wreq[i:i + 1], max_id, snd, dtx, src, payload)
            wres[i], seg_sid[i] = one[0], sids[0]
            total += t
        if sid <= max_id:
            seen.add(sid)
    return wres, seg_sid, total
