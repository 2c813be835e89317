"""A plain-Python model of include/mtcp_gpu_datagen.h: the send-list fold,
WriteTCPDataList's body for one stream, the head of FlushTCPSendingBuffer and
what SendTCPPacket leaves behind for data segments (line numbers: mtcp/src/),
over a grouped batch.  The loop itself is tests/txseg_model.py's (row f8), the
frames are tests/txbuild_model.py's (row f7).  No GPU, no library."""
import os
import struct

import numpy as np

from mtcp_amd._types import ACK_STATE_DTYPE, DATAGEN_RES_DTYPE, DATAGEN_STATE_DTYPE, RCV_STATE_DTYPE
from tests import ackgen_model as am
from tests import txbuild_model as xm
from tests import txseg_model as sm

(NONE, BAD, DEFERRED, IDLE, CONTROL_WAIT, NO_SNDBUF, EMPTY, BEHIND_HEAD, BAD_BURST, SENT, WINDOW,
 NO_ROOM) = range(12)
ON_LIST_BEFORE, ON_LIST_AFTER, RTO_ADD, WACK_ENQUEUED, NEED_WND_ADV = 1, 2, 4, 8, 16
ACK_FAST_RTX, ACK_SEND_LIST_REMOVE = 0x0008, 0x0020          # mtcp_gpu_ackwalk.h
ST_ESTABLISHED, MAX_DIST, M32 = 4, 1 << 30, 0xFFFFFFFF
RET = {CONTROL_WAIT: -1, NO_SNDBUF: 0, EMPTY: 0, BEHIND_HEAD: 0, WINDOW: -3, NO_ROOM: -2}


def seq_lt(a: int, b: int) -> bool:
    """TCP_SEQ_LT (tcp_in.h:37-41)."""
    return ((a - b) & M32) >= 0x80000000


def fold(on: int, flag_words) -> int:
    """tcp_in.c:453 (RemoveFromSendList, tcp_out.c:891-892), then tcp_in.c:426
    (AddtoSendList, tcp_out.c:850-851), packet by packet."""
    for w in flag_words:
        if int(w) & ACK_SEND_LIST_REMOVE:
            on = 0
        if int(w) & ACK_FAST_RTX:
            on = 1
    return on


def snd_is_bad(s) -> bool:
    """mtcp_gpu_ackwalk.h's rule."""
    return bool(s["rsvd"] or s["eff_mss"] == 0 or s["wscale_peer"] > 31 or s["sb_size"] > (1 << 30) or
                s["sb_len"] > s["sb_size"])


def dtx_is_bad(d) -> bool:
    return bool(d["rsvd"].any() or d["on_send_list"] > 1 or d["on_control_list"] > 1)


def void_burst():
    b = np.zeros((), dtype=sm.BURST_DTYPE)
    b["mss"] = 13
    return b


def status_in_front(s, st, t, d, on: int, host_tail: bool, n_links: int) -> int:
    """The status of one stream before the flush; SENT stands for "the flush runs"."""
    if dtx_is_bad(d) or am.is_bad(t, n_links) or snd_is_bad(s):
        return BAD
    if host_tail or st["tcp_state"] != ST_ESTABLISHED or s["tcp_state"] != ST_ESTABLISHED:
        return DEFERRED
    if not on:                                                # tcp_out.c:608
        return IDLE
    if d["on_control_list"]:                                  # tcp_out.c:614-617
        return CONTROL_WAIT
    if not s["has_sndbuf"]:                                   # tcp_out.c:369-373
        return NO_SNDBUF
    if s["sb_len"] == 0:                                      # tcp_out.c:377-380
        return EMPTY
    snd_nxt, head = int(s["snd_nxt"]), int(s["sb_head_seq"])
    if seq_lt(snd_nxt, head):                                 # tcp_out.c:387-394
        return BEHIND_HEAD
    base = int(d["sb_base_seq"])
    if ((snd_nxt - head) & M32) > int(s["sb_len"]) or ((snd_nxt - int(s["snd_una"])) & M32) > MAX_DIST or \
            ((snd_nxt - base) & M32) > MAX_DIST or ((head - base) & M32) > MAX_DIST:
        return BAD_BURST
    return SENT


def burst_of(s, st, t, d, cur_ts: int):
    b = np.zeros((), dtype=sm.BURST_DTYPE)
    snd_nxt = int(s["snd_nxt"])
    b["payload_off"] = (int(d["sb_off"]) + ((snd_nxt - int(d["sb_base_seq"])) & M32)) & 0xFFFFFFFFFFFFFFFF   # :404-405
    for f in ("saddr", "daddr", "sport", "dport", "link", "ip_id"):
        b[f] = t[f]
    b["seq"] = snd_nxt                                        # tcp_out.c:385
    b["ack"] = st["rcv_nxt"]                                  # tcp_out.c:289
    b["ts_val"], b["ts_ecr"] = cur_ts, st["ts_recent"]        # tcp_out.c:118-122
    b["len"] = (int(s["sb_head_seq"]) + int(s["sb_len"]) - snd_nxt) & M32      # tcp_out.c:395
    b["in_flight"] = (snd_nxt - int(s["snd_una"])) & M32      # tcp_out.c:421
    b["window"] = min(int(s["cwnd"]), int(s["peer_wnd"]))     # tcp_out.c:382
    b["peer_wnd"] = s["peer_wnd"]                             # tcp_out.c:423
    b["tcp_window"] = min(int(st["rcv_wnd"]) >> int(t["wscale_mine"]), 65535)  # tcp_out.c:301-302
    b["mss"] = s["mss"]                                       # tcp_out.c:360
    return b


def datagen(ack, ack_stop, n: int, max_id: int, idx, seg_sid, seg_start, nseg: int, seg_stop, state, snd, tx, dtx,
            cur_ts: int, payload_bytes: int, n_links: int, buf_off: int, buf_len: int, off_shift: int,
            slot_bytes: int, seg_cap: int, max_mss: int = 0):
    """mtcp_gpu_datagen[_dev]: (seg[seg_cap], desc[seg_cap], dres[m], total[2],
    snd after, tx after, dtx after, bursts[n]).  Nothing is modified."""
    snd, tx, dtx = snd.copy(), tx.copy(), dtx.copy()
    m = min(int(nseg), n) if n else 0
    bursts = np.zeros(n, dtype=sm.BURST_DTYPE)
    bursts[:] = void_burst()
    front, on_before, on_fold = [NONE] * m, [0] * m, [0] * m
    for j in range(m):
        sid = int(seg_sid[j])
        if sid > max_id:
            continue
        s, st, t, d = snd[sid], state[sid], tx[sid], dtx[sid]
        start = min(int(seg_start[j]), n)
        end = max(min(int(seg_start[j + 1]), n), start)
        host_tail = int(seg_stop[j]) < end or (ack_stop is not None and int(ack_stop[j]) < end)
        on_before[j] = on = int(d["on_send_list"]) & 1
        if ack is not None and not (dtx_is_bad(d) or am.is_bad(t, n_links) or snd_is_bad(s)):
            stop = min(max(int(ack_stop[j]), start), end)
            on = fold(on, [ack[int(q)]["flags"] for q in idx[start:stop] if int(q) < n])
        on_fold[j] = on
        front[j] = status_in_front(s, st, t, d, on, host_tail, n_links)
        if front[j] == SENT:
            bursts[j] = burst_of(s, st, t, d, cur_ts)
    seg, desc, f8, total = sm.expand(bursts, payload_bytes, n_links, buf_off, buf_len, off_shift, slot_bytes, seg_cap,
                                     max_mss)
    dres = np.zeros(m, dtype=DATAGEN_RES_DTYPE)
    for j in range(m):
        r, status = dres[j], front[j]
        r["first_seg"] = f8[j]["first_seg"]
        r["status"] = status
        if status <= BAD:
            continue
        sid = int(seg_sid[j])
        s, st, t, d = snd[sid], state[sid], tx[sid], dtx[sid]
        on, flags, ret = on_fold[j], 0, None
        if status == SENT:
            if f8[j]["status"]:
                status = BAD_BURST
            else:
                e, nbytes, stop = int(f8[j]["n_seg"]), int(f8[j]["bytes"]), int(f8[j]["stop"])
                status = NO_ROOM if stop & sm.STOP_NO_ROOM else WINDOW if stop & sm.STOP_WINDOW else SENT
                ret = e if status == SENT else RET[status]    # tcp_out.c:443, :433, :439-441
                r["n_seg"], r["bytes"], r["stop"] = e, nbytes, stop
                s["snd_nxt"] = (int(s["snd_nxt"]) + nbytes) & M32              # tcp_out.c:332
                tl = int(t["ts_lastack_sent"])
                if e:
                    s["ts_rto"] = (cur_ts + int(s["rto"])) & M32               # tcp_out.c:346
                    if not s["on_rto"]:                                        # timer.c:37
                        flags |= RTO_ADD
                    s["on_rto"] = 1
                    t["ip_id"] = (int(t["ip_id"]) + e) & 0xFFFF                # ip_out.c:139
                    t["ts_lastack_sent"] = tl = cur_ts                         # tcp_out.c:290
                    if int(st["rcv_wnd"]) >> int(t["wscale_mine"]) == 0:       # tcp_out.c:304-306
                        t["need_wnd_adv"] = 1
                        flags |= NEED_WND_ADV
                if status == WINDOW and stop & sm.STOP_PEER_WINDOW:            # tcp_out.c:423
                    if ((((cur_ts - tl) & M32) * 1000) & M32) // 1000 > 500:   # tcp_out.c:429, tcp_in.h:44-50
                        t["is_wack"] = 1                                       # tcp_out.c:430, :931-933
                        flags |= WACK_ENQUEUED
        elif status in RET:
            ret = RET[status]
        if ret is not None and ret >= 0:
            on = 0                                                             # tcp_out.c:639
            if t["ack_cnt"] > 0:                                               # tcp_out.c:643-650
                t["ack_cnt"] = int(t["ack_cnt"]) - ret if int(t["ack_cnt"]) > ret else 0
        d["on_send_list"] = on
        r["status"] = status
        r["flags"] = flags | (ON_LIST_BEFORE if on_before[j] else 0) | (ON_LIST_AFTER if on else 0)
    return seg, desc, dres, total, snd, tx, dtx, bursts


# ---- the reference fixture --------------------------------------------------------
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "datagen_cases.bin")
FAMILIES = ("fits the window", "the window stops", "the 500 ms test", "where snd_nxt is", "after a fast retransmit",
            "nothing to flush", "the slot budget", "the piggy-back decrement", "the wraps", "a zero advertised window",
            "not on the send list", "lists")
SLOT, NOT_SERVED = 1600, 0x7FFFFFFF
SND_WORDS = ("snd_nxt", "snd_una", "peer_wnd", "cwnd", "rto", "ts_rto", "sb_head_seq", "sb_len")


def _record(raw: bytes) -> dict:
    t = np.frombuffer(raw[:32], dtype=am.STATE_DTYPE)[0]
    assert not t["rsvd"].any()
    s = {f: int(t[f]) for f in am.STATE_DTYPE.names if f != "rsvd"}
    s.update(zip(SND_WORDS, struct.unpack("<8I", raw[32:64])))
    s.update(zip(("mss", "on_rto", "has_sndbuf", "on_send_list", "on_control_list"), struct.unpack("<HBBBB", raw[64:70])))
    s.update(zip(("rcv_nxt", "rcv_wnd", "ts_recent", "arena_off"), struct.unpack("<4I", raw[72:88])))
    return s


def load_fixture(path: str = FIXTURE) -> list:
    """The cases tests/c/ref_datagen_gen.c wrote: dicts with cur_ts, budget,
    family and streams; a stream has before, after (records as dicts), data
    (the send buffer's bytes), ret, rto_added, wack_enqueued, frames."""
    raw = open(path, "rb").read()
    magic, version, cases, _ = struct.unpack("<4I", raw[:16])
    assert magic == 0x4E454744 and version == 1
    out, at = [], 16
    for _ in range(cases):
        cur_ts, budget, fam, ns = struct.unpack("<IHBB", raw[at:at + 8])
        at += 8
        streams = []
        for _ in range(ns):
            before = _record(raw[at:at + 88])
            nb, = struct.unpack("<I", raw[at + 88:at + 92])
            at += 92
            streams.append(dict(before=before, data=np.frombuffer(raw, np.uint8, nb, at)))
            at += (nb + 3) & ~3
        for s in streams:
            ret, nf, rto_added, wack = struct.unpack("<iHBB", raw[at:at + 8])
            s.update(ret=ret, rto_added=rto_added, wack_enqueued=wack, after=_record(raw[at + 8:at + 96]), frames=[])
            at += 96
            for _ in range(nf):
                ln, = struct.unpack("<H", raw[at:at + 2])
                s["frames"].append(np.frombuffer(raw, np.uint8, ln, at + 4))
                at += 4 + ((ln + 3) & ~3)
        out.append(dict(cur_ts=cur_ts, budget=budget, family=fam, streams=streams))
    assert at == len(raw)
    return out


def case_batch(c):
    """One fixture case as the call's arguments: stream i has id i and one
    packet (no ACK records: the fold is the identity), the payload arena holds
    each send buffer at its arena_off, the slot budget is the frame buffer's
    length in fixed slots."""
    ns = len(c["streams"])
    snd = np.zeros(ns, dtype=ACK_STATE_DTYPE)
    state = np.zeros(ns, dtype=RCV_STATE_DTYPE)
    tx = np.zeros(ns, dtype=am.STATE_DTYPE)
    dtx = np.zeros(ns, dtype=DATAGEN_STATE_DTYPE)
    end = max(s["before"]["arena_off"] + len(s["data"]) for s in c["streams"]) + 3
    payload = np.full(end, 0xC3, np.uint8)
    for i, s in enumerate(c["streams"]):
        b = s["before"]
        for f in am.STATE_DTYPE.names:
            if f != "rsvd":
                tx[i][f] = b[f]
        for f in SND_WORDS + ("mss", "on_rto", "has_sndbuf"):
            snd[i][f] = b[f]
        snd[i]["eff_mss"], snd[i]["sb_size"], snd[i]["tcp_state"] = b["mss"] - 12, 8192, ST_ESTABLISHED
        state[i]["rcv_nxt"], state[i]["rcv_wnd"], state[i]["ts_recent"] = b["rcv_nxt"], b["rcv_wnd"], b["ts_recent"]
        state[i]["tcp_state"] = ST_ESTABLISHED
        dtx[i]["sb_off"], dtx[i]["sb_base_seq"] = b["arena_off"], b["sb_head_seq"]
        dtx[i]["on_send_list"], dtx[i]["on_control_list"] = b["on_send_list"], b["on_control_list"]
        payload[b["arena_off"]:b["arena_off"] + len(s["data"])] = s["data"]
    idx = np.arange(ns, dtype=np.uint32)
    return dict(n=ns, max_id=ns - 1, idx=idx, seg_sid=idx.copy(), seg_start=np.arange(ns + 1, dtype=np.uint32),
                seg_stop=np.arange(1, ns + 1, dtype=np.uint32), state=state, snd=snd, tx=tx, dtx=dtx,
                cur_ts=c["cur_ts"], payload=payload, n_links=3, buf_off=0, buf_len=c["budget"] * SLOT, off_shift=0,
                slot_bytes=SLOT, seg_cap=97)


def run_batch(b, ack=None, ack_stop=None, nseg=None):
    return datagen(ack, ack_stop, b["n"], b["max_id"], b["idx"], b["seg_sid"], b["seg_start"],
                   len(b["seg_sid"]) if nseg is None else nseg, b["seg_stop"], b["state"], b["snd"], b["tx"], b["dtx"],
                   b["cur_ts"], len(b["payload"]), b["n_links"], b["buf_off"], b["buf_len"], b["off_shift"],
                   b["slot_bytes"], b["seg_cap"], b.get("max_mss", 0))


def after_of(i: int, snd, tx, dtx, before: dict) -> dict:
    """Stream i of a case_batch after the call, in the fixture's fields."""
    a = dict(before)
    for f in am.STATE_DTYPE.names:
        if f != "rsvd":
            a[f] = int(tx[i][f])
    for f in SND_WORDS + ("mss", "on_rto", "has_sndbuf"):
        a[f] = int(snd[i][f])
    a["on_send_list"], a["on_control_list"] = int(dtx[i]["on_send_list"]), int(dtx[i]["on_control_list"])
    return a
