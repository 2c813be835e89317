"""A plain-Python model of include/mtcp_gpu_ackgen.h: EnqueueACK's count,
WriteTCPACKList for one stream and SendTCPPacket for a pure ACK, one statement
per reference line (line numbers: mtcp/src/), then the grouped-batch form on
top of it (the fold over d_place flags, the stop arrays, DEFERRED, BAD, the
room rule, void records, totals).

The per-case form works on a dict `s` with the reference's fields:
    saddr daddr sport dport ip_id ack_cnt is_wack wscale_mine link has_rcvbuf
    need_wnd_adv ts_lastack_sent on_ack_list snd_nxt rcv_nxt rcv_wnd head_seq
    merged_len ts_recent
No GPU, no library."""
import os
import struct

import numpy as np

from tests import txbuild_model as xm

SEG_DTYPE, DESC_DTYPE = xm.SEG_DTYPE, xm.DESC_DTYPE
STATE_DTYPE = np.dtype([("saddr", "<u4"), ("daddr", "<u4"), ("sport", "<u2"), ("dport", "<u2"), ("ip_id", "<u2"),
                        ("ack_cnt", "u1"), ("is_wack", "u1"), ("wscale_mine", "u1"), ("link", "u1"),
                        ("has_rcvbuf", "u1"), ("need_wnd_adv", "u1"), ("ts_lastack_sent", "<u4"),
                        ("rsvd", "u1", (8,))])
RES_DTYPE = np.dtype([("first_seg", "<u4"), ("n_ack", "u1"), ("wack", "u1"), ("status", "u1"), ("flags", "u1"),
                      ("ack", "<u4"), ("window", "<u2"), ("rsvd", "<u2")])
NONE, BAD, DEFERRED, IDLE, NOT_TO_ACK, SENT, NO_ROOM = range(7)
ON_LIST, NEED_WND_ADV = 0x1, 0x2
ACK_OPT_NOW, ACK_OPT_AGGREGATE, ACK_OPT_WACK = 0, 1, 2       # tcp_out.h:9-14
RCV_ACK_NOW, RCV_ACK_AGGREGATE = 0x02, 0x04                  # mtcp_gpu_rcvwalk.h
PUT_VERDICTS = (13, 14, 15)                                  # PUT_DROPPED, PUT_NO_ROOM, PUT_STORED
ST_ESTABLISHED = 4
FRAME_LEN, VOID_FORM = 66, 0xFF
TCP_FLAG_ACK, TCP_FLAG_WACK = 0x10, 0x80
M32 = 0xFFFFFFFF


def seq_leq(a: int, b: int) -> bool:
    """TCP_SEQ_LEQ (tcp_in.h:37-41)."""
    d = (a - b) & M32
    return d == 0 or d >= 0x80000000


# ---- the per-case form ----------------------------------------------------------
def enqueue_ack(s: dict, opt: int) -> None:
    """EnqueueACK (tcp_out.c:911-935)."""
    if opt == ACK_OPT_NOW:                                   # :923
        if s["ack_cnt"] < s["ack_cnt"] + 1:                  # :924, in int: always
            s["ack_cnt"] = (s["ack_cnt"] + 1) & 63           # :925, a 6-bit field (tcp_stream.h:117)
    elif opt == ACK_OPT_AGGREGATE:                           # :927
        if s["ack_cnt"] == 0:                                # :928
            s["ack_cnt"] = 1                                 # :929
    elif opt == ACK_OPT_WACK:                                # :931
        s["is_wack"] = 1                                     # :932
    s["on_ack_list"] = 1                                     # :934 AddtoACKList


def send_ack(s: dict, cur_ts: int, flags: int, room: bool):
    """SendTCPPacket(mtcp, s, cur_ts, flags, NULL, 0) (tcp_out.c:220-354) with
    IPOutput's ip_id (ip_out.c:139): the record of the frame, or None where no
    slot could be had (-2, tcp_out.c:238-240: nothing has changed by then)."""
    if not room:
        return None
    r = np.zeros((), dtype=SEG_DTYPE)
    r["saddr"], r["daddr"] = s["saddr"], s["daddr"]          # ip_out.c:143-144
    r["ip_id"] = s["ip_id"]                                  # ip_out.c:139
    s["ip_id"] = (s["ip_id"] + 1) & 0xFFFF
    r["sport"], r["dport"] = s["sport"], s["dport"]          # :243-244
    if flags & TCP_FLAG_WACK:                                # :265
        r["seq"] = (s["snd_nxt"] - 1) & M32                  # :266
    else:
        r["seq"] = s["snd_nxt"]                              # :284
    r["ack"] = s["rcv_nxt"]                                  # :289
    s["ts_lastack_sent"] = cur_ts                            # :290
    window32 = s["rcv_wnd"] >> s["wscale_mine"]              # :298-301
    r["window"] = min(window32, 65535)                       # :302
    if window32 == 0:                                        # :304
        s["need_wnd_adv"] = 1                                # :305
    r["ts_val"], r["ts_ecr"] = cur_ts, s["ts_recent"]        # :118-122
    r["flags"], r["form"], r["link"] = flags & 0x1F, 1, s["link"]
    return r                                                 # payloadlen 0: :332-351 change nothing


def write_ack_list(s: dict, cur_ts: int, budget: int) -> list:
    """WriteTCPACKList's body for one stream on the list (tcp_out.c:697-761)
    with a slot source that runs dry after `budget` frames: the records."""
    out = []
    if not s["on_ack_list"]:                                 # :697
        return out
    to_ack = False                                           # :700
    if s["has_rcvbuf"]:                                      # :708 (the state is ESTABLISHED, :701)
        if seq_leq(s["rcv_nxt"], (s["head_seq"] + s["merged_len"]) & M32):   # :709-711
            to_ack = True                                    # :712
    if to_ack:                                               # :727
        while s["ack_cnt"] > 0:                              # :729
            r = send_ack(s, cur_ts, TCP_FLAG_ACK, len(out) < budget)         # :730
            if r is None:                                    # :732
                break                                        # :734
            out.append(r)
            s["ack_cnt"] -= 1                                # :736
        if s["is_wack"]:                                     # :740
            s["is_wack"] = 0                                 # :741
            r = send_ack(s, cur_ts, TCP_FLAG_ACK | TCP_FLAG_WACK, len(out) < budget)   # :742
            if r is None:                                    # :744
                s["is_wack"] = 1                             # :746
            else:
                out.append(r)
        if not (s["ack_cnt"] or s["is_wack"]):               # :750
            s["on_ack_list"] = 0                             # :751
    else:
        s["on_ack_list"] = 0                                 # :756
        s["ack_cnt"] = 0                                     # :757
        s["is_wack"] = 0                                     # :758
    return out


def run_case(before: dict, opts, cur_ts: int, budget: int):
    """One fixture case: the EnqueueACK calls, then WriteTCPACKList.
    (records, the stream after)."""
    s = dict(before)
    for o in opts:
        enqueue_ack(s, int(o))
    return write_ack_list(s, cur_ts, budget), s


# ---- the grouped-batch form -------------------------------------------------------
def slot_of(off_shift: int, slot_bytes: int) -> int:
    a = max(2, 1 << off_shift)
    return slot_bytes or (FRAME_LEN + a - 1) // a * a


def room_of(buf_off: int, buf_len: int, off_shift: int, slot: int, seg_cap: int) -> int:
    """mtcp_gpu_txseg.h's room rule for 66 B frames in slots of one size, record
    by record: record k is emitted iff k < seg_cap, its frame ends at or before
    buf_len and its descriptor offset fits 32 bits; the first k that fails ends
    it (the emitted records are a prefix)."""
    k = 0
    while k < seg_cap:
        at = buf_off + k * slot
        if at + FRAME_LEN > buf_len or (at >> off_shift) > M32:
            break
        k += 1
    return k


def is_bad(t, n_links: int) -> bool:
    return bool(t["rsvd"].any() or t["ack_cnt"] > 63 or t["is_wack"] > 1 or t["has_rcvbuf"] > 1 or
                t["need_wnd_adv"] > 1 or t["wscale_mine"] > 31 or t["link"] >= n_links)


def void_records(n: int):
    seg = np.zeros(n, dtype=SEG_DTYPE)
    seg["form"] = VOID_FORM
    return seg


def ackgen(place, n: int, max_id: int, idx, seg_sid, seg_start, nseg: int, seg_stop, ack_stop, state, snd,
           cur_ts: int, tx, n_links: int, buf_off: int, buf_len: int, off_shift: int, slot_bytes: int, seg_cap: int):
    """mtcp_gpu_ackgen[_dev]: (seg[seg_cap], desc[seg_cap], ares[m], total[2],
    tx after).  The arrays may be longer than the call reads; nothing is
    modified."""
    tx = tx.copy()
    m = min(int(nseg), n) if n else 0
    slot = slot_of(off_shift, slot_bytes)
    E = room_of(buf_off, buf_len, off_shift, slot, seg_cap)
    ares = np.zeros(m, dtype=RES_DTYPE)
    recs = []
    planned_before = 0                      # the records planned by the segments in front (saturating at seg_cap)
    firsts = []
    for j in range(m):
        firsts.append(planned_before)
        sid = int(seg_sid[j])
        if sid > max_id:
            continue                                         # NONE
        t = tx[sid]
        if is_bad(t, n_links):
            ares[j]["status"] = BAD
            continue
        start = min(int(seg_start[j]), n)
        end = max(min(int(seg_start[j + 1]), n), start)
        ss = int(seg_stop[j])
        st = state[sid]
        deferred = ss < end or (ack_stop is not None and int(ack_stop[j]) < end) or st["tcp_state"] != ST_ESTABLISHED
        s = {f: int(t[f]) for f in STATE_DTYPE.names if f != "rsvd"}
        s["on_ack_list"] = 1 if (s["ack_cnt"] or s["is_wack"]) else 0
        s["snd_nxt"] = int(snd[sid]["snd_nxt"])
        for f in ("rcv_nxt", "rcv_wnd", "head_seq", "merged_len", "ts_recent"):
            s[f] = int(st[f])
        for p in range(start, min(max(ss, start), end)):
            q = int(idx[p])
            if q >= n:
                continue
            fl, v = int(place[q]["flags"]), int(place[q]["verdict"])
            if fl & RCV_ACK_NOW:
                enqueue_ack(s, ACK_OPT_NOW)
            if fl & RCV_ACK_AGGREGATE:
                enqueue_ack(s, ACK_OPT_AGGREGATE)
            if v in PUT_VERDICTS:
                s["has_rcvbuf"] = 1                          # tcp_in.c:555-566
        r = ares[j]
        r["ack"] = s["rcv_nxt"]
        r["window"] = min(s["rcv_wnd"] >> s["wscale_mine"], 65535)
        r["flags"] = ON_LIST if s["on_ack_list"] else 0
        if deferred:
            r["status"] = DEFERRED
            out = []
        elif not s["on_ack_list"]:
            r["status"] = IDLE
            out = []
        else:
            nwa = s["need_wnd_adv"]
            c0, w0 = s["ack_cnt"], s["is_wack"]
            budget = max(E - planned_before, 0)
            # what the stream would send with every slot it asks for: the plan
            planned = len(write_ack_list(dict(s), cur_ts, 1 << 30))
            to_ack = s["has_rcvbuf"] and seq_leq(s["rcv_nxt"], (s["head_seq"] + s["merged_len"]) & M32)
            out = write_ack_list(s, cur_ts, budget)
            if not to_ack:
                r["status"] = NOT_TO_ACK
            else:
                r["status"] = SENT if len(out) == planned else NO_ROOM
            r["n_ack"] = min(len(out), c0)
            r["wack"] = 1 if len(out) > c0 else 0
            assert not r["wack"] or w0
            if out and (s["rcv_wnd"] >> s["wscale_mine"]) == 0:      # tcp_out.c:304-306 ran
                assert s["need_wnd_adv"] == 1
                r["flags"] |= NEED_WND_ADV
            else:
                assert s["need_wnd_adv"] == nwa
            planned_before = min(planned_before + planned, seg_cap)
        for f in ("ip_id", "ack_cnt", "is_wack", "has_rcvbuf", "need_wnd_adv", "ts_lastack_sent"):
            tx[sid][f] = s[f]
        recs.extend(out)
    T = len(recs)
    assert T == min(planned_before, E)
    seg, desc = void_records(seg_cap), np.zeros(seg_cap, dtype=DESC_DTYPE)
    for k, r in enumerate(recs):
        seg[k] = r
        desc[k]["offset"], desc[k]["len"] = (buf_off + k * slot) >> off_shift, FRAME_LEN
    for j in range(m):
        ares[j]["first_seg"] = min(firsts[j], T)
    total = np.array([T, T * slot], dtype=np.uint64)
    return seg, desc, ares, total, tx


# ---- the reference fixture --------------------------------------------------------
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ackgen_cases.bin")
FAMILIES = ("AGGREGATE only", "k NOWs", "mixed, a count on entry", "is_wack", "rcvbuf == NULL",
            "rcv_nxt past head_seq + merged_len", "the slot budget", "the window", "ip_id near the wrap")
WALK_FIELDS = ("snd_nxt", "rcv_nxt", "rcv_wnd", "head_seq", "merged_len", "ts_recent")


def _stream(raw: bytes) -> dict:
    t = np.frombuffer(raw[:32], dtype=STATE_DTYPE)[0]
    assert not t["rsvd"].any()
    s = {f: int(t[f]) for f in STATE_DTYPE.names if f != "rsvd"}
    s.update(zip(WALK_FIELDS, struct.unpack("<6I", raw[32:56])))
    return s


def load_fixture(path: str = FIXTURE) -> list:
    """The cases tests/c/ref_ackgen_gen.c wrote: dicts with before, after (the
    per-case form's streams), opts, cur_ts, budget, family, frames (k x 66 u8)."""
    raw = open(path, "rb").read()
    magic, version, cases, _ = struct.unpack("<4I", raw[:16])
    assert magic == 0x474B4341 and version == 1
    out, at = [], 16
    for _ in range(cases):
        before = _stream(raw[at:at + 56])
        cur_ts, budget, n_opts, n_frames, fam, listed = struct.unpack("<IHHHBB", raw[at + 56:at + 68])
        at += 68
        opts = np.frombuffer(raw, np.uint8, n_opts, at)
        at += (n_opts + 3) & ~3
        frames = np.frombuffer(raw, np.uint8, 66 * n_frames, at).reshape(n_frames, 66)
        at += 66 * n_frames
        after = _stream(raw[at:at + 56])
        at += 56
        before["on_ack_list"] = 1 if (before["ack_cnt"] or before["is_wack"]) else 0
        after["on_ack_list"] = listed
        out.append(dict(before=before, after=after, opts=opts, cur_ts=cur_ts, budget=budget, family=fam, frames=frames))
    assert at == len(raw)
    return out


def fixture_links():
    """The link table of the fixture's frames: entry i is 02:00:00:00:00:i (the
    ARP answer) and 02:01:00:00:00:i (the interface's address)."""
    links = np.zeros(3, dtype=xm.LINK_DTYPE)
    for i in range(3):
        links[i]["dst"], links[i]["src"] = (2, 0, 0, 0, 0, i), (2, 1, 0, 0, 0, i)
    return links
