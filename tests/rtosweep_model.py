"""A plain-Python model of include/mtcp_gpu_rtosweep.h in two parts (line
numbers: mtcp/src/).

The wheel: AddtoRTOList, CheckRtmTimeout and HandleRTO of timer.c restated line
by line over streams held as dicts, with the list and event functions as
counters: what tests/c/ref_rtosweep_gen.c ran with the reference's own code.

The sweep: the header's contract over the device's records (numpy arrays of
ACK_STATE_DTYPE and DATAGEN_STATE_DTYPE): the due test, the cap, the step, the
result records and the group table.  No GPU, no library."""
import os
import struct

import numpy as np

from mtcp_amd._types import ACK_STATE_DTYPE, DATAGEN_STATE_DTYPE, RTO_REC_DTYPE

M32 = 0xFFFFFFFF
RTO_HASH = 3000                                               # timer.h:7
TCP_MAX_RTX, TCP_MAX_SYN_RETRY, TCP_MAX_BACKOFF = 16, 7, 7    # tcp_in.h:66-68
(ST_CLOSED, ST_LISTEN, ST_SYN_SENT, ST_SYN_RCVD, ST_ESTABLISHED, ST_FIN_WAIT_1, ST_FIN_WAIT_2, ST_CLOSE_WAIT,
 ST_CLOSING, ST_LAST_ACK, ST_TIME_WAIT) = range(11)           # tcp_in.h:70-83
CONN_FAIL, CONN_LOST = 3, 4                                   # tcp_in.h:101-102
NONE, BAD, DEFER_STATE, LOST, RETRANSMIT = range(5)           # enum mtcp_gpu_rto_verdict
SEND_LIST_ADD = 0x01
CALLS = ("send_list", "control_list", "error_event", "destroy")


def s32(v: int) -> int:
    v &= M32
    return v - (1 << 32) if v & 0x80000000 else v


def seq_lt(a: int, b: int) -> bool:
    """TCP_SEQ_LT (tcp_in.h:37-41)."""
    return s32(a - b) < 0


# ---- the wheel (timer.c) ----------------------------------------------------------
class Wheel:
    """struct rto_hashstore with mtcp->rto_list_cnt (timer.h:10-15)."""

    def __init__(self):
        self.rto_now_idx, self.rto_now_ts, self.cnt = 0, 0, 0
        self.lists = [[] for _ in range(RTO_HASH + 1)]


def add_to_rto_list(w: Wheel, s: dict) -> None:
    """AddtoRTOList, timer.c:30-60."""
    if not w.cnt:                                             # :32-35
        w.rto_now_idx, w.rto_now_ts = 0, s["ts_rto"]
    if s["on_rto_idx"] < 0:                                   # :37
        diff = s32(s["ts_rto"] - w.rto_now_ts)                # :47
        if diff < RTO_HASH:                                   # :48-52
            assert diff >= 0, "the C remainder of a negative index"
            s["on_rto_idx"] = (diff + w.rto_now_idx) % RTO_HASH
        else:                                                 # :53-56
            s["on_rto_idx"] = RTO_HASH
        w.lists[s["on_rto_idx"]].append(s)
        w.cnt += 1                                            # :58


def handle_rto(s: dict, calls: dict) -> int:
    """HandleRTO, timer.c:176-337; the list and event functions count."""
    if s["nrtx"] < TCP_MAX_RTX:                               # :186-187
        s["nrtx"] += 1
    else:
        if s["state"] < ST_ESTABLISHED:                       # :191-194
            s["state"], s["close_reason"] = ST_CLOSED, CONN_FAIL
            calls["destroy"] += 1
        else:                                                 # :196-202
            s["state"], s["close_reason"] = ST_CLOSED, CONN_LOST
            calls["error_event" if s["has_socket"] else "destroy"] += 1
        return -1                                             # :205
    if s["nrtx"] > s["max_nrtx"]:                             # :207-209
        s["max_nrtx"] = s["nrtx"]
    if s["state"] >= ST_ESTABLISHED:                          # :212-224
        backoff = min(s["nrtx"], TCP_MAX_BACKOFF)
        rto_prev = s["rto"]
        s["rto"] = ((((s["srtt"] >> 3) + s["rttvar"]) & M32) << backoff) & M32
        if s["rto"] == 0:                                     # unsigned: "<= 0" is "== 0"
            s["rto"] = rto_prev
    elif s["state"] >= ST_SYN_SENT:                           # :225-230
        if s["nrtx"] < TCP_MAX_BACKOFF:
            s["rto"] = (s["rto"] << 1) & M32
    s["ssthresh"] = min(s["cwnd"], s["peer_wnd"]) // 2        # :234
    if s["ssthresh"] < 2 * s["mss"]:                          # :235-237
        s["ssthresh"] = s["mss"] * 2
    s["cwnd"] = s["mss"]                                      # :238
    st = s["state"]
    if st == ST_SYN_SENT:                                     # :249-265
        if s["nrtx"] > TCP_MAX_SYN_RETRY:
            s["state"], s["close_reason"] = ST_CLOSED, CONN_FAIL
            calls["error_event" if s["has_socket"] else "destroy"] += 1
            return -1
    elif st not in (ST_SYN_RCVD, ST_ESTABLISHED, ST_CLOSE_WAIT, ST_LAST_ACK, ST_FIN_WAIT_1, ST_CLOSING):
        return -1                                             # :297-303
    s["snd_nxt"] = s["snd_una"]                               # :305
    if st in (ST_ESTABLISHED, ST_CLOSE_WAIT):                 # :306-309
        calls["send_list"] += 1
    elif st in (ST_FIN_WAIT_1, ST_CLOSING, ST_LAST_ACK):      # :311-330
        if seq_lt(s["snd_nxt"], s["fss"]):
            calls["send_list"] += 1                           # no stream of the cases is on the control list
        else:
            calls["control_list"] += 1
    else:                                                     # :332-333
        calls["control_list"] += 1
    return 0


def check_rtm_timeout(w: Wheel, cur_ts: int, thresh: int, calls_of) -> list:
    """CheckRtmTimeout, timer.c:363-419.  calls_of(stream) -> its counter dict.
    Returns the streams that fired, in the wheel's order."""
    fired = []
    if not w.cnt:                                             # :369-371
        return fired
    cnt = 0
    while True:
        lst = w.lists[w.rto_now_idx]                          # :379
        if s32(cur_ts - w.rto_now_ts) < 0:                    # :380-382
            break
        for s in list(lst):                                   # :384-405
            cnt += 1
            if cnt > thresh:                                  # :386-388
                break
            if s["on_rto_idx"] >= 0:                          # :394-398
                lst.remove(s)
                w.cnt -= 1
                s["on_rto_idx"] = -1
                fired.append(s)
                handle_rto(s, calls_of(s))
        if cnt > thresh:                                      # :407-408
            break
        w.rto_now_idx = (w.rto_now_idx + 1) % RTO_HASH        # :410-411
        w.rto_now_ts = (w.rto_now_ts + 1) & M32
        if w.rto_now_idx % 1000 == 0:                         # :412-414: RearrangeRTOStore, :340-360
            over = w.lists[RTO_HASH]
            for s in list(over):
                diff = s32(w.rto_now_ts - s["ts_rto"])        # :349
                if diff < RTO_HASH:
                    over.remove(s)
                    s["on_rto_idx"] = (diff + w.rto_now_idx) % RTO_HASH
                    w.lists[s["on_rto_idx"]].append(s)
    return fired


# ---- the sweep (include/mtcp_gpu_rtosweep.h) ---------------------------------------
def snd_is_bad(snd):
    """mtcp_gpu_ackwalk.h's rule, elementwise."""
    return ((snd["rsvd"] != 0) | (snd["eff_mss"] == 0) | (snd["wscale_peer"] > 31) | (snd["sb_size"] > (1 << 30)) |
            (snd["sb_len"] > snd["sb_size"]))


def dtx_is_bad(dtx):
    """mtcp_gpu_datagen.h's rule, elementwise."""
    return dtx["rsvd"].any(axis=-1) | (dtx["on_send_list"] > 1) | (dtx["on_control_list"] > 1)


def due_ids(snd, cur_ts: int):
    """on_rto == 1 and (int32_t)(cur_ts - ts_rto) >= 0, ascending id."""
    diff = (np.uint32(cur_ts & M32) - snd["ts_rto"]).astype(np.uint32)
    return np.flatnonzero((snd["on_rto"] == 1) & (diff < 0x80000000))


def sweep(snd, dtx, cur_ts: int, cap: int):
    """mtcp_gpu_rto_sweep[_dev]: (snd after, dtx after, rto[handled],
    seg_sid[handled], seg_start[cap + 1], seg_stop[cap], nseg, total[2]).
    Nothing is modified."""
    assert snd.dtype == ACK_STATE_DTYPE and dtx.dtype == DATAGEN_STATE_DTYPE and len(snd) == len(dtx)
    snd, dtx = snd.copy(), dtx.copy()
    due = due_ids(snd, cur_ts)
    ids = due[:cap]
    s, d = snd[ids], dtx[ids]                                 # copies: the records as the call found them
    bad = snd_is_bad(s) | dtx_is_bad(d)
    defer = ~bad & (s["tcp_state"] != ST_ESTABLISHED)
    lost = ~bad & ~defer & (s["nrtx"] >= TCP_MAX_RTX)         # timer.c:186-206
    rtx = ~bad & ~defer & ~lost
    verdict = np.select([bad, defer, lost], [BAD, DEFER_STATE, LOST], RETRANSMIT).astype(np.uint8)
    out = s.copy()
    out["on_rto"][lost | rtx] = 0                             # timer.c:395-397
    out["tcp_state"][lost] = ST_CLOSED                        # timer.c:196
    nrtx = s["nrtx"].astype(np.uint32) + 1                    # timer.c:187
    backoff = np.minimum(nrtx, TCP_MAX_BACKOFF)               # timer.c:214
    rto = (((s["srtt"] >> 3) + s["rttvar"]).astype(np.uint32).astype(np.uint64) << backoff.astype(np.uint64)) \
        .astype(np.uint32)                                    # timer.c:217-218, in uint32_t with its wrap
    rto = np.where(rto == 0, s["rto"], rto)                   # timer.c:219-224
    mss = s["mss"].astype(np.uint32)
    ssthresh = np.minimum(s["cwnd"], s["peer_wnd"]) // 2      # timer.c:234
    ssthresh = np.where(ssthresh < 2 * mss, 2 * mss, ssthresh)   # timer.c:235-237
    out["nrtx"][rtx] = nrtx[rtx]
    out["rto"][rtx] = rto[rtx]
    out["ssthresh"][rtx] = ssthresh[rtx]
    out["cwnd"][rtx] = mss[rtx]                               # timer.c:238
    out["snd_nxt"][rtx] = s["snd_una"][rtx]                   # timer.c:305
    listed = rtx & (s["has_sndbuf"] != 0)                     # tcp_out.c:842-848
    added = listed & (d["on_send_list"] == 0)                 # tcp_out.c:850-851
    dout = d.copy()
    dout["on_send_list"][listed] = 1
    snd[ids], dtx[ids] = out, dout
    rec = np.zeros(len(ids), dtype=RTO_REC_DTYPE)
    rec["sid"], rec["rto"], rec["nrtx"], rec["verdict"] = ids, out["rto"], out["nrtx"], verdict
    rec["flags"] = np.where(added, SEND_LIST_ADD, 0)
    total = np.array([len(due), len(ids)], dtype=np.uint64)
    return (snd, dtx, rec, ids.astype(np.uint32), np.zeros(cap + 1, np.uint32), np.zeros(cap, np.uint32), len(ids),
            total)


# ---- the reference fixture --------------------------------------------------------
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rtosweep_cases.bin")
FAMILIES = ("around cur_ts", "several ticks in one call", "the count and the LOST exit", "the rto arithmetic",
            "ssthresh and its floor", "the send list", "the host's states", "random mixes")
WORDS = ("snd_nxt", "snd_una", "peer_wnd", "cwnd", "ssthresh", "rto", "ts_rto", "srtt", "rttvar", "fss")
BYTES = ("state", "nrtx", "max_nrtx", "on_rto", "has_sndbuf", "on_send_list", "has_socket", "close_reason", "fired",
         "pad") + CALLS
REC = 56


def _record(raw: bytes) -> dict:
    s = dict(zip(WORDS, struct.unpack("<10I", raw[:40])))
    s["mss"], = struct.unpack("<H", raw[40:42])
    s.update(zip(BYTES, raw[42:56]))
    assert s.pop("pad") == 0
    return s


def load_fixture(path: str = FIXTURE) -> list:
    """The cases tests/c/ref_rtosweep_gen.c wrote: dicts with family, before
    (one record per stream) and calls: (cur_ts, one record per stream) each."""
    raw = open(path, "rb").read()
    magic, version, cases, _ = struct.unpack("<4I", raw[:16])
    assert magic == 0x534F5452 and version == 1
    out, at = [], 16
    for _ in range(cases):
        fam, ns, nc, _ = raw[at:at + 4]
        at += 4
        before = [_record(raw[at + REC * i:at + REC * (i + 1)]) for i in range(ns)]
        at += REC * ns
        calls = []
        for _ in range(nc):
            cur_ts, = struct.unpack("<I", raw[at:at + 4])
            at += 4
            calls.append((cur_ts, [_record(raw[at + REC * i:at + REC * (i + 1)]) for i in range(ns)]))
            at += REC * ns
        out.append(dict(family=fam, before=before, calls=calls))
    assert at == len(raw)
    return out


def mirrors(records):
    """Fixture records as the device's mirrors: stream i has id i.  What the
    fixture does not hold is set so that the record is not BAD (eff_mss 1 where
    mss is below 13) and a send buffer of 4000, 700 or 90 bytes from snd_una is there."""
    n = len(records)
    snd, dtx = np.zeros(n, dtype=ACK_STATE_DTYPE), np.zeros(n, dtype=DATAGEN_STATE_DTYPE)
    for i, r in enumerate(records):
        for f in ("snd_nxt", "snd_una", "peer_wnd", "cwnd", "ssthresh", "rto", "ts_rto", "srtt", "rttvar", "mss",
                  "nrtx", "on_rto", "has_sndbuf"):
            snd[i][f] = r[f]
        snd[i]["tcp_state"] = r["state"]
        snd[i]["eff_mss"] = max(r["mss"] - 12, 1)
        snd[i]["sb_head_seq"], snd[i]["sb_len"], snd[i]["sb_size"] = r["snd_una"], (4000, 700, 90)[i % 3], 8192
        snd[i]["user"] = (i * 7 + np.arange(40)) & 0xFF
        dtx[i]["sb_off"], dtx[i]["sb_base_seq"] = 1 + 4002 * i, r["snd_una"]
        dtx[i]["on_send_list"] = r["on_send_list"]
    return snd, dtx


# ---- the send side behind a sweep (mtcp_gpu_rto_send_dev) --------------------------
N_LINKS, SLOT, ARENA_STRIDE = 3, 1600, 4002


def send_side(n: int, seed: int):
    """What the data generation reads beyond snd and dtx for n streams laid out
    as mirrors() does: (state, tx, payload)."""
    from mtcp_amd._types import RCV_STATE_DTYPE
    from tests import ackgen_model as am
    rng = np.random.default_rng(seed)
    state, tx = np.zeros(n, dtype=RCV_STATE_DTYPE), np.zeros(n, dtype=am.STATE_DTYPE)
    state["rcv_nxt"], state["ts_recent"] = rng.integers(0, 1 << 32, n), rng.integers(0, 1 << 32, n)
    state["rcv_wnd"], state["tcp_state"] = rng.integers(1 << 15, 1 << 20, n), ST_ESTABLISHED
    tx["saddr"], tx["daddr"] = rng.integers(0, 1 << 32, n), rng.integers(0, 1 << 32, n)
    tx["sport"], tx["dport"], tx["ip_id"] = (rng.integers(0, 1 << 16, n) for _ in range(3))
    tx["wscale_mine"], tx["link"], tx["has_rcvbuf"] = rng.integers(0, 15, n), rng.integers(0, N_LINKS, n), 1
    tx["ts_lastack_sent"] = rng.integers(0, 1 << 32, n)
    payload = rng.integers(0, 256, ARENA_STRIDE * n + 16, dtype=np.uint8)
    return state, tx, payload


def send(snd, dtx, cur_ts: int, cap: int, state, tx, payload_bytes: int, seg_cap: int):
    """mtcp_gpu_rto_send_dev: the sweep, then tests/datagen_model.py over the
    table it wrote with ack None and n = cap.  Returns (the sweep's tuple, the
    data generation's tuple)."""
    from tests import datagen_model as dm
    sw = sweep(snd, dtx, cur_ts, cap)
    snd1, dtx1, _, seg_sid, seg_start, seg_stop, nseg, _ = sw
    sid = np.zeros(cap, np.uint32)
    sid[:nseg] = seg_sid
    dg = dm.datagen(None, None, cap, len(snd) - 1, np.zeros(cap, np.uint32), sid, seg_start, nseg, seg_stop, state,
                    snd1, tx, dtx1, cur_ts, payload_bytes, N_LINKS, 0, seg_cap * SLOT, 0, SLOT, seg_cap)
    return sw, dg


def flush_bytes(mss: int, peer_wnd: int, buffered: int) -> tuple:
    """What FlushTCPSendingBuffer's loop (tcp_out.c:401-443) sends from snd_una
    right after HandleRTO: whole packets of at most mss - 12 bytes while they
    fit MIN(cwnd, peer_wnd) = MIN(mss, peer_wnd).  (segments, bytes)."""
    window, sent, segs = min(mss, peer_wnd), 0, 0
    while buffered - sent > 0:
        ln = min(buffered - sent, mss - 12)
        if sent + ln > window:                                # tcp_out.c:421-433
            break
        sent, segs = sent + ln, segs + 1
    return segs, sent
