"""TEST INFRASTRUCTURE ONLY — FlushTCPSendingBuffer's walk (mtcp/src/tcp_out.c:
357-449) over the streams of a send list as WriteTCPDataList runs it
(tcp_out.c:587-674), restated in Python as include/mtcp_gpu_txseg.h states it:
a `while` per burst, one iteration per segment, the reference's comparisons in
the reference's order.  The expected records, descriptors, results and totals
of every f8 test come from here, never from the C plan or the kernels, and
nothing here is a closed form: no division, no count computed ahead of the
loop.

The stream's state is the burst's snapshot: snd_nxt = seq, snd_una = seq -
in_flight, sndbuf->head at payload_off - (bytes sent so far), cwnd/peer_wnd
folded into `window` and `peer_wnd`.  get_wptr (eth_out.c:58) is the slot
rule of the header: it has no room (IPOutput NULL, tcp_out.c:238-240) where a
record index reaches seg_cap, a frame ends past buf_len or an offset needs more
than 32 bits.
"""
from __future__ import annotations

import numpy as np

from .txbuild_model import ACK, DEFAULT_MSS, DESC_DTYPE, SEG_DTYPE

BURST_DTYPE = np.dtype([
    ("payload_off", "<u8"), ("saddr", "<u4"), ("daddr", "<u4"), ("sport", "<u2"), ("dport", "<u2"),
    ("seq", "<u4"), ("ack", "<u4"), ("ts_val", "<u4"), ("ts_ecr", "<u4"), ("len", "<u4"),
    ("in_flight", "<u4"), ("window", "<u4"), ("peer_wnd", "<u4"), ("tcp_window", "<u2"), ("ip_id", "<u2"),
    ("mss", "<u2"), ("link", "u1"), ("rsvd0", "u1"), ("rsvd1", "<u4"),
])
RESULT_DTYPE = np.dtype([("first_seg", "<u4"), ("n_seg", "<u4"), ("bytes", "<u4"), ("status", "u1"),
                         ("stop", "u1"), ("rsvd", "<u2")])
assert BURST_DTYPE.itemsize == 64 and RESULT_DTYPE.itemsize == 16

OK, BAD_BURST, BAD_PAYLOAD = 0, 1, 2
STOP_WINDOW, STOP_PEER_WINDOW, STOP_NO_ROOM = 0x1, 0x2, 0x4
VOID_FORM = 0xFF
OPTLEN_ACK = 12             # CalculateOptionLength(TCP_FLAG_ACK), tcp_out.c:21-60: timestamps on, SACK off


def align_of(off_shift: int) -> int:
    return max(2, 1 << off_shift)


def status_of(b, payload_bytes: int, n_links: int, slot_bytes: int, max_mss: int) -> int:
    """The per-burst status of include/mtcp_gpu_txseg.h, in its order."""
    mss = int(b["mss"])
    if b["rsvd0"] or b["rsvd1"] or mss < 13:
        return BAD_BURST
    maxlen = mss - OPTLEN_ACK
    if maxlen > max_mss + OPTLEN_ACK or 66 + maxlen > 65535 or (slot_bytes and 66 + maxlen > slot_bytes):
        return BAD_BURST
    if int(b["link"]) >= n_links or int(b["in_flight"]) + int(b["len"]) > 0xFFFFFFFF:
        return BAD_BURST
    if int(b["payload_off"]) + int(b["len"]) > payload_bytes:
        return BAD_PAYLOAD
    return OK


def void_records(n: int) -> np.ndarray:
    seg = np.zeros(n, dtype=SEG_DTYPE)
    seg["form"] = VOID_FORM
    return seg


def expand(bursts, payload_bytes: int, n_links: int, buf_off: int, buf_len: int, off_shift: int,
           slot_bytes: int, seg_cap: int, max_mss: int = 0):
    """(seg[seg_cap], desc[seg_cap], res[len(bursts)], total[2]) of
    mtcp_gpu_tx_segment_dev for these arguments."""
    A = align_of(off_shift)
    assert slot_bytes % A == 0 and buf_off % A == 0 and seg_cap > 0
    mm = max_mss or DEFAULT_MSS
    seg, desc = void_records(seg_cap), np.zeros(seg_cap, dtype=DESC_DTYPE)
    res = np.zeros(len(bursts), dtype=RESULT_DTYPE)
    k = 0                    # records emitted: the index of the next one
    slot = buf_off           # where the next slot begins
    full = False             # get_wptr has answered NULL: WriteTCPDataList has stopped (tcp_out.c:633-636)
    rows = []                # (burst, payload_off, seq, ip_id, payload_len, offset) of every record
    for i, (b, r) in enumerate(zip(bursts, res)):
        r["first_seg"] = k
        r["status"] = status_of(b, payload_bytes, n_links, slot_bytes, mm)
        if r["status"]:
            continue
        maxlen = int(b["mss"]) - OPTLEN_ACK                         # tcp_out.c:360
        window, peer_wnd = int(b["window"]), int(b["peer_wnd"])     # tcp_out.c:382
        snd_nxt = int(b["seq"])
        snd_una = snd_nxt - int(b["in_flight"])                     # unwrapped: the header's 64-bit test
        end_seq = snd_nxt + int(b["len"])                           # head_seq + sndbuf->len
        ip_id = int(b["ip_id"])
        packets, sent, stop = 0, 0, 0
        while True:                                                 # tcp_out.c:384
            seq = snd_nxt
            buffered_len = end_seq - seq                            # tcp_out.c:395
            if buffered_len == 0:                                   # tcp_out.c:401
                break
            data = int(b["payload_off"]) + (seq - int(b["seq"]))    # tcp_out.c:404-405
            if buffered_len > maxlen:                               # tcp_out.c:407-411
                ln = maxlen
            else:
                ln = buffered_len
            if seq - snd_una + ln > window:                         # tcp_out.c:421
                stop = STOP_WINDOW                                  # tcp_out.c:433: -3
                if seq - snd_una + ln > peer_wnd:                   # tcp_out.c:423
                    stop |= STOP_PEER_WINDOW
                break
            # SendTCPPacket(..., TCP_FLAG_ACK, data, len) (tcp_out.c:437): IPOutput asks for the slot first
            frame = 66 + ln
            if full or k >= seg_cap or slot + frame > buf_len or (slot >> off_shift) > 0xFFFFFFFF:
                full = True
                stop = STOP_NO_ROOM                                 # tcp_out.c:238-240, :439-441: -2
                break
            rows.append((i, data, seq & 0xFFFFFFFF, ip_id, ln, slot >> off_shift))   # tcp_out.c:284, ip_out.c:139
            ip_id = (ip_id + 1) & 0xFFFF
            slot += slot_bytes if slot_bytes else (frame + A - 1) // A * A      # pslib.c:146
            k += 1
            snd_nxt += ln                                           # tcp_out.c:332
            sent += ln
            packets += 1                                            # tcp_out.c:443
        r["n_seg"], r["bytes"], r["stop"] = packets, sent, stop
    if rows:
        src, data, seqs, ids, lens, offs = (np.array(c, dtype=np.uint64) for c in zip(*rows))
        s, src = seg[:k], src.astype(np.int64)
        for f in ("saddr", "daddr", "sport", "dport", "ack", "ts_val", "ts_ecr", "mss", "link"):
            s[f] = bursts[f][src]
        s["window"] = bursts["tcp_window"][src]
        s["payload_off"], s["seq"], s["ip_id"], s["payload_len"] = data, seqs, ids, lens
        s["flags"], s["form"], s["wscale"] = ACK, 1, 0              # TCP_FLAG_ACK alone (tcp_out.c:437)
        desc["offset"][:k], desc["len"][:k] = offs, lens + np.uint64(66)
    return seg, desc, res, np.array([k, slot - buf_off], dtype=np.uint64)


def random_bursts(n: int, seed: int, payload_bytes: int, n_links: int = 3, mss_choices=(536, 1460, 1460, 8960),
                  max_len: int = 70000, p_stop: float = 0.25, p_empty: float = 0.05):
    """n plausible bursts into a payload buffer of payload_bytes: a share of
    them empty, a share with a window that stops the walk somewhere."""
    rng = np.random.default_rng(seed)
    b = np.zeros(n, dtype=BURST_DTYPE)
    for f in ("saddr", "daddr", "seq", "ack", "ts_val", "ts_ecr"):
        b[f] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    for f in ("sport", "dport", "tcp_window", "ip_id"):
        b[f] = rng.integers(0, 1 << 16, n)
    b["link"] = rng.integers(0, n_links, n)
    b["mss"] = rng.choice(mss_choices, n)
    ln = np.minimum(np.exp(rng.uniform(0, np.log(max_len), n)).astype(np.int64), max(payload_bytes, 1) - 1)
    ln[rng.random(n) < p_empty] = 0
    b["len"] = ln
    b["payload_off"] = (rng.random(n) * (payload_bytes - ln)).astype(np.int64)
    infl = rng.integers(0, 20000, n)
    b["in_flight"] = infl
    window = infl + ln + rng.integers(0, 5000, n)                   # open: the whole burst passes
    stopped = rng.random(n) < p_stop
    cut = (rng.random(n) * (ln + 1)).astype(np.int64)               # closes somewhere inside the burst
    window[stopped] = (infl + cut)[stopped]
    below = stopped & (rng.random(n) < 0.1)                         # a window below what is in flight already
    window[below] = (infl // 2)[below]
    b["window"] = window
    rel = rng.integers(0, 3, n)                                     # peer_wnd above, equal to, below window
    b["peer_wnd"] = np.clip(window + (rel - 1) * rng.integers(1, 4000, n), 0, 0xFFFFFFFF)
    return b


def _burst(**kw):
    b = np.zeros(1, dtype=BURST_DTYPE)
    b["saddr"], b["daddr"], b["sport"], b["dport"] = 0x0A000001, 0x0A000002, 0x1234, 0x5000
    b["seq"], b["ack"], b["ts_val"], b["ts_ecr"] = 1000, 2000, 3000, 4000
    b["tcp_window"], b["ip_id"], b["mss"], b["link"] = 0x7210, 7, 1460, 1
    b["window"] = b["peer_wnd"] = 0xFFFFFFFF
    for k, v in kw.items():
        b[k] = v
    return b


def _lay_out(parts):
    """The bursts of `parts` with their payloads back to back from byte 1."""
    b = np.concatenate(parts)
    at = 1
    for x in b:
        x["payload_off"] = at
        at += int(x["len"]) + 1
    return b, at


def edge_lists():
    """The edge lists of the f8 tests: (name, bursts, arguments of expand)."""
    out = []
    roomy = dict(n_links=3, buf_off=0, buf_len=1 << 40, off_shift=0, slot_bytes=0, seg_cap=512)

    # every length around a segment boundary at every mss
    parts = []
    for mss in (13, 14, 536, 1460, 8960, 65481):
        m = mss - OPTLEN_ACK
        for ln in (0, 1, m - 1, m, m + 1, 2 * m, 2 * m + 1):
            parts.append(_burst(mss=mss, len=ln))
    b, nbytes = _lay_out(parts)
    out.append(("lengths", b, dict(roomy, payload_bytes=nbytes, max_mss=65535)))

    # windows: below what is in flight, none, exactly k full segments, stopping at the tail, exactly all;
    # peer_wnd above, equal to and below window
    m, parts = 1448, []
    ln, infl = 5 * m + 100, 3000
    for w in [-1, 0, m - 1] + [k * m for k in range(1, 6)] + [k * m + 1 for k in range(1, 5)] + [ln - 1, ln, ln + 1]:
        for dp in (500, 0, -500):
            window = max(infl + w, 0) if w >= 0 else infl // 2
            parts.append(_burst(len=ln, in_flight=infl, window=window, peer_wnd=max(window + dp, 0)))
    parts.append(_burst(len=ln, in_flight=0, window=0, peer_wnd=0))
    b, nbytes = _lay_out(parts)
    out.append(("windows", b, dict(roomy, payload_bytes=nbytes, max_mss=0)))

    # wrap-around of ip_id and seq
    b, nbytes = _lay_out([_burst(len=4 * 1448 + 5, ip_id=0xFFFE, seq=0xFFFFFF00),
                          _burst(len=3 * 524, mss=536, ip_id=0xFFFF, seq=0xFFFFFFFF)])
    out.append(("wrap", b, dict(roomy, payload_bytes=nbytes, max_mss=0)))

    # every refusal, one at a time, between good bursts
    good = lambda: _burst(len=2000)
    parts = [good(), _burst(len=2000, rsvd0=1), good(), _burst(len=2000, rsvd1=1), _burst(len=2000, mss=12),
             _burst(len=2000, mss=0), good(), _burst(len=2000, mss=1500), _burst(len=2000, link=3),
             _burst(len=2000, in_flight=0xFFFFFFFF), good(), _burst(len=0xFFFFFFFF, in_flight=1), good()]
    b, nbytes = _lay_out(parts)
    b[-2]["payload_off"] = 1
    bad_payload = [_burst(len=2000, payload_off=nbytes - 1999), _burst(len=0, payload_off=nbytes + 1),
                   _burst(len=2000, payload_off=nbytes - 2000), _burst(len=0, payload_off=nbytes),
                   _burst(len=5, payload_off=0xFFFFFFFFFFFFFFFE)]
    b = np.concatenate([b] + bad_payload)
    out.append(("refusals", b, dict(roomy, payload_bytes=nbytes, max_mss=0)))
    out.append(("refusals_fixed_slots", b, dict(roomy, payload_bytes=nbytes, max_mss=0, slot_bytes=1536)))
    b2, nb2 = _lay_out([good(), _burst(len=3000, mss=1460), _burst(len=3000, mss=536), good()])
    out.append(("frame_above_slot", b2, dict(roomy, payload_bytes=nb2, max_mss=0, slot_bytes=1024)))
    b3, nb3 = _lay_out([_burst(len=70000, mss=65482), _burst(len=70000, mss=65481)])
    out.append(("frame_above_64k", b3, dict(roomy, payload_bytes=nb3, max_mss=65535)))

    # room: six bursts of three segments, a stopped one and an empty one among them
    parts = [_burst(len=2 * 1448 + 10, ip_id=100 * i) for i in range(6)]
    parts.insert(2, _burst(len=0))
    parts.insert(4, _burst(len=5000, window=10, peer_wnd=5))
    b, nbytes = _lay_out(parts)
    for off_shift in (0, 1, 6):
        A = align_of(off_shift)
        for slot_bytes in (0, 1536):
            base = dict(payload_bytes=nbytes, n_links=3, buf_off=4 * A, off_shift=off_shift, slot_bytes=slot_bytes,
                        max_mss=0)
            tag = f"shift{off_shift}_{'fixed' if slot_bytes else 'packed'}"
            out.append((f"room_none_{tag}", b, dict(base, buf_len=1 << 40, seg_cap=64)))
            _, d, _, tot = expand(b, **dict(base, buf_len=1 << 40, seg_cap=64))
            assert int(tot[0]) == 18
            out.append((f"room_exact_cap_{tag}", b, dict(base, buf_len=1 << 40, seg_cap=18)))
            for cut, where in ((6, "boundary"), (7, "inside"), (8, "inside2")):
                out.append((f"room_cap_{where}_{tag}", b, dict(base, buf_len=1 << 40, seg_cap=cut)))
                end = (int(d["offset"][cut - 1]) << off_shift) + int(d["len"][cut - 1])
                out.append((f"room_buf_{where}_{tag}", b, dict(base, buf_len=end, seg_cap=64)))
                out.append((f"room_buf_{where}_short_{tag}", b, dict(base, buf_len=end - 1, seg_cap=64)))
                # record `cut` is the first whose offset does not fit 32 bits
                rel = (int(d["offset"][cut]) << off_shift) - base["buf_off"]
                far = ((0xFFFFFFFF << off_shift) // A + 1) * A - rel
                out.append((f"room_off_{where}_{tag}", b, dict(base, buf_off=far, buf_len=1 << 62, seg_cap=64)))
    out.append(("room_buf_off_past_buf_len", b, dict(base, buf_off=1 << 20, buf_len=1 << 10, seg_cap=64)))
    out.append(("room_buf_off_past_32_bits", b, dict(base, off_shift=0, buf_off=1 << 33, buf_len=1 << 40, seg_cap=64)))
    return out
