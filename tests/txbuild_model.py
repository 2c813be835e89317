"""TEST INFRASTRUCTURE ONLY — the reference's tx frame builders restated in
numpy/Python: SendTCPPacketStandalone and SendTCPPacket (mtcp/src/tcp_out.c:
135-354) with CalculateOptionLength (tcp_out.c:21-60), GenerateTCPOptions
(tcp_out.c:79-122), IPOutputStandalone / IPOutput (mtcp/src/ip_out.c:35-167),
EthernetOutput (mtcp/src/eth_out.c:35-80), ip_fast_csum (io_engine/include/
ps.h:66-95) and TCPCalcChecksum (mtcp/src/tcp_util.c:157-190), as
include/mtcp_gpu_txbuild.h states them.  The expected bytes of every frame
builder test come from here, from tests/golden/txbuild_frames.*.bin (frames
the reference's own code wrote) or from the oracle, never from the kernel.

The fixture is one stream of `u16 len | frame` records in send order, 4 054
frames and 1 784 508 bytes, cut at a record boundary into two files so that
each stays below 1 MiB (tests/make_txbuild_golden.py).
"""
from __future__ import annotations

import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE_PARTS = tuple(os.path.join(HERE, "golden", f"txbuild_frames.{i}.bin") for i in range(2))
FIXTURE_FRAMES, FIXTURE_BYTES = 4054, 1784508
PART_LIMIT = 1 << 20

DESC_DTYPE = np.dtype([("offset", "<u4"), ("len", "<u2"), ("flags", "u1"), ("rsvd", "u1")])
SEG_DTYPE = np.dtype([
    ("payload_off", "<u8"), ("saddr", "<u4"), ("daddr", "<u4"), ("sport", "<u2"), ("dport", "<u2"),
    ("seq", "<u4"), ("ack", "<u4"), ("ts_val", "<u4"), ("ts_ecr", "<u4"), ("window", "<u2"),
    ("ip_id", "<u2"), ("payload_len", "<u2"), ("mss", "<u2"), ("flags", "u1"), ("form", "u1"),
    ("wscale", "u1"), ("link", "u1"),
])
LINK_DTYPE = np.dtype([("dst", "u1", (6,)), ("src", "u1", (6,))])
assert SEG_DTYPE.itemsize == 48 and LINK_DTYPE.itemsize == 12

FIN, SYN, RST, PSH, ACK = 0x01, 0x02, 0x04, 0x08, 0x10
BUILT, BAD_SEG, BAD_DESC, BAD_PAYLOAD = 0, 1, 2, 3
NO_CSUM = 0x1
DEFAULT_MSS = 1460          # TCP_DEFAULT_MSS (tcp_in.h:33)


def optlen_of(flags: int) -> int:
    """CalculateOptionLength (tcp_out.c:21-60) with TCP_OPT_TIMESTAMP_ENABLED
    TRUE and TCP_OPT_SACK_ENABLED FALSE."""
    return 20 if flags & SYN else 12


def frame_len(flags: int, payload_len: int) -> int:
    return 54 + optlen_of(flags) + payload_len


def _fold(s: int) -> int:
    """tcp_util.c:184-188; also ip_fast_csum's result (ps.h:66-95)."""
    s = (s >> 16) + (s & 0xFFFF)
    s += s >> 16
    return ~s & 0xFFFF


def _words(b: np.ndarray) -> int:
    """Sum of the little-endian u16 words of b, an odd last byte alone
    (tcp_util.c:166-174)."""
    n = len(b) & ~1
    s = int(b[:n].view("<u2").sum(dtype=np.uint64)) if n else 0
    return s + (int(b[-1]) if len(b) & 1 else 0)


def build_frame(s, payload: np.ndarray, link, no_csum: bool = False) -> np.ndarray:
    """One segment's frame; s is a SEG_DTYPE record with a status of BUILT."""
    flags, form = int(s["flags"]), int(s["form"])
    optlen, plen = optlen_of(flags), int(s["payload_len"])
    f = np.zeros(54 + optlen + plen, dtype=np.uint8)
    # EthernetOutput (eth_out.c:72-77)
    f[0:6], f[6:12], f[12:14] = link["dst"], link["src"], (0x08, 0x00)
    # IPOutputStandalone / IPOutput (ip_out.c:66-76, :135-145)
    tot = 40 + optlen + plen
    ip_id = int(s["ip_id"])
    f[14:24] = (0x45, 0, tot >> 8, tot & 0xFF, ip_id >> 8, ip_id & 0xFF, 0x40, 0, 64, 6)
    f[26:30] = np.frombuffer(np.uint32(s["saddr"]).tobytes(), np.uint8)
    f[30:34] = np.frombuffer(np.uint32(s["daddr"]).tobytes(), np.uint8)
    # SendTCPPacketStandalone / SendTCPPacket (tcp_out.c:160-192, :240-300)
    t = f[34:]
    t[0:2] = np.frombuffer(np.uint16(s["sport"]).tobytes(), np.uint8)
    t[2:4] = np.frombuffer(np.uint16(s["dport"]).tobytes(), np.uint8)
    t[4:8] = np.frombuffer(int(s["seq"]).to_bytes(4, "big"), np.uint8)
    if flags & ACK:                                                      # tcp_out.c:175-178
        t[8:12] = np.frombuffer(int(s["ack"]).to_bytes(4, "big"), np.uint8)
    t[12] = ((20 + optlen) // 4) << 4
    t[13] = flags & 0x1F
    t[14:16] = (int(s["window"]) >> 8, int(s["window"]) & 0xFF)
    ts = np.frombuffer(int(s["ts_val"]).to_bytes(4, "big") + int(s["ts_ecr"]).to_bytes(4, "big"), np.uint8)
    o = t[20:20 + optlen]
    if form == 1 and flags & SYN:                                        # GenerateTCPOptions, tcp_out.c:79-114
        mss = int(s["mss"])
        o[0:4] = (2, 4, mss >> 8, mss % 256)
        o[4:8] = (1, 1, 8, 10)
        o[8:16] = ts
        o[16:20] = (1, 3, 3, int(s["wscale"]))
    else:                                   # tcp_out.c:185-190, :118-122; a form-0 SYN's bytes 12-19 stay
        o[0:4] = (1, 1, 8, 10)              # the memset's zeros (tcp_out.c:160)
        o[4:12] = ts
    t[20 + optlen:] = payload[int(s["payload_off"]):int(s["payload_off"]) + plen]
    if not no_csum:
        f[24:26] = np.frombuffer(np.uint16(_fold(_words(f[14:34]))).tobytes(), np.uint8)    # ip_out.c:94, :164
        pseudo = _words(f[26:34]) + 0x0600 + (((20 + optlen + plen) >> 8) | (((20 + optlen + plen) & 0xFF) << 8))
        t[16:18] = np.frombuffer(np.uint16(_fold(_words(t) + pseudo)).tobytes(), np.uint8)  # tcp_out.c:208-210
    return f


def status_of(s, d, n_links: int, payload_bytes: int, buf_len: int, off_shift: int, max_mss: int) -> int:
    """The per-segment status of include/mtcp_gpu_txbuild.h, in its order."""
    flags, plen = int(s["flags"]), int(s["payload_len"])
    optlen = optlen_of(flags)
    L = 54 + optlen + plen
    if flags & ~0x1F or s["form"] > 1 or s["link"] >= n_links or plen > max_mss + optlen or L > 65535:
        return BAD_SEG                                                   # tcp_out.c:149, :231
    off = int(d["offset"]) << off_shift
    if int(d["len"]) != L or off & 1 or off + L > buf_len:
        return BAD_DESC
    if int(s["payload_off"]) + plen > payload_bytes:
        return BAD_PAYLOAD
    return BUILT


def build_frames(seg, payload, links, desc, image, off_shift: int = 0, max_mss: int = 0, flags: int = 0):
    """mtcp_gpu_tx_build over a copy of `image` (what the buffer held before):
    (image, status).  Only built frames' bytes differ from the input."""
    image = np.array(image, dtype=np.uint8, copy=True)
    status = np.zeros(len(seg), dtype=np.uint8)
    mm = max_mss or DEFAULT_MSS
    for i, (s, d) in enumerate(zip(seg, desc)):
        status[i] = status_of(s, d, len(links), len(payload), len(image), off_shift, mm)
        if status[i] == BUILT:
            f = build_frame(s, payload, links[int(s["link"])], bool(flags & NO_CSUM))
            off = int(d["offset"]) << off_shift
            image[off:off + len(f)] = f
    return image, status


def segs_from_frames(frames, form: int = 0):
    """(seg, payload, links) whose frames are `frames` (a list of uint8 arrays
    built by the reference): the payloads back to back, one link entry per
    distinct Ethernet address pair."""
    seg = np.zeros(len(frames), dtype=SEG_DTYPE)
    links, pay, at = {}, [], 0
    for s, f in zip(seg, frames):
        f = np.asarray(f, dtype=np.uint8)
        key = f[0:12].tobytes()
        s["link"] = links.setdefault(key, len(links))
        t = f[34:]
        optlen = 4 * (int(t[12]) >> 4) - 20
        s["flags"], s["form"] = t[13], form
        assert optlen == optlen_of(int(t[13])) and f[14] == 0x45 and f[23] == 6, "not a frame of these builders"
        s["ip_id"] = (int(f[18]) << 8) | int(f[19])
        s["saddr"], s["daddr"] = f[26:30].copy().view("<u4")[0], f[30:34].copy().view("<u4")[0]
        s["sport"], s["dport"] = t[0:2].copy().view("<u2")[0], t[2:4].copy().view("<u2")[0]
        s["seq"], s["ack"] = int.from_bytes(t[4:8].tobytes(), "big"), int.from_bytes(t[8:12].tobytes(), "big")
        s["window"] = (int(t[14]) << 8) | int(t[15])
        s["ts_val"] = int.from_bytes(t[24:28].tobytes(), "big")
        s["ts_ecr"] = int.from_bytes(t[28:32].tobytes(), "big")
        body = t[20 + optlen:]
        s["payload_off"], s["payload_len"] = at, len(body)
        pay.append(body)
        at += len(body)
    table = np.zeros(len(links), dtype=LINK_DTYPE)
    for key, i in links.items():
        table[i]["dst"], table[i]["src"] = np.frombuffer(key[:6], np.uint8), np.frombuffer(key[6:], np.uint8)
    payload = np.concatenate(pay) if at else np.zeros(0, dtype=np.uint8)
    return seg, payload, table


def garbage_unread_fields(seg, seed: int = 7):
    """A copy of seg with the fields the builders never read filled with
    garbage: ack without TCP_FLAG_ACK, mss and wscale outside a form-1 SYN."""
    rng = np.random.default_rng(seed)
    out = seg.copy()
    out["ack"][(out["flags"] & ACK) == 0] = 0xDEADBEEF
    unread = ~((out["form"] == 1) & ((out["flags"] & SYN) != 0))
    out["mss"][unread] = rng.integers(1, 1 << 16, int(unread.sum()))
    out["wscale"][unread] = rng.integers(1, 256, int(unread.sum()))
    return out


def parse_stream(raw: np.ndarray) -> list:
    """The frames of a `u16 len | frame` stream."""
    frames, at = [], 0
    while at < len(raw):
        n = int(raw[at]) | (int(raw[at + 1]) << 8)
        frames.append(raw[at + 2:at + 2 + n])
        at += 2 + n
    assert at == len(raw)
    return frames


def load_fixture() -> list:
    raw = np.concatenate([np.fromfile(p, dtype=np.uint8) for p in FIXTURE_PARTS])
    return parse_stream(raw)


def slots(lens, slot: int, off_shift: int = 0, first: int = 0):
    """Descriptors of frames of `lens` bytes in slots of `slot` bytes from byte `first`."""
    desc = np.zeros(len(lens), dtype=DESC_DTYPE)
    desc["offset"] = (first + np.arange(len(lens), dtype=np.int64) * slot) >> off_shift
    desc["len"] = lens
    return desc


def mixed_segments(seed=11):
    """Both forms, every flag set with and without SYN, non-zero ip_id, odd
    source offsets, MSS and jumbo payloads."""
    rng = np.random.default_rng(seed)
    plens = [0, 1, 2, 3, 63, 64, 65, 127, 1447, 1448, 1449, 1460, 4000, 8948, 8960, 8972, 8980]
    seg = np.zeros(2 * 2 * len(plens), dtype=SEG_DTYPE)
    i, at = 0, 1
    for form in (0, 1):
        for syn in (0, SYN):
            for plen in plens:
                s = seg[i]
                s["form"], s["flags"] = form, syn | int(rng.choice([0, ACK, ACK | PSH, FIN | ACK, RST]))
                if plen > 8960 + optlen_of(int(s["flags"])):
                    plen = 8960 + optlen_of(int(s["flags"]))
                s["payload_off"], s["payload_len"] = at, plen
                at += plen + int(rng.integers(0, 3))
                s["saddr"], s["daddr"] = rng.integers(1, 1 << 32, 2, dtype=np.uint64)
                s["sport"], s["dport"] = rng.integers(1, 1 << 16, 2)
                s["seq"], s["ack"], s["ts_val"], s["ts_ecr"] = rng.integers(0, 1 << 32, 4, dtype=np.uint64)
                s["window"], s["ip_id"], s["mss"] = rng.integers(1, 1 << 16, 3)
                s["wscale"], s["link"] = rng.integers(0, 15), rng.integers(0, 3)
                i += 1
    payload = rng.integers(0, 256, at, dtype=np.uint8)
    links = np.zeros(3, dtype=LINK_DTYPE)
    links["dst"], links["src"] = rng.integers(0, 256, (3, 6)), rng.integers(0, 256, (3, 6))
    lens = [frame_len(int(s["flags"]), int(s["payload_len"])) for s in seg]
    desc = slots(lens, 9216)
    return seg, payload, links, desc, 9216 * len(seg)


def build_uniform(seg, payload, links, no_csum: bool = False) -> np.ndarray:
    """build_frame for segments that share flags and payload_len, all of
    status BUILT, vectorised: the frames as an (n, frame_len) array.  For
    batches too large for the per-segment loop (tools/txbuild_bench.py);
    tests/test_txbuild_model.py holds it to build_frame."""
    n, flags, plen = len(seg), int(seg["flags"][0]), int(seg["payload_len"][0])
    assert (seg["flags"] == flags).all() and (seg["payload_len"] == plen).all()
    optlen = optlen_of(flags)
    H = 54 + optlen
    Lp = (H + plen + 1) & ~1                     # one pad byte for the word view of an odd segment
    F = np.zeros((n, Lp), dtype=np.uint8)
    be32 = lambda a: np.ascontiguousarray(a, dtype=">u4").view(np.uint8).reshape(n, 4)
    be16 = lambda a: np.ascontiguousarray(a, dtype=">u2").view(np.uint8).reshape(n, 2)
    raw = lambda a: np.ascontiguousarray(a).view(np.uint8).reshape(n, -1)
    lk = links[seg["link"]]
    F[:, 0:6], F[:, 6:12], F[:, 12] = lk["dst"], lk["src"], 0x08
    F[:, 14], F[:, 20], F[:, 22], F[:, 23] = 0x45, 0x40, 64, 6
    F[:, 16:18] = be16(np.full(n, 40 + optlen + plen))
    F[:, 18:20] = be16(seg["ip_id"])
    F[:, 26:30], F[:, 30:34] = raw(seg["saddr"]), raw(seg["daddr"])
    F[:, 34:36], F[:, 36:38] = raw(seg["sport"]), raw(seg["dport"])
    F[:, 38:42] = be32(seg["seq"])
    if flags & ACK:
        F[:, 42:46] = be32(seg["ack"])
    F[:, 46], F[:, 47] = ((20 + optlen) // 4) << 4, flags & 0x1F
    F[:, 48:50] = be16(seg["window"])
    form1 = (seg["form"] == 1) & bool(flags & SYN)
    o = F[:, 54:54 + optlen]
    o[:, 0:4] = (1, 1, 8, 10)
    o[:, 4:8], o[:, 8:12] = be32(seg["ts_val"]), be32(seg["ts_ecr"])
    if form1.any():
        k = np.flatnonzero(form1)
        o[k, 4:8] = (1, 1, 8, 10)
        o[k, 8:12], o[k, 12:16] = be32(seg["ts_val"])[k], be32(seg["ts_ecr"])[k]
        o[k, 0], o[k, 1], o[k, 2], o[k, 3] = 2, 4, seg["mss"][k] >> 8, seg["mss"][k] & 0xFF
        o[k, 16], o[k, 17], o[k, 18], o[k, 19] = 1, 3, 3, seg["wscale"][k]
    if plen:
        off = seg["payload_off"].astype(np.int64)
        step = int(off[1] - off[0]) if n > 1 else plen
        if n > 1 and step >= 0 and (np.diff(off) == step).all():
            src = np.lib.stride_tricks.as_strided(payload[int(off[0]):], (n, plen), (step, 1), writeable=False)
        else:
            src = payload[off[:, None] + np.arange(plen)]
        F[:, H:H + plen] = src
    if not no_csum:
        fold = lambda s: ~((s >> 16) + (s & 0xFFFF) + (((s >> 16) + (s & 0xFFFF)) >> 16)) & 0xFFFF
        ip = F[:, 14:34].copy().view("<u2").sum(axis=1, dtype=np.uint64)
        F[:, 24:26] = fold(ip).astype("<u2").view(np.uint8).reshape(n, 2)
        tl = 20 + optlen + plen
        tcp = F[:, 34:].copy().view("<u2").sum(axis=1, dtype=np.uint64) + \
            F[:, 26:34].copy().view("<u2").sum(axis=1, dtype=np.uint64) + 0x0600 + ((tl >> 8) | ((tl & 0xFF) << 8))
        F[:, 50:52] = fold(tcp).astype("<u2").view(np.uint8).reshape(n, 2)
    return F[:, :H + plen]
