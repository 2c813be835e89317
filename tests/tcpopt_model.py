"""TEST INFRASTRUCTURE ONLY — the reference's two TCP option walks restated in
Python (ParseTCPTimestamp mtcp/src/tcp_util.c:61-92, ParseTCPOptions
tcp_util.c:14-59), the random option blocks they are pinned on, the golden
fixture's record layout and a builder that embeds option blocks in valid
IPv4/TCP frames.  The expected values of every option-record test come from
here or from tests/golden/tcpopt_cases.bin, never from the kernel.

Both walks run over tcpopt[0..len) but may read behind it: the length byte at
index len, the two MSS bytes up to len + 2, the timestamps up to len + 8.  The
restatement reports the highest index it read, and whether the reference would
never return (a skipped option of length 0 does `i += optlen - 2` and lands on
the same byte again).
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "tcpopt_cases.bin")
NCASES = 8192
BLOCK = 56                    # bytes stored per case: 40 of options + what a walk may read behind

TS_FOUND, MSS, WSCALE, SACK_PERMIT, SAW_TS, TS_UNPINNED, SYN_UNPINNED = 0x01, 0x02, 0x04, 0x08, 0x20, 0x40, 0x80
TCPOPT_DTYPE = np.dtype([("ts_val", "<u4"), ("ts_ref", "<u4"), ("ts_recent", "<u4"), ("mss", "<u2"),
                         ("wscale", "u1"), ("flags", "u1")])

# one fixture case: the block, and what the REFERENCE returned for it
# (nonterm bit 0: ParseTCPTimestamp would not return, bit 1: ParseTCPOptions;
# those walks were never passed to the reference and their outputs are 0)
CASE_DTYPE = np.dtype([("len", "u1"), ("nonterm", "u1"), ("bytes", "u1", (BLOCK,)),
                       ("ts_ret", "u1"), ("sack_permit", "u1"), ("saw_timestamp", "u1"), ("wscale", "u1"),
                       ("mss", "<u2"), ("eff_mss", "<u2"), ("seen", "u1"), ("rsvd", "u1"),
                       ("ts_val", "<u4"), ("ts_ref", "<u4"), ("ts_recent", "<u4")])
assert CASE_DTYPE.itemsize == 80


def _be32(b, i):
    return (int(b[i]) << 24) | (int(b[i + 1]) << 16) | (int(b[i + 2]) << 8) | int(b[i + 3])


def walk_ts(b, length: int) -> dict:
    """ParseTCPTimestamp (tcp_util.c:61-92) over b[0..length)."""
    r = dict(ret=0, ts_val=0, ts_ref=0, hi=-1, nonterm=False)
    i = 0
    while i < length:
        r["hi"] = max(r["hi"], i)
        opt = int(b[i]); i += 1
        if opt == 0:
            break
        if opt == 1:
            continue
        r["hi"] = max(r["hi"], i)
        optlen = int(b[i]); i += 1
        if i + optlen - 2 > length:
            break
        if opt == 8:
            r["hi"] = max(r["hi"], i + 7)
            r["ts_val"], r["ts_ref"], r["ret"] = _be32(b, i), _be32(b, i + 4), 1
            return r
        if optlen == 0:
            r["nonterm"] = True
            return r
        i += optlen - 2
    return r


def walk_syn(b, length: int) -> dict:
    """ParseTCPOptions (tcp_util.c:14-59) over b[0..length)."""
    r = dict(mss=0, eff_mss=0, wscale=0, sack_permit=0, saw_timestamp=0, ts_recent=0, seen=0, flags=0,
             hi=-1, nonterm=False)
    i = 0
    while i < length:
        r["hi"] = max(r["hi"], i)
        opt = int(b[i]); i += 1
        if opt == 0:
            break
        if opt == 1:
            continue
        r["hi"] = max(r["hi"], i)
        optlen = int(b[i]); i += 1
        if i + optlen - 2 > length:
            break
        if opt == 2:
            r["hi"] = max(r["hi"], i + 1)
            r["mss"] = (int(b[i]) << 8) + int(b[i + 1])
            r["eff_mss"] = (r["mss"] - 12) & 0xFFFF
            r["flags"] |= MSS
            r["seen"] |= MSS
            i += 2
        elif opt == 3:
            r["hi"] = max(r["hi"], i)
            r["wscale"] = int(b[i])
            r["flags"] |= WSCALE
            r["seen"] |= WSCALE
            i += 1
        elif opt == 4:
            r["sack_permit"] = 1
            r["flags"] |= SACK_PERMIT
        elif opt == 8:
            r["hi"] = max(r["hi"], i + 3)
            r["saw_timestamp"], r["ts_recent"] = 1, _be32(b, i)
            r["flags"] |= SAW_TS
            i += 8
        else:
            if optlen == 0:
                r["nonterm"] = True
                return r
            i += optlen - 2
    return r


def expected_record(b, length: int, tcp_flags: int, avail: int) -> np.void:
    """The mtcp_gpu_tcpopt record of a TCP_OK frame whose option block is
    b[0..length) (length = 4*doff - 20) with `avail` bytes from the first
    option byte to the frame's end; b holds at least length + 9 bytes."""
    rec = np.zeros((), dtype=TCPOPT_DTYPE)
    if length <= 0:
        return rec
    flags = 0
    if not tcp_flags & 0x04:                    # RST clear: ParseTCPTimestamp (tcp_in.c:108-109)
        t = walk_ts(b, length)
        if t["nonterm"] or t["hi"] >= avail:
            flags |= TS_UNPINNED
        elif t["ret"]:
            rec["ts_val"], rec["ts_ref"] = t["ts_val"], t["ts_ref"]
            flags |= TS_FOUND
    if tcp_flags & 0x02:                        # SYN: ParseTCPOptions (tcp_in.c:72, :88)
        s = walk_syn(b, length)
        if s["nonterm"] or s["hi"] >= avail:
            flags |= SYN_UNPINNED
        else:
            rec["ts_recent"], rec["mss"], rec["wscale"] = s["ts_recent"], s["mss"], s["wscale"]
            flags |= s["flags"]
    rec["flags"] = flags
    return rec


def record_of_case(c, tcp_flags: int, avail: int) -> np.void:
    """expected_record from a FIXTURE case: the reference's own outputs, the
    restatement only for the highest index read and the endless walks."""
    rec = np.zeros((), dtype=TCPOPT_DTYPE)
    length, b = int(c["len"]), c["bytes"]
    if length <= 0:
        return rec
    flags = 0
    if not tcp_flags & 0x04:
        if (c["nonterm"] & 1) or walk_ts(b, length)["hi"] >= avail:
            flags |= TS_UNPINNED
        elif c["ts_ret"]:
            rec["ts_val"], rec["ts_ref"] = c["ts_val"], c["ts_ref"]
            flags |= TS_FOUND
    if tcp_flags & 0x02:
        s = walk_syn(b, length)
        if (c["nonterm"] & 2) or s["hi"] >= avail:
            flags |= SYN_UNPINNED
        else:
            rec["ts_recent"], rec["mss"], rec["wscale"] = c["ts_recent"], c["mss"], c["wscale"]
            flags |= int(c["seen"]) | (SACK_PERMIT if c["sack_permit"] else 0) | \
                     (SAW_TS if c["saw_timestamp"] else 0)
    rec["flags"] = flags
    return rec


# ---- the block generator ----------------------------------------------------
KINDS = (0, 1, 2, 3, 4, 5, 8, 6, 30, 254)
NATURAL = {2: 4, 3: 3, 4: 2, 5: 10, 8: 10, 6: 6, 30: 4, 254: 4}
LENGTHS = np.arange(0, 44, 4)
LENGTH_P = np.array([1, 1, 2, 12, 2, 2, 2, 1, 1, 1, 2], dtype=float)     # weighted to 12
LENGTH_P /= LENGTH_P.sum()


def gen_block(rng: np.random.Generator) -> tuple[int, np.ndarray]:
    """(len, BLOCK bytes): a sequence of options of KINDS with their natural
    lengths (about 15 % of the length bytes replaced by 0, 1, 2, 3, 255 or a
    random byte), random bytes mixed in, random bytes behind the block."""
    length = int(rng.choice(LENGTHS, p=LENGTH_P))
    b = rng.integers(0, 256, BLOCK, dtype=np.uint8)
    i = 0
    while i < length:
        u = rng.random()
        if u < 0.06:                             # a few random bytes, then options again
            i += int(rng.integers(1, 4))
            continue
        # NOPs pad as real stacks do; END is rare, or most blocks would end early
        kind = int(rng.choice(KINDS, p=(0.03, 0.30, 0.09, 0.09, 0.09, 0.05, 0.20, 0.05, 0.05, 0.05)))
        b[i] = kind
        i += 1
        if kind in (0, 1):
            continue
        optlen = NATURAL[kind]
        if rng.random() < 0.15:
            optlen = int(rng.choice((0, 1, 2, 3, 255, int(rng.integers(0, 256)))))
        if i < BLOCK:
            b[i] = optlen
        i += 1
        i += max(NATURAL[kind] - 2, 0)           # the option's data stays random
    return length, b


def gen_blocks(n: int, seed: int):
    rng = np.random.default_rng(seed)
    return [gen_block(rng) for _ in range(n)]


# ---- the live reference (oracle/_ref/libref_rx.so) ---------------------------
class RefWalks:
    """ParseTCPTimestamp / ParseTCPOptions of the reference itself, called on
    zeroed fake tcp_stream / tcp_send_vars / tcp_recv_vars buffers (x86-64
    offsets: stream rcvvar @48, sndvar @56, byte 34 bit 3 saw_timestamp, bit 4
    sack_permit, 72 B; send vars mss @2, eff_mss @4, wscale_peer @7, 176 B;
    recv vars ts_recent @24, ts_last_ts_upd @32, 96 B)."""

    CUR_TS = 0x5A5A1234

    def __init__(self):
        import oracle
        self.R = ctypes.CDLL(oracle.REF_LIB_PATH)
        vp = ctypes.c_void_p
        self.R.ParseTCPTimestamp.argtypes = [vp, vp, vp, ctypes.c_int]
        self.R.ParseTCPTimestamp.restype = ctypes.c_int
        self.R.ParseTCPOptions.argtypes = [vp, ctypes.c_uint32, vp, ctypes.c_int]
        self.R.ParseTCPOptions.restype = None
        self.stream = np.zeros(72, np.uint8)
        self.snd = np.zeros(176, np.uint8)
        self.rcv = np.zeros(96, np.uint8)
        self.ts = np.zeros(2, np.uint32)
        self.buf = np.zeros(BLOCK + 8, np.uint8)

    def ts_walk(self, b, length: int) -> dict:
        self.buf[:BLOCK] = b
        self.ts[:] = 0
        self.stream[:] = 0
        ret = self.R.ParseTCPTimestamp(self.stream.ctypes.data, self.ts.ctypes.data, self.buf.ctypes.data, length)
        return dict(ret=int(ret), ts_val=int(self.ts[0]), ts_ref=int(self.ts[1]))

    def syn_walk(self, b, length: int) -> dict:
        """The reference's outputs, and `seen`: MSS where it wrote mss (then
        (mss, eff_mss) != (0, 0): eff_mss = mss - 12), WSCALE where it wrote
        wscale_peer (the same value over a 0x00 and over a 0xFF prefill)."""
        r = self._syn_walk(b, length, 0x00)
        seen = MSS if (r["mss"], r["eff_mss"]) != (0, 0) else 0
        if self._syn_walk(b, length, 0xFF)["wscale"] == r["wscale"]:
            seen |= WSCALE
        r["seen"] = seen
        return r

    def _syn_walk(self, b, length: int, wscale_prefill: int) -> dict:
        self.buf[:BLOCK] = b
        self.stream[:] = 0
        self.snd[:] = 0
        self.snd[7] = wscale_prefill
        self.rcv[:] = 0
        self.stream[48:56].view(np.uint64)[0] = self.rcv.ctypes.data
        self.stream[56:64].view(np.uint64)[0] = self.snd.ctypes.data
        self.R.ParseTCPOptions(self.stream.ctypes.data, self.CUR_TS, self.buf.ctypes.data, length)
        saw = (int(self.stream[34]) >> 3) & 1
        assert int(self.rcv[32:36].view(np.uint32)[0]) == (self.CUR_TS if saw else 0)
        return dict(mss=int(self.snd[2:4].view(np.uint16)[0]), eff_mss=int(self.snd[4:6].view(np.uint16)[0]),
                    wscale=int(self.snd[7]), sack_permit=(int(self.stream[34]) >> 4) & 1, saw_timestamp=saw,
                    ts_recent=int(self.rcv[24:28].view(np.uint32)[0]))


TS_KEYS = ("ret", "ts_val", "ts_ref")
SYN_KEYS = ("mss", "eff_mss", "wscale", "sack_permit", "saw_timestamp", "ts_recent", "seen")


def load_fixture() -> np.ndarray:
    return np.fromfile(FIXTURE, dtype=CASE_DTYPE)


# ---- frames -------------------------------------------------------------------
def frame_raw(ihl: int, doff: int, tcp_flags: int, body: bytes, ip_len: int | None = None, seed: int = 0,
              eth_type: int = 0x0800) -> bytearray:
    """Ethernet + IPv4 (ihl words) + the 20 fixed TCP bytes (doff as given) +
    `body` (options and payload), check fields 0.  ip_len: tot_len, by
    default through the end of the frame."""
    rng = np.random.default_rng(seed)
    tot = 4 * ihl + 20 + len(body) if ip_len is None else ip_len
    f = bytearray(rng.integers(0, 256, 12, dtype=np.uint8).tobytes()) + bytes([eth_type >> 8, eth_type & 0xFF])
    ip = bytearray(4 * ihl)
    ip[0] = 0x40 | ihl
    ip[2], ip[3] = tot >> 8, tot & 0xFF
    ip[4:6] = rng.integers(0, 256, 2, dtype=np.uint8).tobytes()
    ip[6], ip[8], ip[9] = 0x40, 64, 6
    ip[12:20] = rng.integers(1, 255, 8, dtype=np.uint8).tobytes()
    ip[20:] = rng.integers(0, 256, 4 * ihl - 20, dtype=np.uint8).tobytes()
    tcp = bytearray(rng.integers(0, 256, 20, dtype=np.uint8).tobytes())
    tcp[12], tcp[13] = (doff << 4) & 0xF0, tcp_flags
    tcp[16:20] = b"\0\0\0\0"
    return f + ip + tcp + bytes(body)


def frame_bytes(block, length: int, trailing: bytes = b"", ihl: int = 5, tcp_flags: int = 0x10,
                ip_len: int | None = None, seed: int = 0) -> bytearray:
    """A frame whose TCP header carries block[0..length) as its options
    (doff = 5 + length / 4) with `trailing` behind them."""
    assert length % 4 == 0 and 0 <= length <= 40 and 5 <= ihl <= 15
    return frame_raw(ihl, 5 + length // 4, tcp_flags, bytes(bytearray(block[:length])) + bytes(trailing),
                     ip_len, seed)


DESC_DTYPE = np.dtype([("offset", "<u4"), ("len", "<u2"), ("flags", "u1"), ("rsvd", "u1")])


def pack_chunk(frames, starts=None, slot: int = 128, tail: int = 256, seed: int = 1):
    """(buf, desc) of a chunk holding `frames` at byte offsets `starts`
    (default: one `slot`-aligned slot each); the bytes between and behind the
    frames are random, so a read past a frame's end shows; buf is a multiple
    of 16 bytes with at least `tail` spare bytes; off_shift 0."""
    if starts is None:
        starts, pos = [], 0
        for f in frames:
            starts.append(pos)
            pos += (len(f) + slot - 1) // slot * slot
    end = max([s + len(f) for s, f in zip(starts, frames)] + [0])
    buf = np.random.default_rng(seed).integers(0, 256, (end + tail + 15) & ~15, dtype=np.uint8)
    desc = np.zeros(len(frames), dtype=DESC_DTYPE)
    for k, (s, f) in enumerate(zip(starts, frames)):
        buf[s:s + len(f)] = np.frombuffer(bytes(f), np.uint8)
        desc[k] = (s, len(f), 0, 0)
    return buf, desc


def fill_checksums(buf: np.ndarray, desc: np.ndarray) -> int:
    """Valid IP and TCP checksums for every well-formed frame: the oracle's tx
    fill (ip_out.c:164, tcp_out.c:329).  It leaves frames with doff < 5
    alone; those get the same two values from the oracle's ip_fast_csum and
    TCPCalcChecksum, frame by frame."""
    import oracle
    n = oracle.tx_fill(buf, np.ascontiguousarray(desc, dtype=oracle.DESC_DTYPE), 0)
    for d in desc:
        o, ln = int(d["offset"]), int(d["len"])
        f = buf[o:o + ln]
        if ln < 54 or bytes(f[12:14]) != b"\x08\x00" or (f[14] >> 4) != 4:
            continue
        ihl = int(f[14]) & 15
        t = 14 + 4 * ihl
        tot = (int(f[16]) << 8) | int(f[17])
        if ihl < 5 or t + 20 > ln or (int(f[t + 12]) >> 4) >= 5 or 14 + tot > ln or tot < 4 * ihl + 20:
            continue
        f[24:26] = 0
        f[24:26] = np.frombuffer(np.uint16(oracle.ip_fast_csum(bytes(f[14:t]), ihl)).tobytes(), np.uint8)
        f[t + 16:t + 18] = 0
        sa, da = (int(np.frombuffer(bytes(f[a:a + 4]), "<u4")[0]) for a in (26, 30))
        c = oracle.tcp_calc_checksum(bytes(f[t:14 + tot]), tot - 4 * ihl, sa, da)
        f[t + 16:t + 18] = np.frombuffer(np.uint16(c).tobytes(), np.uint8)
    return n
