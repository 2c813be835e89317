"""Deterministic edge batches for the rx / tx kernels (tests/test_edge_frames.py
on the CPU, tests/test_gpu_edges.py on the GPU): frames placed on the kernels'
own structural boundaries instead of where a random draw happens to put them.

Every kernel walks a frame as 16 B chunks of the aligned grid, nch =
((p & 15) + len + 15) >> 4 of them, and changes its head / tail handling at
multiples of a granule: 4 chunks (a quad, rx_wave.hpp), 8 (oct), 16 (row), 64
(one wave load), 96 (rx_kernel's trip, kUnroll 6 x 16 lanes), 128 and 640 (the
wave kernel's 2- and 10-load trips) and 256 (the span kernel's window,
rx_span.hpp kStride).  The families:

  S, M, J  length sweeps (ihl 5, doff 5, no padding) at every even start phase
           p & 15: S every length 54..600; M windows around 768..1536 and
           2048, 3072, 4096 plus filler so that the average slot dispatches
           the 1 536 B / 2 048 B trips; J windows around the multiples of 256
           from 1792 to 4352 and around 8192, 10240, 12288, 20480
  Mt       M repeated until n > 65 536 (rx_kernel's unrolled schedule)
  H        ihl 5..15 x doff 5..15 x phase x payload length -1..33 (-1: a
           tot_len one short of the headers, TCP_LEN_BAD)
  P        Ethernet padding 0..40 B and a tot_len claiming 1..17 B more than
           the frame (TRUNCATED)
  I        ICMP datagrams of every length 0..70 and 1471..1481
  Z, Zf    frames whose correct iph->check and tcph->check are both 0x0000,
           and the same frames storing 0xFFFF in both fields
  D<s>     descriptor arithmetic at off_shift s: positions at and past 2^32,
           offset 0xFFFFFFFF, frames ending at and one byte past buf_len

Frame i starts at ((pos + 127) & ~127) + sh + 16 * k, pos being one byte past
the previous frame's end (so that at least one byte of garbage separates two
frames), sh the even phase under test and k = 0..7 derived from the frame's
index and length.  Every byte that is not a header field the case needs is
drawn from 1..254: a zero byte hides an over-read, and so does an 0xFF pair
(0xFFFF is the one's-complement zero).  For the same reason no run of 1..256
bytes just before a frame's start or just past its end may sum to a multiple
of 0xFFFF; the builder redraws the garbage byte next to the frame until that
holds.  Valid checksums come from the oracle's tx fill.

build(name) builds a family from scratch; get(name) returns one shared,
read-only copy.
"""
import functools

import numpy as np

import oracle
from mtcp_amd import DESC_DTYPE

PHASES = tuple(range(0, 16, 2))
WINDOWS = (1, 2, 4, 8, 16, 32, 64, 128, 256)
GRANULES = (4, 8, 16, 64, 96, 128, 256, 640)
LEAD = 256                      # garbage before the first frame and after the last
SHIFTS = (0, 1, 4, 6, 16)
FAMILIES = ("S", "M", "J", "Mt", "H", "P", "I", "Z", "Zf") + tuple(f"D{s}" for s in SHIFTS)


# ---- placement and garbage ---------------------------------------------------
def _starts(lens, shs, ks):
    starts = np.zeros(len(lens), np.int64)
    pos = LEAD
    for i in range(len(lens)):
        starts[i] = ((pos + 127) & ~127) + int(shs[i]) + 16 * int(ks[i])
        pos = int(starts[i]) + int(lens[i]) + 1
    return starts, ((pos + 127) & ~127) + LEAD


def window_sums(buf, at, k):
    """The checksum-style sum (little-endian 16-bit words, an odd last byte
    alone) of the k bytes from each position of `at`; -1 where the window
    leaves the buffer."""
    at = np.asarray(at, np.int64)
    inside = (at >= 0) & (at + k <= len(buf))
    base = np.where(inside, at, 0)
    w = np.where(np.arange(k) % 2 == 0, 1, 256).astype(np.int32)
    s = np.empty(len(at), np.int64)
    for lo in range(0, len(at), 8192):                  # blocks: the gather stays small
        idx = base[lo:lo + 8192, None] + np.arange(k)
        s[lo:lo + 8192] = (buf[idx].astype(np.int32) * w).sum(axis=1)
    return np.where(inside, s, -1)


def window_violations(buf, starts, lens):
    """(frame, side) of every frame with a run of k bytes just before its
    start (side 0) or just past its end (side 1) whose sum is a multiple of
    0xFFFF, k in WINDOWS."""
    starts = np.asarray(starts, np.int64)
    ends = starts + np.asarray(lens, np.int64)
    bad = []
    for k in WINDOWS:
        for side, at in ((0, starts - k), (1, ends)):
            s = window_sums(buf, at, k)
            bad += [(int(i), side) for i in np.nonzero((s >= 0) & (s % 0xFFFF == 0))[0]]
    return bad


def _settle_garbage(buf, starts, lens):
    """Step the garbage byte beside a frame (1..254, never a frame's byte)
    until no window of window_violations is left."""
    starts = np.asarray(starts, np.int64)
    ends = starts + np.asarray(lens, np.int64)
    for _ in range(64):
        bad = window_violations(buf, starts, lens)
        if not bad:
            return
        for i, side in bad:
            at = int(ends[i]) if side else int(starts[i]) - 1
            buf[at] = buf[at] % 254 + 1
    raise AssertionError("garbage windows did not settle")


def _ip_check(f, ihl):
    f[24:26] = 0
    c = oracle.ip_fast_csum(f[14:14 + 4 * ihl].tobytes(), ihl)
    f[24], f[25] = c & 0xFF, c >> 8


def _header(f, ihl, doff, tot_len, proto=6):
    f[12:14] = (0x08, 0x00)
    f[14] = 0x40 | ihl
    f[16:18] = (tot_len >> 8, tot_len & 0xFF)
    f[23] = proto
    T = 14 + 4 * ihl
    if proto == 6:
        f[T + 12] = (doff << 4) | (int(f[T + 12]) & 0x0F)
    _ip_check(f, ihl)


def _desc(starts, lens, off_shift=0):
    d = np.zeros(len(lens), dtype=DESC_DTYPE)
    d["offset"] = (np.asarray(starts, np.int64) >> off_shift).astype(np.uint32)
    d["len"] = np.asarray(lens).astype(np.uint16)
    return d


def _assemble(specs, seed):
    """specs: (len, sh, ihl, doff, tot_len, proto) per frame.  Garbage, headers,
    IP header checksums, then the oracle's tx fill for the TCP frames it takes."""
    rng = np.random.default_rng(seed)
    lens = np.array([s[0] for s in specs], np.int64)
    shs = np.array([s[1] for s in specs], np.int64)
    ks = (np.arange(len(specs)) * 5 + (lens >> 1)) & 7
    starts, size = _starts(lens, shs, ks)
    buf = rng.integers(1, 255, size, dtype=np.uint8)
    for (L, _, ihl, doff, tot_len, proto), o in zip(specs, starts):
        _header(buf[o:o + L], ihl, doff, tot_len, proto)
    desc = _desc(starts, lens)
    oracle.tx_fill(buf, desc, 0)
    return buf, desc


def _finish(buf, desc, off_shift=0):
    _settle_garbage(buf, desc["offset"].astype(np.int64) << off_shift, desc["len"])
    return buf, desc


def _plain(L, sh):
    return (L, sh, 5, 5, L - 14, 6)


def _window(centres, half=34):
    return sorted({L for c in centres for L in range(c - half, c + half + 1)})


# ---- the families --------------------------------------------------------------
def build_S():
    return _finish(*_assemble([_plain(L, sh) for L in range(54, 601) for sh in PHASES], 1001))


M_CENTRES = (768, 1024, 1280, 1536, 2048, 3072, 4096)
J_CENTRES = tuple(range(1792, 4353, 256)) + (8192, 10240, 12288, 20480)


def build_M():
    specs = [_plain(L, sh) for L in _window(M_CENTRES) for sh in PHASES]
    fresh = 1100
    while True:
        lens = np.array([s[0] for s in specs], np.int64)
        _, size = _starts(lens, [s[1] for s in specs], (np.arange(len(specs)) * 5 + (lens >> 1)) & 7)
        if size // len(specs) <= 1500:
            break
        # filler of 768..1280 B, a fresh seed per round, every phase in turn
        more = np.random.default_rng(fresh).integers(768, 1281, 512)
        specs += [_plain(int(L), PHASES[j % 8]) for j, L in enumerate(more)]
        fresh += 1
    return _finish(*_assemble(specs, 1002))


def build_J():
    return _finish(*_assemble([_plain(L, sh) for L in _window(J_CENTRES) for sh in PHASES], 1003))


def build_Mt():
    buf, desc = get("M")
    reps = 65536 // len(desc) + 1
    stride = len(buf)                               # a multiple of 128: phases and lines unchanged
    assert stride % 128 == 0
    tb = np.tile(buf, reps)
    td = np.tile(desc, reps)
    td["offset"] = (np.tile(desc["offset"].astype(np.int64), reps) +
                    np.repeat(np.arange(reps, dtype=np.int64) * stride, len(desc))).astype(np.uint32)
    return _finish(tb, td)


H_PAYLOADS = (-1, 0, 1, 2, 3, 15, 16, 17, 33)


def h_specs():
    return [(14 + 4 * (ihl + doff) + pl, sh, ihl, doff, 4 * (ihl + doff) + pl, 6)
            for ihl in range(5, 16) for doff in range(5, 16) for sh in PHASES for pl in H_PAYLOADS]


def build_H():
    return _finish(*_assemble(h_specs(), 1004))


P_LENGTHS = (60, 61, 62, 63, 64, 1514, 2046)


def p_specs():
    """(spec, pad): pad > 0 Ethernet padding, pad < 0 a tot_len claiming -pad bytes more."""
    out = []
    for L in P_LENGTHS:
        for sh in PHASES:
            out += [((L, sh, 5, 5, L - 14 - pad, 6), pad) for pad in range(0, 41)]
            out += [((L, sh, 5, 5, L - 14 + more, 6), -more) for more in range(1, 18)]
    return out


def build_P():
    return _finish(*_assemble([s for s, _ in p_specs()], 1005))


I_LENGTHS = tuple(range(0, 71)) + tuple(range(1471, 1482))


def i_specs():
    """(spec, claims_more)."""
    out = []
    for ihl in (5, 6):
        for dl in I_LENGTHS:
            out += [((14 + 4 * ihl + dl, sh, ihl, 0, 4 * ihl + dl, 1), False) for sh in PHASES]
        for j, (dl, more) in enumerate(((0, 1), (8, 1), (33, 5), (64, 17), (1472, 2), (1481, 17))):
            out.append(((14 + 4 * ihl + dl, PHASES[(j + ihl) % 8], ihl, 0, 4 * ihl + dl + more, 1), True))
    return out


def build_I():
    return _finish(*_assemble([s for s, _ in i_specs()], 1006))


Z_LENGTHS = (60, 1514, 2050)


def _oc_add(a, b):
    s = a + b
    return (s & 0xFFFF) + (s >> 16)


def _z_raw():
    buf, desc = _assemble([_plain(L, PHASES[j % 8]) for L in Z_LENGTHS for j in range(64)], 1007)
    for o in desc["offset"].astype(np.int64):
        f = buf[o:o + 56]
        # one's-complement add each filled check into a word its sum covers
        # (the IP id, the first payload word): the rest then sums to 0xFFFF
        for word, check in ((18, 24), (54, 50)):
            v = _oc_add(int(f[word]) | int(f[word + 1]) << 8, int(f[check]) | int(f[check + 1]) << 8)
            f[word], f[word + 1] = v & 0xFF, v >> 8
    assert oracle.tx_fill(buf, desc, 0) == len(desc)
    for o in desc["offset"].astype(np.int64):
        assert not buf[o + 24:o + 26].any() and not buf[o + 50:o + 52].any(), "check fields must fill to 0x0000"
    return buf, desc


def build_Z():
    return _finish(*_z_raw())


def build_Zf():
    buf, desc = _z_raw()
    for o in desc["offset"].astype(np.int64):
        buf[o + 24:o + 26] = 0xFF
        buf[o + 50:o + 52] = 0xFF
    return _finish(buf, desc)


D_LENGTHS = (60, 1000, 590, 54, 777, 128, 1001)      # each shorter than a 1 KiB slot
# (the device entry points take a buf_len that is a multiple of 16: include/mtcp_gpu.h)
D_LAST = {0: 960, 1: 960, 4: 960, 6: 960, 16: 60000}
D_CASES = ("at 2^32", "at 2^32 + one slot", "offset 0xFFFFFFFF", "one byte past buf_len",
           "length 0 at buf_len", "length 60 at buf_len", "length 13 at 0", "odd start")


def build_D(s):
    """-> (buf, desc, n_valid, cases): the valid frames' descriptors, then one
    per case of `cases` (names from D_CASES).  Every out-of-range byte position,
    truncated to 32 bits, is the start of a valid frame of the buffer (or, for
    offset 0xFFFFFFFF, still far past it): a kernel that truncates answers
    TCP_OK, which fails the comparison, and reads nothing outside the buffer."""
    rng = np.random.default_rng(1010 + s)
    slot = 1 << 16 if s == 16 else 1024
    lens = np.array(D_LENGTHS + (D_LAST[s],), np.int64)
    if s == 16:
        lens[1], lens[4] = 9000, 40000
    nv = len(lens)
    starts = np.arange(nv, dtype=np.int64) * slot
    buf_len = int(starts[-1] + lens[-1])                 # the last frame ends exactly at buf_len
    buf = rng.integers(1, 255, buf_len, dtype=np.uint8)
    for o, L in zip(starts, lens):
        _header(buf[o:o + L], 5, 5, int(L) - 14, 6)
    valid = _desc(starts, lens, s)
    assert oracle.tx_fill(buf, valid, s) == nv
    at_end = -(-buf_len >> s)                            # buf_len itself where 2^s divides it
    extra = []
    if s:
        extra += [("at 2^32", 1 << (32 - s), 60), ("at 2^32 + one slot", (1 << (32 - s)) + (slot >> s), int(lens[1]))]
    extra += [("offset 0xFFFFFFFF", 0xFFFFFFFF, 60),
              ("one byte past buf_len", int(starts[-1]) >> s, int(lens[-1]) + 1),
              ("length 0 at buf_len", at_end, 0), ("length 60 at buf_len", at_end, 60),
              ("length 13 at 0", 0, 13)]
    if s == 0:
        extra.append(("odd start", int(starts[2]) + 1, 60))
    d = np.zeros(len(extra), DESC_DTYPE)
    d["offset"] = [e[1] for e in extra]
    d["len"] = [e[2] for e in extra]
    _settle_garbage(buf, starts, lens)
    return buf, np.concatenate([valid, d]), nv, tuple(e[0] for e in extra)


_BUILDERS = {"S": build_S, "M": build_M, "J": build_J, "Mt": build_Mt, "H": build_H, "P": build_P,
             "I": build_I, "Z": build_Z, "Zf": build_Zf}
_BUILDERS.update({f"D{s}": functools.partial(build_D, s) for s in SHIFTS})


def build(name):
    return _BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def get(name):
    out = build(name)
    for a in out[:2]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_rx(name, rss_queues=8):
    """The oracle's records of a family (RSS: key 0x05.., `rss_queues` queues,
    endian check on; 0: no RSS), computed once."""
    buf, desc = get(name)[:2]
    shift = int(name[1:]) if name[0] == "D" else 0
    out = oracle.rx_chunk(buf, desc, shift, oracle.rss_cfg(None, rss_queues, 1) if rss_queues else None)
    out.setflags(write=False)
    return out


def nch_of(desc):
    """Chunks of the 16 B grid each frame touches (rx_wave.hpp: nch), and its phase p & 15."""
    p = desc["offset"].astype(np.int64)
    sh = p & 15
    return (sh + desc["len"].astype(np.int64) + 15) >> 4, sh
