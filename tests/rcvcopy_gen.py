"""Batches for the receive copy (include/mtcp_gpu_rcvcopy.h) with hand-written
records: what tests/test_rcvcopy_model.py feeds the host-compiled plan and
tests/test_gpu_rcvcopy.py the kernels.  The expectation of every batch is
tests/rcvcopy_model.py's copy().

A batch is a dict: buf, desc, off_shift, res, place, sid, max_id, group (idx,
seg_sid, seg_start as tests/group_model.py writes them), seg_stop, rbuf, arena.
Receive buffers in the arena are separated by guard bands of at least 64 B of
GUARD; the chunks hold random bytes, so stale bytes matter.
"""
import numpy as np

from mtcp_amd._types import DESC_DTYPE, RCV_BUF_DTYPE, RCV_COPY, RCV_PLACE_DTYPE, RESULT_DTYPE
from tests import group_model as gm

GUARD = 0x5A
PUT_STORED = 15


def arena_for(rng, sizes, aligns=None):
    """(arena, data offsets): chunk k of sizes[k] bytes at an offset that is
    aligns[k] mod 16 (random if None), 64-79 B of GUARD around each."""
    offs, pos = [], 64
    for k, size in enumerate(sizes):
        a = int(rng.integers(0, 16)) if aligns is None or aligns[k] is None else aligns[k]
        d0 = pos + ((a - pos) & 15)
        offs.append(d0)
        pos = d0 + size + 64
    arena = np.full((pos + 15) & ~15, GUARD, np.uint8)
    for d0, size in zip(offs, sizes):
        arena[d0:d0 + size] = rng.integers(0, 256, size, dtype=np.uint8)
    return arena, offs


def finish(b):
    b["group"] = gm.group(b["sid"], b["max_id"])
    idx, seg_sid, seg_start = b["group"]
    stop = seg_start[1:].copy()
    stop[seg_sid > b["max_id"]] = seg_start[:-1][seg_sid > b["max_id"]]
    b.setdefault("seg_stop", stop)
    return b


def build(rng, streams, width=8, absent=2):
    """streams: dicts with size, head, last, pkts = [(put_off, len, source
    alignment 0-15 or None)] in list order, and optionally align (of data_off).
    width: the group width the batch is to get (the average slot is steered:
    filler packets without COPY for 8, spare bytes behind the chunk for 32)."""
    ns = len(streams)
    max_id = ns - 1 + absent
    sizes = [s["size"] for s in streams] + [64] * absent
    arena, offs = arena_for(rng, sizes, [s.get("align") for s in streams] + [None] * absent)
    rbuf = np.zeros(max_id + 1, RCV_BUF_DTYPE)
    for k in range(max_id + 1):
        head, last = (streams[k]["head"], streams[k]["last"]) if k < ns else (3, 9)
        rbuf[k] = (offs[k], sizes[k], head, head + last, last, (0, 0))
    keys = np.concatenate([np.sort(rng.random(len(s["pkts"]))) for s in streams] + [np.zeros(0)])
    owner = np.concatenate([np.full(len(s["pkts"]), k, np.int64) for k, s in enumerate(streams)] + [np.zeros(0, np.int64)])
    which = np.concatenate([np.arange(len(s["pkts"])) for s in streams] + [np.zeros(0, np.int64)]).astype(np.int64)
    order = np.argsort(keys, kind="stable")
    n = len(order)
    sid = owner[order].astype(np.uint32)
    res, place, desc = np.zeros(n, RESULT_DTYPE), np.zeros(n, RCV_PLACE_DTYPE), np.zeros(n, DESC_DTYPE)
    pos = 0
    for p in range(n):
        off, ln, sa = streams[int(owner[order[p]])]["pkts"][int(which[order[p]])]
        doff = int(rng.integers(5, 16))
        hdr = 14 + 4 * (5 + doff)
        sa = int(rng.integers(0, 16)) if sa is None else sa
        at = pos + ((sa - hdr - pos) & 15)
        flen = hdr + ln + int(rng.integers(0, 4))
        desc[p] = (at, flen, 0, 0)
        res["payload_len"][p], res["ihl_doff"][p] = ln, 5 | doff << 4
        place[p] = (off, 0, 0, ln, PUT_STORED, RCV_COPY | (int(rng.integers(0, 16)) << 1))
        pos = (at + flen + 15) & ~15
    if width == 8 and n:                                   # filler frames of 64 B, MISS, until the average slot is 512 B
        extra = max(0, -(-(pos + 256) // 448) - n)
        sid = np.concatenate([sid, np.full(extra, gm.FLOW_MISS, np.uint32)])
        res, place = np.concatenate([res, np.zeros(extra, RESULT_DTYPE)]), np.concatenate([place, np.zeros(extra, RCV_PLACE_DTYPE)])
        fill = np.zeros(extra, DESC_DTYPE)
        fill["offset"], fill["len"] = pos + 64 * np.arange(extra), 60
        desc = np.concatenate([desc, fill])
        pos += 64 * extra
        n += extra
    blen = (pos + 256 + 15) & ~15
    if width == 32:
        blen = max(blen, (513 * n + 15) & ~15)
    buf = rng.integers(0, 256, blen, dtype=np.uint8)
    return finish({"buf": buf, "desc": desc, "off_shift": 0, "res": res, "place": place, "sid": sid, "max_id": max_id,
                   "rbuf": rbuf, "arena": arena, "width": width})


def random_batch(rng, nstreams, garbage=False):
    """Lists of 0-90 packets, every status byte reachable: BAD records, ranges
    past the buffer, every BAD_SRC cause, deferrals inside a list.  With
    `garbage`, random bytes in the placement records and in the buffer records
    (half of them keep their chunk and get consistent random offsets, the
    others are random through and through), with valid group arrays."""
    lens = [int(rng.integers(0, 91)) if rng.random() < 0.2 else int(rng.integers(0, 8)) for _ in range(nstreams)]
    max_id = nstreams + 3
    sid = np.concatenate([np.full(k, s, np.uint32) for s, k in enumerate(lens)] + [np.full(5, gm.FLOW_MISS, np.uint32)])
    sid = sid[rng.permutation(len(sid))]
    n = len(sid)
    sizes = [int(rng.choice([64, 256, 1000])) for _ in range(max_id + 1)]
    arena, offs = arena_for(rng, sizes)
    rbuf = np.zeros(max_id + 1, RCV_BUF_DTYPE)
    for s in range(max_id + 1):
        head = int(rng.integers(0, sizes[s] + 1)) if rng.random() < 0.7 else 0
        last = int(rng.integers(0, sizes[s] - head + 1))
        rbuf[s] = (offs[s], sizes[s], head, head + last, last, (0, 0))
    bad = rng.random(max_id + 1)
    rbuf["rsvd"][bad < 0.03, 1] = 1
    rbuf["size"][(bad >= 0.03) & (bad < 0.05)] = 0
    rbuf["last_len"][(bad >= 0.05) & (bad < 0.08)] += 1
    rbuf["data_off"][(bad >= 0.08) & (bad < 0.10)] = len(arena)
    place, res, desc = np.zeros(n, RCV_PLACE_DTYPE), np.zeros(n, RESULT_DTYPE), np.zeros(n, DESC_DTYPE)
    for p in range(n):
        s = int(sid[p])
        size = sizes[s] if s <= max_id else 64
        ln = int(rng.integers(1, 61))
        place[p] = (int(rng.integers(0, max(size - ln, 0) + 1)), 0, 0, ln, PUT_STORED, RCV_COPY if rng.random() < 0.9 else 0)
        res["payload_len"][p], res["ihl_doff"][p] = ln, 5 | int(rng.integers(5, 16)) << 4
        desc[p] = (p * 3, 14 + 4 * (5 + (int(res["ihl_doff"][p]) >> 4)) + ln, 0, 0)     # off_shift 6: 192 B slots
    r = rng.random(n)
    place["put_off"][r < 0.04] += 1000                                    # BAD_RANGE
    res["payload_len"][(r >= 0.04) & (r < 0.06)] += 1                     # BAD_SRC: the lengths differ
    desc["len"][(r >= 0.06) & (r < 0.08)] -= 1                            # BAD_SRC: the payload leaves the frame
    desc["offset"][(r >= 0.08) & (r < 0.10)] = 3 * n                      # BAD_SRC: the descriptor leaves the chunk
    if garbage:
        keep = rng.random(max_id + 1) < 0.5
        junk = rng.integers(0, 256, rbuf.nbytes, dtype=np.uint8).view(RCV_BUF_DTYPE).copy()
        junk["data_off"] %= np.uint64(2 * len(arena))
        junk["size"] >>= rng.integers(0, 32, max_id + 1).astype(np.uint32)
        for f in ("data_off", "size"):
            junk[f][keep] = rbuf[f][keep]
        junk["rsvd"][keep] = 0
        junk["tail_offset"][keep] %= junk["size"][keep] + np.uint32(1)
        junk["head_offset"][keep] %= junk["tail_offset"][keep] + np.uint32(1)
        junk["last_len"][keep] = junk["tail_offset"][keep] - junk["head_offset"][keep]
        rbuf = junk
        place = rng.integers(0, 256, place.nbytes, dtype=np.uint8).view(RCV_PLACE_DTYPE).copy()
        place["put_off"] >>= rng.integers(0, 32, n).astype(np.uint32)
        place["put_len"] = np.where(rng.random(n) < 0.5, res["payload_len"], place["put_len"])
    b = {"buf": rng.integers(0, 256, 192 * n, dtype=np.uint8), "desc": desc, "off_shift": 6, "res": res,
         "place": place, "sid": sid, "max_id": max_id, "rbuf": rbuf, "arena": arena, "width": 8}
    b["group"] = gm.group(sid, max_id)
    idx, seg_sid, seg_start = b["group"]
    stop = seg_start[1:].copy()
    cut = rng.random(len(stop)) < 0.2                                     # a deferral somewhere in the list
    stop[cut] = seg_start[:-1][cut] + (rng.random(cut.sum()) * (stop[cut] - seg_start[:-1][cut])).astype(np.uint32)
    b["seg_stop"] = stop
    return finish(b)
