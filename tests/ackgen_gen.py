"""Batches for the ACK generation tests (include/mtcp_gpu_ackgen.h), at the
level of the call's inputs: placement records carrying ACK flags and verdicts,
the group arrays of tests/group_model.py over the packets' stream ids, the two
stop arrays, the walks' states and the tx records.  A stream is a dict:

    len      packets of the stream in the batch
    flags    "now" | "agg" | "none" | "mixed" | an array of placement flag bytes
    put      True: the first packet's verdict is PUT_STORED (else SEQ_* / ACK_ONLY)
    defer    None | ("seg", k) | ("ack", k): the stop array that ends k packets in
    tx       overrides of the stream's tx record
    state    overrides of its receive state
"""
import numpy as np

from mtcp_amd._types import ACK_STATE_DTYPE, RCV_PLACE_DTYPE, RCV_STATE_DTYPE
from tests import ackgen_model as am
from tests import group_model as gm

NOW, AGG = am.RCV_ACK_NOW, am.RCV_ACK_AGGREGATE
ROOMY = dict(buf_off=0, buf_len=1 << 40, off_shift=0, slot_bytes=0)


def flags_of(spec, k: int, rng) -> np.ndarray:
    if isinstance(spec, str):
        if spec == "now":
            return np.full(k, NOW, np.uint8)
        if spec == "agg":
            return np.full(k, AGG, np.uint8)
        if spec == "none":
            return np.zeros(k, np.uint8)
        assert spec == "mixed"
        return rng.choice(np.array([0, NOW, AGG, 0x01 | AGG, 0x08 | AGG], np.uint8), size=k, p=[.2, .35, .25, .1, .1])
    a = np.asarray(spec, dtype=np.uint8)
    assert len(a) == k
    return a


def make(streams, seed=1, max_id=None, n_miss=0, n_none=0, with_ack_stop=True, n_links=3, seg_cap=None, **room):
    rng = np.random.default_rng(seed)
    S = len(streams)
    max_id = max(2 * S, 7) if max_id is None else max_id
    ids = rng.choice(max_id + 1, size=S, replace=False).astype(np.uint32)
    sid = np.concatenate([np.full(int(s["len"]), ids[i], np.uint32) for i, s in enumerate(streams)] +
                         [np.full(n_miss, gm.FLOW_MISS, np.uint32), np.full(n_none, gm.FLOW_NONE, np.uint32)])
    sid = sid[rng.permutation(len(sid))]
    n = len(sid)
    place = np.zeros(n, dtype=RCV_PLACE_DTYPE)
    state = np.zeros(max_id + 1, dtype=RCV_STATE_DTYPE)
    state["head_seq"] = rng.integers(0, 1 << 32, max_id + 1, dtype=np.uint64)
    state["merged_len"] = rng.integers(0, 1 << 16, max_id + 1)
    state["rcv_nxt"] = state["head_seq"] + state["merged_len"]
    state["rcv_wnd"] = rng.integers(1, 1 << 22, max_id + 1)
    state["size"] = 1 << 22
    state["ts_recent"] = rng.integers(0, 1 << 32, max_id + 1, dtype=np.uint64)
    state["tcp_state"] = am.ST_ESTABLISHED
    snd = np.frombuffer(rng.bytes(128 * (max_id + 1)), dtype=ACK_STATE_DTYPE).copy()
    tx = np.zeros(max_id + 1, dtype=am.STATE_DTYPE)
    for f in ("saddr", "daddr"):
        tx[f] = rng.integers(0, 1 << 32, max_id + 1, dtype=np.uint64)
    for f in ("sport", "dport", "ip_id"):
        tx[f] = rng.integers(0, 1 << 16, max_id + 1)
    tx["wscale_mine"] = rng.integers(0, 15, max_id + 1)
    tx["link"] = rng.integers(0, n_links, max_id + 1)
    tx["has_rcvbuf"] = 1
    tx["ts_lastack_sent"] = rng.integers(0, 1 << 32, max_id + 1, dtype=np.uint64)
    idx, seg_sid, seg_start = gm.group(sid, max_id)
    m = len(seg_sid)
    seg_stop = seg_start[1:].copy()
    seg_stop[seg_sid > max_id] = seg_start[:-1][seg_sid > max_id]        # MISS, NONE: their start
    ack_stop = seg_stop.copy()
    seg_of = {int(s): j for j, s in enumerate(seg_sid)}
    for i, s in enumerate(streams):
        k = int(s["len"])
        for f, v in s.get("tx", {}).items():
            tx[ids[i]][f] = v
        for f, v in s.get("state", {}).items():
            state[ids[i]][f] = v
        if k == 0:
            continue
        at = np.nonzero(sid == ids[i])[0]                                # arrival order: the list's order
        fl = flags_of(s.get("flags", "mixed"), k, rng)
        place["flags"][at] = fl
        place["verdict"][at] = np.where(fl & NOW, 11, np.where(fl & AGG, 10, 12))
        place["verdict"][at[(fl & 0x01) != 0]] = 15
        if s.get("put"):
            place["verdict"][at[0]] = 15
        j = seg_of[int(ids[i])]
        if s.get("defer"):
            which, cut = s["defer"]
            stop = int(seg_start[j]) + cut
            assert stop < seg_start[j + 1]
            if which == "seg":
                seg_stop[j] = stop
                ack_stop[j] = stop
                place["flags"][at[cut:]], place["verdict"][at[cut:]] = 0, 6   # DEFER_BEHIND
                place["verdict"][at[cut]] = 3                                  # DEFER_FLAGS
            else:
                ack_stop[j] = stop
    b = dict(place=place, n=n, max_id=max_id, sid=sid, ids=ids, group=(idx, seg_sid, seg_start), seg_stop=seg_stop,
             ack_stop=ack_stop if with_ack_stop else None, state=state, snd=snd, tx=tx, n_links=n_links,
             cur_ts=int(rng.integers(0, 1 << 32)), seg_cap=seg_cap if seg_cap is not None else 64 * max(m, 1) + 3)
    b.update(ROOMY)
    b.update(room)
    return b


def expect(b, nseg=None):
    idx, seg_sid, seg_start = b["group"]
    return am.ackgen(b["place"], b["n"], b["max_id"], idx, seg_sid, seg_start,
                     len(seg_sid) if nseg is None else nseg, b["seg_stop"], b["ack_stop"], b["state"], b["snd"],
                     b["cur_ts"], b["tx"], b["n_links"], b["buf_off"], b["buf_len"], b["off_shift"],
                     b["slot_bytes"], b["seg_cap"])
