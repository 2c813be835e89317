"""Data generation (include/mtcp_gpu_datagen.h) timed on the
device: one process, HIP events around windows of launches on one stream, the
median window per launch.

The batch is made at the call's input level (no frames, no walks in front): n
ACK records over n / 16 streams in random arrival order, the group arrays of
tests/group_model.py, every list walked to its end, every stream with eight
full segments buffered (mss 1460) in one payload arena.  Legs:

    open     every stream is on the send list and its window has room for two
             full segments (what an ACK that opens the window leaves): WINDOW
             with two segments out per stream
    rtx      no stream is on the list; one stream in 64 has a FAST_RTX record
             and sends two segments, the others are IDLE
    heavy    as open, with half the batch in ONE stream (the wave's fold), in
             windows of heavy_launches
    small    4 096 records as open, captured once as a graph and replayed

per leg:
    reset_us     the copies that put d_snd, d_tx and d_dtx back (in every
                 other figure; subtracted in the *_net figures)
    datagen_us   mtcp_gpu_datagen_dev: burst, row f8's launches, commit
    pattern_us   tools/datagen_pattern.hip's two kernels around the library's
                 own mtcp_gpu_tx_segment_dev on the same bursts: the same
                 loads and stores on the same grids without the fold, the
                 status chain and the commit arithmetic
    send_us      mtcp_gpu_data_send_dev: the same and the frame builder behind it

Correctness first: before anything is timed the call's bytes (d_seg, d_desc,
d_dres, d_total, d_snd, d_tx, d_dtx) are compared with tests/datagen_model.py,
for the whole batch up to --check-n records and, for a larger batch, for the
same leg at --check-n records in full and for the large batch's totals and a
sample of its streams.

    python tools/datagen_bench.py [--n 1048576] [--out profiles/datagen/bench_datagen.json]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mtcp_amd._types import (ACK_REC_DTYPE, ACK_STATE_DTYPE, ACKGEN_STATE_DTYPE, DATAGEN_RES_DTYPE,  # noqa: E402
                             DATAGEN_STATE_DTYPE, DESC_DTYPE, RCV_STATE_DTYPE, TX_BURST_DTYPE, TX_LINK_DTYPE,
                             TX_SEG_DTYPE)
from tests import datagen_model as dm  # noqa: E402
from tests import group_model as gm  # noqa: E402

CUR_TS = 0x12345678
MSS, SEG = 1460, 1448
SLOT = 1536


def make(n, per, kind, seed=7):
    """The call's inputs for n packets, `per` a stream."""
    rng = np.random.default_rng(seed)
    ns = n // per
    max_id = ns - 1
    owner = np.repeat(np.arange(ns, dtype=np.uint32), per)
    if kind == "heavy":
        owner[:n // 2] = 0
    perm = rng.permutation(n)
    sid = owner[perm]
    ack = np.zeros(n, dtype=ACK_REC_DTYPE)
    ack["verdict"], ack["flags"] = 12, 0x0001
    snd = np.zeros(ns, dtype=ACK_STATE_DTYPE)
    snd["sb_head_seq"] = rng.integers(0, 1 << 32, ns, dtype=np.uint64)
    snd["snd_nxt"] = snd["snd_una"] = snd["sb_head_seq"]
    snd["sb_len"], snd["sb_size"] = 8 * SEG, 1 << 16
    snd["cwnd"] = 2 * SEG + rng.integers(0, 1000, ns)
    snd["peer_wnd"] = 2 * SEG + rng.integers(0, 1000, ns)
    snd["mss"], snd["eff_mss"], snd["tcp_state"], snd["has_sndbuf"] = MSS, SEG, 4, 1
    snd["rto"] = rng.integers(1, 3000, ns)
    state = np.zeros(ns, dtype=RCV_STATE_DTYPE)
    for f in ("rcv_nxt", "ts_recent"):
        state[f] = rng.integers(0, 1 << 32, ns, dtype=np.uint64)
    state["rcv_wnd"], state["tcp_state"] = rng.integers(1 << 15, 1 << 22, ns), 4
    tx = np.zeros(ns, dtype=ACKGEN_STATE_DTYPE)
    for f in ("saddr", "daddr", "ts_lastack_sent"):
        tx[f] = rng.integers(0, 1 << 32, ns, dtype=np.uint64)
    for f in ("sport", "dport", "ip_id"):
        tx[f] = rng.integers(0, 1 << 16, ns)
    tx["wscale_mine"], tx["link"], tx["has_rcvbuf"], tx["ack_cnt"] = 7, rng.integers(0, 3, ns), 1, rng.integers(0, 4, ns)
    dtx = np.zeros(ns, dtype=DATAGEN_STATE_DTYPE)
    dtx["sb_off"] = 1 + np.arange(ns, dtype=np.uint64) * (8 * SEG + 2)
    dtx["sb_base_seq"] = snd["sb_head_seq"]
    if kind == "rtx":
        first = np.full(ns, -1, np.int64)
        first[sid[::-1]] = np.arange(n - 1, -1, -1)                        # each stream's first packet
        hit = np.arange(0, ns, 64)
        ack["flags"][first[hit]] |= dm.ACK_FAST_RTX
    else:
        dtx["on_send_list"] = 1
    return dict(n=n, max_id=max_id, sid=sid, ack=ack, state=state, snd=snd, tx=tx, dtx=dtx,
                payload_bytes=int(ns * (8 * SEG + 2) + 64))


def model_of(b, segs=None):
    """tests/datagen_model.py's answer for the batch, or for the segments `segs` of its table alone."""
    idx, seg_sid, seg_start = b["group"]
    ack, n = b["ack"], b["n"]
    if segs is not None:                                                   # their packets alone, renumbered
        lens = (seg_start[1:] - seg_start[:-1])[segs]
        pk = np.concatenate([idx[seg_start[j]:seg_start[j + 1]] for j in segs])
        ack, n, idx = ack[pk], len(pk), np.arange(len(pk), dtype=np.uint32)
        seg_sid, seg_start = seg_sid[segs], np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    stop = seg_start[1:]
    return dm.datagen(ack, stop, n, b["max_id"], idx, seg_sid, seg_start, len(seg_sid), stop, b["state"],
                      b["snd"], b["tx"], b["dtx"], CUR_TS, b["payload_bytes"], 3, 0, 1 << 40, 6, SLOT, b["seg_cap"])


def pattern_lib():
    P = ctypes.CDLL(os.path.join(ROOT, "tools", "libdatagen_pattern.so"))
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    P.datagen_pattern_burst.argtypes = [vp, vp, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    P.datagen_pattern_commit.argtypes = [u32, u32, vp, vp, vp, vp, vp, vp, vp, vp]
    P.datagen_pattern_offsets.argtypes = [u32, ctypes.POINTER(ctypes.c_uint64)]
    P.datagen_pattern_burst.restype = P.datagen_pattern_commit.restype = ctypes.c_int
    return P


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--per", type=int, default=16, help="packets per stream")
    ap.add_argument("--check-n", type=int, default=1 << 16, help="the largest batch checked in full against the model")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--launches", type=int, default=20, help="launches per timed window")
    ap.add_argument("--heavy-launches", type=int, default=2, help="launches per timed window of the heavy leg")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch

    from mtcp_amd import gpu
    P = pattern_lib()
    dev = torch.device("cuda", 0)
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    zeros = lambda k: torch.zeros(k, dtype=torch.uint8, device=dev)
    line = {"n": args.n, "per_stream": args.per, "slot_bytes": SLOT, "mss": MSS, "launches": args.launches,
            "heavy_launches": args.heavy_launches, "rounds": args.rounds, "check_n": args.check_n}
    st = torch.cuda.Stream(device=dev)
    h = st.cuda_stream
    links = np.zeros(3, dtype=TX_LINK_DTYPE)
    links["dst"][:, 0], links["src"][:, 0] = 2, 2

    def timed(leg, launches):
        times = []
        for _ in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(launches):
                leg()
            e1.record(st)
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3 / launches)
        times.sort()
        return round(times[len(times) // 2], 2), round((times[-1] - times[0]) / times[len(times) // 2], 3)

    class Leg:
        """One batch on the device and its legs."""

        def __init__(self, ctx, kind, n, with_image):
            self.ctx, self.kind = ctx, kind
            b = self.b = make(n, args.per, kind)
            b["group"] = idx, seg_sid, seg_start = gm.group(b["sid"], b["max_id"])
            self.m = m = len(seg_sid)
            self.cap = b["seg_cap"] = 2 * m + 8
            pad = lambda a, k: np.concatenate([a, np.zeros(k - len(a), np.uint32)]).astype(np.uint32)
            d = self.d = dict(ack=to_dev(b["ack"]), idx=to_dev(idx), sid=to_dev(pad(seg_sid, n)),
                              start=to_dev(pad(seg_start, n + 1)), nseg=to_dev(np.array([m], np.uint32)),
                              stop=to_dev(pad(seg_start[1:], n)), state=to_dev(b["state"]), links=to_dev(links))
            for k in ("snd", "tx", "dtx"):
                d[k], d[k + "0"] = to_dev(b[k]), to_dev(b[k])
            cap = self.cap
            self.seg, self.desc, self.dres, self.total = zeros(48 * cap), zeros(8 * cap), zeros(16 * n), zeros(16)
            self.status = zeros(cap)
            self.image = zeros(SLOT * cap) if with_image else None
            self.payload = torch.empty(b["payload_bytes"], dtype=torch.uint8, device=dev)
            self.work = zeros(gpu.Context.datagen_work_bytes(n, b["max_id"]))
            self.head = (d["ack"], d["stop"], n, b["max_id"], d["idx"], d["sid"], d["start"], d["nseg"], d["stop"],
                         d["state"], d["snd"], d["tx"], d["dtx"], CUR_TS)
            off = (ctypes.c_uint64 * 4)()
            P.datagen_pattern_offsets(n, off)
            self.off = [int(x) for x in off]

        def reset(self, suffix="0"):
            with torch.cuda.stream(st):
                for k in ("snd", "tx", "dtx"):
                    self.d[k].copy_(self.d[k + suffix], non_blocking=True)

        def gen(self):
            self.reset()
            self.ctx.datagen_dev(*self.head, self.b["payload_bytes"], 3, 0, SLOT * self.cap, 6, SLOT, self.seg, self.desc,
                                 self.cap, self.dres, self.total, self.work, stream=st)

        def send(self):
            self.reset()
            self.ctx.data_send_dev(*self.head, self.payload, self.d["links"], self.image, 0, 6, SLOT, self.seg, self.desc,
                                   self.cap, self.dres, self.total, self.status, self.work, stream=st)

        def pattern(self):
            d, b, n = self.d, self.b, self.b["n"]
            raw = lambda t_: ctypes.c_void_p(t_.data_ptr())
            self.reset("p")
            rc = P.datagen_pattern_burst(raw(d["ack"]), raw(d["stop"]), n, b["max_id"], raw(d["idx"]), raw(d["sid"]),
                                         raw(d["start"]), raw(d["nseg"]), raw(d["stop"]), raw(d["state"]), raw(d["snd"]),
                                         raw(d["tx"]), raw(d["dtx"]), raw(self.work), ctypes.c_void_p(h))
            self.ctx.tx_segment_dev(self.work[self.off[0]:self.off[1]], n, b["payload_bytes"], 3, 0, SLOT * self.cap, 6, SLOT,
                                    self.seg, self.desc, self.cap, self.work[self.off[1]:self.off[2]], self.total,
                                    self.work[self.off[3]:], stream=st)
            rc |= P.datagen_pattern_commit(n, b["max_id"], raw(d["sid"]), raw(d["nseg"]), raw(d["snd"]), raw(d["tx"]),
                                           raw(d["dtx"]), raw(self.dres), raw(self.work), ctypes.c_void_p(h))
            if rc != 0:
                raise SystemExit("the pattern kernels did not launch")

        def outputs(self):
            m = self.m
            return (self.seg.cpu().numpy().view(TX_SEG_DTYPE), self.desc.cpu().numpy().view(DESC_DTYPE),
                    self.dres.cpu().numpy().view(DATAGEN_RES_DTYPE)[:m], self.total.cpu().numpy().view(np.uint64),
                    self.d["snd"].cpu().numpy().view(ACK_STATE_DTYPE), self.d["tx"].cpu().numpy().view(ACKGEN_STATE_DTYPE),
                    self.d["dtx"].cpu().numpy().view(DATAGEN_STATE_DTYPE))

        def check(self, full):
            """The call's bytes against the model; then the pattern's records, made from the call's own bursts."""
            self.gen()
            st.synchronize()
            got = self.outputs()
            b, m = self.b, self.m
            names = ("seg", "desc", "dres", "total", "snd", "tx", "dtx")
            if full:
                for g, e, name in zip(got, model_of(b)[:7], names):
                    if g.tobytes() != e.tobytes():
                        raise SystemExit(f"{self.kind}, n {b['n']}: {name} differs from the model")
            else:
                segs = np.unique(np.concatenate([[0], np.random.default_rng(1).integers(0, m, 300)]))
                want = model_of(b, segs)
                ids = b["group"][1][segs]
                for k, name in ((4, "snd"), (5, "tx"), (6, "dtx")):
                    if got[k][ids].tobytes() != want[k][ids].tobytes():
                        raise SystemExit(f"{self.kind}: {name} of the sampled streams differs from the model")
                for f in ("n_seg", "bytes", "status", "stop", "flags"):
                    if not np.array_equal(got[2][segs][f], want[2][f]):
                        raise SystemExit(f"{self.kind}: dres.{f} of the sampled segments differs from the model")
                if int(got[3][0]) != int(got[2]["n_seg"].sum()) or int(got[3][0]) > self.cap:
                    raise SystemExit(f"{self.kind}: the totals are not consistent")
            T = int(got[3][0])
            bursts = self.work[self.off[0]:self.off[1]].cpu().numpy().view(TX_BURST_DTYPE)[:m]
            seg_sid = b["group"][1]
            ok = seg_sid <= b["max_id"]
            snd_p, dtx_p = b["snd"].copy(), b["dtx"].copy()
            ids = seg_sid[ok]
            snd_p["snd_nxt"][ids], snd_p["sb_len"][ids] = bursts["seq"][ok], bursts["len"][ok]
            snd_p["snd_una"][ids], snd_p["cwnd"][ids] = bursts["in_flight"][ok], bursts["window"][ok]
            snd_p["mss"][ids] = bursts["mss"][ok]
            dtx_p["sb_off"][ids] = bursts["payload_off"][ok]
            self.d["sndp"], self.d["txp"], self.d["dtxp"] = to_dev(snd_p), to_dev(b["tx"]), to_dev(dtx_p)
            self.pattern()
            st.synchronize()
            if int(self.total.cpu().numpy().view(np.uint64)[0]) != T:
                raise SystemExit(f"{self.kind}: the pattern's fan-out is not the call's")
            return T, np.bincount(got[2]["status"], minlength=12).tolist()

    with gpu.Context(0) as ctx:
        for kind in ("open", "rtx", "heavy"):
            if args.n > args.check_n:
                Leg(ctx, kind, args.check_n, False).check(True)            # the same leg, small enough to check in full
            leg = Leg(ctx, kind, args.n, True)
            T, status = leg.check(args.n <= args.check_n)
            name = kind + "_"
            line[name + "records"], line[name + "segments"], line[name + "status"] = T, leg.m, status
            launches = args.heavy_launches if kind == "heavy" else args.launches
            legs = {"reset_us": leg.reset, "datagen_us": leg.gen, "pattern_us": leg.pattern}
            if leg.image is not None:
                legs["send_us"] = leg.send
            for key, fn in legs.items():
                line[name + key], line[name + key + "_spread"] = timed(fn, launches)
            r = line[name + "reset_us"]
            line[name + "datagen_us_net"] = round(line[name + "datagen_us"] - r, 2)
            line[name + "pattern_us_net"] = round(line[name + "pattern_us"] - r, 2)
            line[name + "pattern_over_datagen"] = round(line[name + "pattern_us_net"] / line[name + "datagen_us_net"], 3)
            if "send_us" in legs:
                line[name + "send_us_net"] = round(line[name + "send_us"] - r, 2)
            del leg
            torch.cuda.empty_cache()
        # 4 096 records as one captured launch set
        leg = Leg(ctx, "open", 4096, True)
        T, status = leg.check(True)
        line["small_records"], line["small_segments"] = T, leg.m
        for key, fn in (("reset_us", leg.reset), ("datagen_us", leg.gen), ("pattern_us", leg.pattern), ("send_us", leg.send)):
            fn()
            st.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=st):
                fn()
            with torch.cuda.stream(st):
                line["small_" + key], line["small_" + key + "_spread"] = timed(graph.replay, args.launches)
            del graph
        r = line["small_reset_us"]
        for key in ("datagen_us", "pattern_us", "send_us"):
            line["small_" + key + "_net"] = round(line["small_" + key] - r, 2)
        line["small_pattern_over_datagen"] = round(line["small_pattern_us_net"] / line["small_datagen_us_net"], 3)
    print(json.dumps(line))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
