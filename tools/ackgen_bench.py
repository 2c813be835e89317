"""ACK generation (include/mtcp_gpu_ackgen.h) timed on the
device: one process, HIP events around windows of launches on one stream, the
median window per launch.

The batch is made at the call's input level (no frames, no walks in front):
n placement records over n / 16 streams in random arrival order, every packet
with an EnqueueACK flag (two ACK_OPT_NOW per stream, the rest
ACK_OPT_AGGREGATE, a PUT_STORED verdict with the latter), the group arrays of
tests/group_model.py, every list walked to its end.  Legs:

    reset_us     the copy that puts d_tx back (in every other leg; subtracted
                 in the *_net figures)
    ackgen_us    mtcp_gpu_ackgen_dev: plan, scan, emit and commit
    pattern_us   tools/ackgen_pattern.hip: the same three launches on the same
                 grids with the same loads and stores and none of the fold,
                 plan, record or commit arithmetic; its d_tx holds each
                 stream's emitted count, so the fan-out is the call's own
    send_us      mtcp_gpu_ack_send_dev: the same and the frame builder behind it
    heavy_*      ackgen and pattern with half the batch in ONE stream (the
                 wave's cooperative fold), in windows of heavy_launches
    sweep        a batch of mid-length lists (--mid-per packets a stream on
                 average, 8 to 2 * mid_per - 8 each) through the library's launches
                 with the plan kernel's lane threshold 4 .. 128
                 (ackgen_variant_launch), net of the reset

Correctness first: the totals and a sample of streams are checked against
tests/ackgen_model.py's per-case form before anything is printed, and every
sweep variant must give the library's bytes.

    python tools/ackgen_bench.py [--n 1048576] [--out profiles/ackgen/bench_ackgen.json]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mtcp_amd._types import (ACK_STATE_DTYPE, ACKGEN_RES_DTYPE, ACKGEN_STATE_DTYPE, RCV_PLACE_DTYPE,  # noqa: E402
                             RCV_STATE_DTYPE, TX_LINK_DTYPE)
from tests import ackgen_model as am  # noqa: E402
from tests import group_model as gm  # noqa: E402

CUR_TS = 0x12345678
SLOT = 128


def make(n, per, kind, seed=7):
    """(place, sid, max_id, state, snd, tx): n packets, `per` a stream on
    average.  kind "even": `per` each; "heavy": the first half of the packets
    belongs to stream 0; "mid": 8 to 2 * per - 8 packets a stream."""
    rng = np.random.default_rng(seed)
    ns = n // per
    max_id = ns - 1
    if kind == "mid":
        lens = rng.integers(8, 2 * per - 7, ns)
        owner = np.repeat(np.arange(ns, dtype=np.uint32), lens)[:n]
        owner = np.concatenate([owner, np.full(n - len(owner), ns - 1, np.uint32)])
    else:
        owner = np.repeat(np.arange(ns, dtype=np.uint32), per)
        if kind == "heavy":
            owner[:n // 2] = 0
    sid = owner[rng.permutation(n)]
    place = np.zeros(n, dtype=RCV_PLACE_DTYPE)
    now = rng.random(n) < 2.0 / per
    place["flags"] = np.where(now, am.RCV_ACK_NOW, am.RCV_ACK_AGGREGATE | 0x01)
    place["verdict"] = np.where(now, 11, 15)
    state = np.zeros(ns, dtype=RCV_STATE_DTYPE)
    state["head_seq"] = rng.integers(0, 1 << 32, ns, dtype=np.uint64)
    state["merged_len"] = rng.integers(0, 1 << 16, ns)
    state["rcv_nxt"] = state["head_seq"] + state["merged_len"]
    state["rcv_wnd"] = rng.integers(1, 1 << 22, ns)
    state["ts_recent"] = rng.integers(0, 1 << 32, ns, dtype=np.uint64)
    state["tcp_state"] = am.ST_ESTABLISHED
    snd = np.zeros(ns, dtype=ACK_STATE_DTYPE)
    snd["snd_nxt"] = rng.integers(0, 1 << 32, ns, dtype=np.uint64)
    tx = np.zeros(ns, dtype=ACKGEN_STATE_DTYPE)
    for f in ("saddr", "daddr"):
        tx[f] = rng.integers(0, 1 << 32, ns, dtype=np.uint64)
    for f in ("sport", "dport", "ip_id"):
        tx[f] = rng.integers(0, 1 << 16, ns)
    tx["wscale_mine"], tx["link"], tx["has_rcvbuf"] = 7, rng.integers(0, 3, ns), 1
    return place, sid, max_id, state, snd, tx


def pattern_lib():
    P = ctypes.CDLL(os.path.join(ROOT, "tools", "libackgen_pattern.so"))
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    tail = [vp, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, u32, vp, vp, vp, vp]
    P.ackgen_pattern_launch.argtypes, P.ackgen_pattern_launch.restype = tail, ctypes.c_int
    P.ackgen_variant_launch.argtypes, P.ackgen_variant_launch.restype = [u32] + tail, ctypes.c_int
    return P


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--per", type=int, default=16, help="packets per stream")
    ap.add_argument("--mid-per", type=int, default=36, help="packets per stream of the sweep's batch, on average")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--launches", type=int, default=20, help="launches per timed window")
    ap.add_argument("--heavy-launches", type=int, default=2, help="launches per timed window of the heavy legs")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch

    from mtcp_amd import gpu
    P = pattern_lib()
    dev = torch.device("cuda", 0)
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    zeros = lambda k: torch.zeros(k, dtype=torch.uint8, device=dev)
    n = args.n
    line = {"n": n, "per_stream": args.per, "slot_bytes": SLOT, "launches": args.launches,
            "heavy_launches": args.heavy_launches, "rounds": args.rounds}
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

    with gpu.Context(0) as ctx:
        for name, kind, per in (("", "even", args.per), ("heavy_", "heavy", args.per), ("mid_", "mid", args.mid_per)):
            place, sid, max_id, state, snd, tx = make(n, per, kind)
            idx, seg_sid, seg_start = gm.group(sid, max_id)
            m = len(seg_sid)
            pad = lambda a, k: np.concatenate([a, np.zeros(k - len(a), np.uint32)]).astype(np.uint32)
            # every stream plans at most its NOWs + 1 records
            nows = np.bincount(sid[place["flags"] == am.RCV_ACK_NOW], minlength=max_id + 1)
            cap = int(np.minimum(nows + 1, 63).sum())
            d = dict(place=to_dev(place), idx=to_dev(idx), sid=to_dev(pad(seg_sid, n)), start=to_dev(pad(seg_start, n + 1)),
                     nseg=to_dev(np.array([m], np.uint32)), stop=to_dev(pad(seg_start[1:], n)), state=to_dev(state),
                     snd=to_dev(snd), tx0=to_dev(tx), tx=to_dev(tx), links=to_dev(links))
            seg, desc, ares, total = zeros(48 * cap), zeros(8 * cap), zeros(16 * n), zeros(16)
            status, image = zeros(cap), zeros(SLOT * cap)
            work = zeros(gpu.Context.ackgen_work_bytes(n, max_id))
            head = (d["place"], n, max_id, d["idx"], d["sid"], d["start"], d["nseg"], d["stop"], d["stop"], d["state"],
                    d["snd"], CUR_TS, d["tx"])
            raw = lambda t_: ctypes.c_void_p(t_.data_ptr())
            tail = (raw(d["place"]), n, max_id, raw(d["idx"]), raw(d["sid"]), raw(d["start"]), raw(d["nseg"]),
                    raw(d["stop"]), raw(d["stop"]), raw(d["state"]), raw(d["snd"]), raw(d["tx"]), raw(seg), raw(desc), cap,
                    raw(ares), raw(total), raw(work), ctypes.c_void_p(h))

            def reset(src="tx0"):
                with torch.cuda.stream(st):
                    d["tx"].copy_(d[src], non_blocking=True)

            def leg_gen():
                reset()
                ctx.ackgen_dev(*head, 3, 0, SLOT * cap, 6, SLOT, seg, desc, cap, ares, total, work, stream=st)

            def leg_send():
                reset()
                ctx.ack_send_dev(*head, d["links"], image, 0, 6, SLOT, seg, desc, cap, ares, total, status, work, stream=st)

            def leg_pattern():
                reset("tx_pat")
                if P.ackgen_pattern_launch(*tail) != 0:
                    raise SystemExit("the pattern kernels did not launch")

            def leg_variant(lane_max):
                reset()
                if P.ackgen_variant_launch(lane_max, *tail) != 0:
                    raise SystemExit("a variant did not launch")

            leg_send()
            st.synchronize()
            # correctness first
            snap = lambda: tuple(x.cpu().numpy().copy() for x in (seg, desc, ares, total, d["tx"]))
            want = snap()
            T = int(want[3].view(np.uint64)[0])
            res = want[2].view(ACKGEN_RES_DTYPE)[:m]
            tx_after = want[4].view(ACKGEN_STATE_DTYPE)
            if not (res["status"] == am.SENT).all() or T != int(res["n_ack"].sum()) or T > cap or \
                    int((status.cpu().numpy()[:T] != 0).sum()) or not (tx_after["ack_cnt"] == 0).all():
                raise SystemExit("the call's totals are not consistent")
            for j in np.random.default_rng(1).integers(0, m, 200).tolist() + [0]:
                s = int(seg_sid[j])
                opts = [am.ACK_OPT_NOW if f == am.RCV_ACK_NOW else am.ACK_OPT_AGGREGATE
                        for f in place["flags"][idx[seg_start[j]:seg_start[j + 1]]]]
                b = {f: int(tx[s][f]) for f in am.STATE_DTYPE.names if f != "rsvd"}
                b.update(on_ack_list=0, snd_nxt=int(snd[s]["snd_nxt"]),
                         **{f: int(state[s][f]) for f in ("rcv_nxt", "rcv_wnd", "head_seq", "merged_len", "ts_recent")})
                recs, after = am.run_case(b, opts, CUR_TS, 1 << 30)
                if len(recs) != int(res[j]["n_ack"]) or after["ip_id"] != int(tx_after[s]["ip_id"]):
                    raise SystemExit(f"segment {j} differs from the model")
            line[name + "records"], line[name + "segments"] = T, m
            # the pattern's fan-out: each stream's emitted count in its tx record
            tx_pat = tx.copy()
            tx_pat["ack_cnt"][seg_sid[seg_sid <= max_id]] = res["n_ack"][seg_sid <= max_id]
            d["tx_pat"] = to_dev(tx_pat)
            leg_pattern()
            st.synchronize()
            if int(total.cpu().numpy().view(np.uint64)[0]) != T:
                raise SystemExit("the pattern's fan-out is not the call's")
            launches = args.heavy_launches if kind == "heavy" else args.launches
            if kind == "mid":
                line["mid_per_stream"] = per
                line["mid_reset_us"], _ = timed(reset, launches)
                sweep = {}
                for lane_max in (4, 8, 16, 32, 64, 128):
                    leg_variant(lane_max)
                    st.synchronize()
                    if any(a.tobytes() != b_.tobytes() for a, b_ in zip(snap(), want)):
                        raise SystemExit(f"lane threshold {lane_max} differs from the library")
                    us, spread = timed(lambda: leg_variant(lane_max), launches)
                    sweep[str(lane_max)] = {"us_net": round(us - line["mid_reset_us"], 2), "spread": spread}
                line["mid_sweep"] = sweep
                us, _ = timed(leg_pattern, launches)
                line["mid_pattern_us_net"] = round(us - line["mid_reset_us"], 2)
                continue
            legs = {"reset_us": reset, "ackgen_us": leg_gen, "pattern_us": leg_pattern}
            if kind == "even":
                legs["send_us"] = leg_send
            for key, leg in legs.items():
                line[name + key], line[name + key + "_spread"] = timed(leg, launches)
            r = line[name + "reset_us"]
            line[name + "ackgen_us_net"] = round(line[name + "ackgen_us"] - r, 2)
            line[name + "pattern_us_net"] = round(line[name + "pattern_us"] - r, 2)
            line[name + "pattern_over_ackgen"] = round(line[name + "pattern_us_net"] / line[name + "ackgen_us_net"], 3)
    print(json.dumps(line))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
