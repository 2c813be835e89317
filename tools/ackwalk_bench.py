#!/usr/bin/env python3
"""Measures the per-stream ProcessACK walk (SURVEY §8 f13,
mtcp_amd/csrc/ackwalk_kernels.hpp) on the MI355X against its yardsticks.

Workload: the batches of tools/rcvwalk_bench.py (C3's bimodal batch through rx,
its 4-tuples from a pool of keys the device flow table holds, looked up and
grouped, the sequence numbers rewritten per stream), walked by the receive
walk, and on top the send side: every stream has a send buffer that holds what
its packets acknowledge, all of it sent; every packet acknowledges one more
effective MSS, one in eight repeats the ACK before it (old: the packets carry
payload, so it is no duplicate); the congestion window starts in slow start
and passes ssthresh (four MSS) with a stream's third new ACK, so most steps
take both of ProcessACK's divisions;
timestamps on, no RTT estimate yet.  In one process, HIP events around
`launches` launches, median of `rounds` alternating rounds after one second of
untimed launches, per case:

  (a) front_us    the rx, lookup, group and receive-walk launches in front;
  (b) walk_us     a device copy that puts the send states back, then
                  mtcp_gpu_ackwalk_dev (gather, walk);
  (c) pattern_us  the same copy, then tools/ackwalk_pattern.hip: the same loads
                  and stores on the same grids, no comparisons, no divisions;
  (d) reset_us    the copy alone;
  (e) rcvwalk_us  f11's walk of the same batch with its own state copy, and
                  rcv_reset_us, that copy alone: the yardstick next door;
  (f) host_us     one host core running the same step function as a plain loop
                  over the same records (best of 3, wall clock).

Cases: f11's six.  Every output of every case is compared with
tests/ackwalk_model.py (and the receive walk's with tests/rcvwalk_model.py)
before anything is printed.  One JSON line; frac_of_pattern = (c - d) / (b - d),
price_of_front = (b - d) / a, over_rcvwalk = (b - d) / (e - its reset).

    make tools/libackwalk_pattern.so tools/librcvwalk_pattern.so tools/libgroup_pattern.so
    python tools/ackwalk_bench.py [--n 1048576] [--out profiles/ackwalk/bench_ackwalk.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CUR_TS = 5000


def pattern_lib():
    P = ctypes.CDLL(os.path.join(ROOT, "tools", "libackwalk_pattern.so"))
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    P.ackwalk_pattern_launch.argtypes = [vp, vp, vp, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    P.ackwalk_pattern_launch.restype = ctypes.c_int
    P.ackwalk_host_loop.argtypes = [vp, vp, vp, u32, u32, vp, vp, vp, u32, u32, vp, vp, vp]
    P.ackwalk_host_loop.restype = None
    return P


def ack_inputs(res, sid, max_id, rng):
    """res with ack_seq / window rewritten, and the send states: see the module's text."""
    from mtcp_amd._types import ACK_STATE_DTYPE
    n = len(res)
    res = res.copy()
    on = sid <= max_id
    order = np.argsort(np.where(on, sid, max_id + 1), kind="stable")
    s_sorted = sid[order]
    first = np.ones(n, bool)
    first[1:] = s_sorted[1:] != s_sorted[:-1]
    eff = 1448
    fresh = (rng.random(n) >= 1 / 8) | first                 # this packet acknowledges new data
    csum = np.cumsum(fresh)
    k = csum - np.maximum.accumulate(np.where(first, csum - fresh, 0))     # new segments acknowledged so far, this stream
    iss = rng.integers(0, 1 << 32, max_id + 1, dtype=np.uint64).astype(np.uint32)
    res["ack_seq"][order] = (iss[np.minimum(s_sorted, max_id)].astype(np.int64) + k * eff) & 0xFFFFFFFF
    res["window"] = 40000
    total = np.zeros(max_id + 2, np.int64)
    np.add.at(total, np.where(on, sid, max_id + 1)[order], fresh * eff)
    queued = total[:-1] + 10000
    if queued.max() > 1 << 30:
        raise SystemExit("a stream's share does not fit the largest send buffer")
    snd = np.zeros(max_id + 1, ACK_STATE_DTYPE)
    snd["snd_una"] = snd["sb_head_seq"] = snd["last_ack_seq"] = snd["snd_wl2"] = iss
    snd["sb_len"], snd["snd_nxt"] = queued, iss + queued.astype(np.uint32)
    snd["sb_size"] = np.maximum(65536, 1 << np.ceil(np.log2(queued + 1)).astype(np.int64))
    snd["snd_wnd"] = snd["sb_size"] - snd["sb_len"]
    snd["peer_wnd"], snd["cwnd"], snd["ssthresh"], snd["rto"] = 40000, 2 * 1460, 4 * 1460, 30
    snd["mss"], snd["eff_mss"], snd["tcp_state"], snd["saw_timestamp"], snd["has_sndbuf"] = 1460, eff, 4, 1, 1
    return res, snd


def run(args, P, t, n, max_id, shape, graph, launches=None, rounds=None):
    import torch
    from group_bench import timed
    from mtcp_amd import gpu
    from mtcp_amd._types import ACK_REC_DTYPE, ACK_STATE_DTYPE, RCV_PLACE_DTYPE, RCV_STATE_DTYPE, RESULT_DTYPE
    from rcvwalk_bench import walk_inputs
    from tests import ackwalk_model as am
    from tests import rcvwalk_model as rm

    ctx, dev = t.ctx, t.dev
    st = torch.cuda.Stream(device=dev)
    h = st.cuda_stream
    mk = lambda b: torch.zeros(max(b, 16), dtype=torch.uint8, device=dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    rng = np.random.default_rng(n + max_id)
    sid = t.want_sid[:n].copy()
    if shape == "half_one_stream":
        sid = np.where((rng.random(n) < 0.5) & (sid <= max_id), 7, sid).astype(np.uint32)
    res0 = t.d_look.cpu().numpy().view(RESULT_DTYPE)[:n]
    res, opt, state = walk_inputs(res0, sid, max_id, shape == "delayed", rng)      # f11's batch
    res, snd = ack_inputs(res, sid, max_id, rng)
    d_sid, d_res, d_opt, d_state0, d_snd0 = up(sid), up(res), up(opt), up(state), up(snd)
    gwb, rwb = gpu.Context.group_work_bytes(n, max_id), gpu.Context.rcvwalk_work_bytes(n, max_id)
    wb = gpu.Context.ackwalk_work_bytes(n, max_id)
    d_idx, d_ssid, d_sstart, d_nseg, d_gwork = mk(4 * n), mk(4 * n), mk(4 * n + 4), mk(4), mk(gwb)
    d_look_sid = mk(4 * n)
    d_state, d_place, d_rstop, d_rwork = mk(64 * (max_id + 1)), mk(16 * n), mk(4 * n), mk(rwb)
    d_place2, d_rstop2 = mk(16 * n), mk(4 * n)             # the timed receive walks write here: d_place stays the input
    sets = {k: (mk(128 * (max_id + 1)), mk(16 * n), mk(4 * n), mk(wb)) for k in ("walk", "pattern")}

    def rcv_reset():
        with torch.cuda.stream(st):
            d_state.copy_(d_state0, non_blocking=True)

    def rcv_walk(place, stop):
        rcv_reset()
        ctx.rcvwalk_dev(d_res, d_opt, n, max_id, d_idx, d_ssid, d_sstart, d_nseg, d_state, place, stop, d_rwork, stream=st)

    def leg_front():
        ctx.rx_chunk_dev(t.d_buf, t.d_desc, n, 6, t.d_res, stream=st)
        t.tab.lookup_dev(t.d_look, n, d_look_sid, None, stream=st)
        ctx.group_dev(d_sid, n, max_id, d_idx, d_ssid, d_sstart, d_nseg, d_gwork, stream=st)
        rcv_walk(d_place2, d_rstop2)

    def reset(which):
        with torch.cuda.stream(st):
            sets[which][0].copy_(d_snd0, non_blocking=True)

    def leg_walk():
        reset("walk")
        s, a, q, w = sets["walk"]
        ctx.ackwalk_dev(d_res, d_opt, d_place, n, max_id, d_idx, d_ssid, d_sstart, d_nseg, CUR_TS, s, a, q, w, stream=st)

    def leg_pattern():
        reset("pattern")
        s, a, q, w = sets["pattern"]
        if P.ackwalk_pattern_launch(d_res.data_ptr(), d_opt.data_ptr(), d_place.data_ptr(), n, max_id, d_idx.data_ptr(),
                                    d_ssid.data_ptr(), d_sstart.data_ptr(), d_nseg.data_ptr(), s.data_ptr(),
                                    a.data_ptr(), q.data_ptr(), w.data_ptr(), h) != 0:
            raise SystemExit("the pattern kernels did not launch")

    legs = {"front_us": leg_front, "walk_us": leg_walk, "pattern_us": leg_pattern, "reset_us": lambda: reset("walk"),
            "rcvwalk_us": lambda: rcv_walk(d_place2, d_rstop2), "rcv_reset_us": rcv_reset}
    leg_front()
    rcv_walk(d_place, d_rstop)
    st.synchronize()
    # correctness first: nothing is printed for outputs that are wrong
    m = int(d_nseg.cpu().numpy().view(np.uint32)[0])
    u32 = lambda x, k: x.cpu().numpy().view(np.uint32)[:k].copy()
    idx, ssid, sstart = u32(d_idx, n), u32(d_ssid, m), u32(d_sstart, m + 1)
    rwant = rm.walk(res, opt, max_id, idx, ssid, sstart, state)
    if d_place.cpu().numpy().view(RCV_PLACE_DTYPE)[:n].tobytes() != rwant[0].tobytes() or \
            d_state.cpu().numpy().view(RCV_STATE_DTYPE)[:max_id + 1].tobytes() != rwant[1].tobytes():
        raise SystemExit("the receive walk's outputs differ from its model")
    want = am.walk(res, opt, rwant[0], max_id, idx, ssid, sstart, CUR_TS, snd)
    leg_walk()
    st.synchronize()
    s, a, q, _ = sets["walk"]
    if a.cpu().numpy().view(ACK_REC_DTYPE)[:n].tobytes() != want[0].tobytes() or \
            s.cpu().numpy().view(ACK_STATE_DTYPE)[:max_id + 1].tobytes() != want[1].tobytes() or \
            not np.array_equal(u32(q, m), want[2]):
        raise SystemExit("the ACK walk's outputs differ from the model")
    leg_pattern()
    st.synchronize()
    ar = argparse.Namespace(**vars(args))
    ar.launches, ar.rounds = launches or args.launches, rounds or args.rounds
    med, spread = timed(ar, legs, st, graph)
    # one host core, the same step function as a plain loop
    place = np.ascontiguousarray(rwant[0])
    ack, stop = np.zeros(n, ACK_REC_DTYPE), np.zeros(m, np.uint32)
    host_us = None
    for _ in range(3):
        hs = snd.copy()
        t0 = time.perf_counter()
        P.ackwalk_host_loop(res.ctypes.data, opt.ctypes.data, place.ctypes.data, n, max_id, idx.ctypes.data,
                            ssid.ctypes.data, sstart.ctypes.data, m, CUR_TS, hs.ctypes.data, ack.ctypes.data,
                            stop.ctypes.data)
        dt = (time.perf_counter() - t0) * 1e6
        host_us = dt if host_us is None else min(host_us, dt)
    if ack.tobytes() != want[0].tobytes() or hs.tobytes() != want[1].tobytes():
        raise SystemExit("the host loop's outputs differ from the model")
    print(f"measured: {n} records, max_id {max_id}, {shape}", file=sys.stderr, flush=True)
    counts = np.bincount(want[0]["verdict"], minlength=16)
    seg_len = np.diff(sstart.astype(np.int64))[ssid <= max_id]
    walk, pat = med["walk_us"] - med["reset_us"], med["pattern_us"] - med["reset_us"]
    rcv = med["rcvwalk_us"] - med["rcv_reset_us"]
    return {
        "case": f"{n} records, max_id {max_id}, {shape}{', HIP graph' if graph else ''}",
        "launches_per_window": ar.launches, "rounds": ar.rounds,
        **{k: round(v, 2) for k, v in med.items()},
        "spread_us": spread,
        "host_us": round(host_us, 1),
        "stream_segments": int(len(seg_len)), "longest_segment": int(seg_len.max()) if len(seg_len) else 0,
        "verdicts": {am.ACK_VERDICTS[k]: int(c) for k, c in enumerate(counts) if c},
        "share_deferred": round(float(counts[1:7].sum()) / n, 4),
        "walk_less_reset_us": round(walk, 2),
        "rcvwalk_less_reset_us": round(rcv, 2),
        "frac_of_pattern": round(pat / walk, 3),
        "price_of_front": round(walk / med["front_us"], 3),
        "over_rcvwalk": round(walk / rcv, 3),
        "host_over_walk": round(host_us / walk, 2),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--launches", type=int, default=20, help="launches per timed window")
    ap.add_argument("--warm-seconds", type=float, default=1.0)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the MI355X only")
    from group_bench import Table
    from mtcp_amd import gpu
    P = pattern_lib()
    line = {
        "tool": "tools/ackwalk_bench.py",
        "device": torch.cuda.get_device_name(0),
        "round_len": gpu.Context.ackwalk_short_len(),
        "method": f"HIP events around {args.launches} launches (2 for the heavy stream), median of {args.rounds} "
                  f"alternating rounds (5 for the heavy stream) after {args.warm_seconds} s of untimed launches, one "
                  "process; every timed walk and pattern launch is preceded by a device copy that puts the state "
                  "array back (reset_us and rcv_reset_us, subtracted in the ratios); no counter or trace run stands "
                  "behind any figure",
        "yardsticks": "pattern_us (tools/ackwalk_pattern.hip): same loads and stores on the same grids, no "
                      "comparisons, no divisions; front_us: the rx, lookup, group and receive-walk launches; "
                      "rcvwalk_us: f11's walk of the same batch; host_us: the same step function as a plain loop on "
                      "one host core, best of 3; share_deferred",
    }
    def keep(name, result):                                # the file holds the cases measured so far
        line[name] = result
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(line) + "\n")

    with gpu.Context(0) as ctx:
        t = Table(ctx, args.n, 65536, 17)
        keep("c3_64k_streams_in_order", run(args, P, t, args.n, 65535, "in_order", False))
        keep("c3_64k_streams_delayed", run(args, P, t, args.n, 65535, "delayed", False))
        keep("c3_half_one_stream", run(args, P, t, args.n, 65535, "half_one_stream", False, 2, 5))
        keep("small_4096_graph", run(args, P, t, 4096, 65535, "in_order", True))
        t.close()
        t = Table(ctx, args.n, 16384, 15)
        keep("c3_16k_streams_delayed", run(args, P, t, args.n, 16383, "delayed", False))
        t.close()
        flows = 1 << 20
        t = Table(ctx, args.n, flows, 21)
        keep("c3_1m_streams", run(args, P, t, args.n, flows - 1, "in_order", False))
        t.close()
    print(json.dumps(line))


if __name__ == "__main__":
    main()
