#!/usr/bin/env python3
"""Measures the per-stream receive walk (SURVEY §8 f11,
mtcp_amd/csrc/rcvwalk_kernels.hpp) on the MI355X against four yardsticks.

Workload: C3's bimodal batch (mtcp_gpu_pktgen_dev) through rx, its records'
4-tuples drawn from a pool of keys the device flow table holds (the Table of
tools/group_bench.py), looked up and grouped.  The walk's inputs are those
records with the sequence numbers rewritten per stream: every stream sends its
TCP_OK packets' payloads back to back from rcv_nxt (in arrival order, or with
one segment in eight moved 1-8 places back in its stream's list), flags ACK,
and an option record with a rising timestamp; every stream starts fresh with a
buffer that holds its whole share.  In one process, HIP events around
`launches` launches, median of `rounds` alternating rounds after one second of
untimed launches, per case:

  (a) front_us    the rx, lookup and group launches in front;
  (b) walk_us     a device copy that puts the state array back, then
                  mtcp_gpu_rcvwalk_dev (gather, walk);
  (c) pattern_us  the same copy, then tools/rcvwalk_pattern.hip: the same loads
                  and stores on the same grids, no comparisons, no fragment work;
  (d) reset_us    the copy alone;
  (e) host_us     one host core running the same step function as a plain loop
                  over the same records (best of 3, wall clock).

Cases: 65 536 streams in order and with delays, 1 M streams, half the batch
one stream, 16 384 streams (64 packets each: several rounds a lane), 4 096 records as one captured launch.  With --sweep the walk is
also timed at other round lengths and take-over counts.  Every output of every
case is compared with tests/rcvwalk_model.py before anything is printed.  One
JSON line; frac_of_pattern = (c - d) / (b - d), price_of_front = (b - d) / a.

    make tools/librcvwalk_pattern.so tools/libgroup_pattern.so
    python tools/rcvwalk_bench.py [--n 1048576] [--sweep] [--out profiles/rcvwalk/bench_rcvwalk.json]
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

MISS, NONE = 0xFFFFFFFE, 0xFFFFFFFF
SWEEP = ((32, 0), (32, 1), (32, 3), (32, 8), (8, 3), (128, 3), (0xFFFFFFFF, 0))   # (round length, take-over count)


def pattern_lib():
    P = ctypes.CDLL(os.path.join(ROOT, "tools", "librcvwalk_pattern.so"))
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    P.rcvwalk_pattern_launch.argtypes = [vp, vp, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    P.rcvwalk_pattern_launch.restype = ctypes.c_int
    P.rcvwalk_variant_launch.argtypes = [u32, u32, vp, vp, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    P.rcvwalk_variant_launch.restype = ctypes.c_int
    P.rcvwalk_host_loop.argtypes = [vp, vp, u32, u32, vp, vp, vp, u32, vp, vp, vp]
    P.rcvwalk_host_loop.restype = None
    return P


def walk_inputs(res, sid, max_id, delayed, rng):
    """res with seq / tcp_flags rewritten, the option records and the fresh
    states: every stream's packets carry its bytes back to back."""
    from mtcp_amd._types import RCV_STATE_DTYPE, TCPOPT_DTYPE, TCPOPT_TS_FOUND
    n = len(res)
    res = res.copy()
    on = sid <= max_id
    order = np.argsort(np.where(on, sid, max_id + 1), kind="stable")      # a stream's packets, in arrival order
    s_sorted = sid[order]
    first = np.ones(n, bool)
    first[1:] = s_sorted[1:] != s_sorted[:-1]
    if delayed:                                            # one in eight moves 1-8 places back in its stream's list
        pos = np.arange(n, dtype=np.float64)
        move = (rng.random(n) < 1 / 8) & on[order]
        pos = pos + np.where(move, rng.integers(1, 9, n) + 0.5, 0)
        start = np.maximum.accumulate(np.where(first, np.arange(n), 0))
        seg_end = np.append(np.nonzero(first)[0][1:], n)[np.cumsum(first) - 1]
        pos = np.minimum(pos, seg_end - 0.25)              # never past its stream's last place
        send = np.lexsort((pos, start))                    # the sending order inside each stream's slots
    else:
        send = np.arange(n)
    ln = res["payload_len"][order].astype(np.int64)
    # bytes are numbered in SENDING order (the list before the delays); they arrive in list order
    ln_sent = ln.copy()
    csum = np.cumsum(ln_sent) - ln_sent
    base = np.maximum.accumulate(np.where(first, csum, 0))
    off_sent = csum - base                                 # offset of the k-th sent segment of its stream
    irs = rng.integers(0, 1 << 32, max_id + 1, dtype=np.uint64).astype(np.uint32)
    seq_sent = (irs[np.minimum(s_sorted, max_id)].astype(np.int64) + 1 + off_sent) & 0xFFFFFFFF
    # the segment sent k-th arrives at slot send^-1: slot j receives what was sent at send[j]
    arr_seq, arr_len = seq_sent[send], ln_sent[send]
    res["seq"][order] = arr_seq
    res["payload_len"][order] = arr_len
    res["tcp_flags"] = 0x10
    opt = np.zeros(n, TCPOPT_DTYPE)
    opt["ts_val"], opt["ts_ref"], opt["flags"] = np.arange(n) // 64 + 1000, 7, TCPOPT_TS_FOUND
    total = np.zeros(max_id + 2, np.int64)
    np.add.at(total, np.where(on, sid, max_id + 1), res["payload_len"].astype(np.int64))
    state = np.zeros(max_id + 1, RCV_STATE_DTYPE)
    size = np.maximum(65536, 1 << np.ceil(np.log2(np.maximum(total[:-1], 1) + 1)).astype(np.int64))
    if size.max() > 1 << 30:
        raise SystemExit("a stream's share does not fit the largest buffer")
    state["rcv_nxt"] = state["head_seq"] = irs + np.uint32(1)
    state["rcv_wnd"] = state["size"] = size
    state["ts_recent"], state["tcp_state"], state["saw_timestamp"] = 999, 4, 1
    return res, opt, state


def run(args, P, t, n, max_id, shape, graph, sweep, launches=None, rounds=None):
    import torch
    from group_bench import timed
    from mtcp_amd import gpu
    from mtcp_amd._types import RCV_PLACE_DTYPE, RCV_STATE_DTYPE, RESULT_DTYPE
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
    res, opt, state = walk_inputs(res0, sid, max_id, shape == "delayed", rng)
    d_sid, d_res, d_opt, d_state0 = up(sid), up(res), up(opt), up(state)
    gwb, wb = gpu.Context.group_work_bytes(n, max_id), gpu.Context.rcvwalk_work_bytes(n, max_id)
    d_idx, d_ssid, d_sstart, d_nseg, d_gwork = mk(4 * n), mk(4 * n), mk(4 * n + 4), mk(4), mk(gwb)
    d_look_sid = mk(4 * n)
    sets = {k: (mk(64 * (max_id + 1)), mk(16 * n), mk(4 * n), mk(wb)) for k in ("walk", "pattern")}

    def leg_front():
        ctx.rx_chunk_dev(t.d_buf, t.d_desc, n, 6, t.d_res, stream=st)
        t.tab.lookup_dev(t.d_look, n, d_look_sid, None, stream=st)
        ctx.group_dev(d_sid, n, max_id, d_idx, d_ssid, d_sstart, d_nseg, d_gwork, stream=st)

    def reset(which):
        with torch.cuda.stream(st):
            sets[which][0].copy_(d_state0, non_blocking=True)

    def leg_walk():
        reset("walk")
        s, p, q, w = sets["walk"]
        ctx.rcvwalk_dev(d_res, d_opt, n, max_id, d_idx, d_ssid, d_sstart, d_nseg, s, p, q, w, stream=st)

    def leg_pattern():
        reset("pattern")
        s, p, q, w = sets["pattern"]
        if P.rcvwalk_pattern_launch(d_res.data_ptr(), d_opt.data_ptr(), n, max_id, d_idx.data_ptr(), d_ssid.data_ptr(),
                                    d_sstart.data_ptr(), d_nseg.data_ptr(), s.data_ptr(), p.data_ptr(), q.data_ptr(),
                                    w.data_ptr(), h) != 0:
            raise SystemExit("the pattern kernels did not launch")

    def leg_variant(short, wmax):
        def go():
            reset("walk")
            s, p, q, w = sets["walk"]
            if P.rcvwalk_variant_launch(short, wmax, d_res.data_ptr(), d_opt.data_ptr(), n, max_id, d_idx.data_ptr(),
                                        d_ssid.data_ptr(), d_sstart.data_ptr(), d_nseg.data_ptr(), s.data_ptr(),
                                        p.data_ptr(), q.data_ptr(), w.data_ptr(), h) != 0:
                raise SystemExit("a variant did not launch")
        return go

    legs = {"front_us": leg_front, "walk_us": leg_walk, "pattern_us": leg_pattern, "reset_us": lambda: reset("walk")}
    leg_front()
    st.synchronize()
    # correctness first: nothing is printed for outputs that are wrong
    m = int(d_nseg.cpu().numpy().view(np.uint32)[0])
    u32 = lambda x, k: x.cpu().numpy().view(np.uint32)[:k].copy()
    idx, ssid, sstart = u32(d_idx, n), u32(d_ssid, m), u32(d_sstart, m + 1)
    want = rm.walk(res, opt, max_id, idx, ssid, sstart, state)

    def verify(what):
        st.synchronize()
        s, p, q, _ = sets["walk"]
        if p.cpu().numpy().view(RCV_PLACE_DTYPE)[:n].tobytes() != want[0].tobytes() or \
                s.cpu().numpy().view(RCV_STATE_DTYPE)[:max_id + 1].tobytes() != want[1].tobytes() or \
                not np.array_equal(u32(q, m), want[2]):
            raise SystemExit(f"{what}: the walk's outputs differ from the model")

    leg_walk()
    verify("the library")
    variants = {}
    if sweep:
        for short, wmax in SWEEP:
            leg_variant(short, wmax)()
            verify(f"round {short}, take-over {wmax}")
            variants[f"round_{short if short != 0xFFFFFFFF else 'all'}_wave_{wmax}_us"] = leg_variant(short, wmax)
    leg_pattern()
    st.synchronize()
    a = argparse.Namespace(**vars(args))
    a.launches, a.rounds = launches or args.launches, rounds or args.rounds
    med, spread = timed(a, {**legs, **variants}, st, graph)
    # one host core, the same step function as a plain loop
    place, stop = np.zeros(n, RCV_PLACE_DTYPE), np.zeros(m, np.uint32)
    host_us = None
    for _ in range(3):
        hs = state.copy()
        t0 = time.perf_counter()
        P.rcvwalk_host_loop(res.ctypes.data, opt.ctypes.data, n, max_id, idx.ctypes.data, ssid.ctypes.data,
                            sstart.ctypes.data, m, hs.ctypes.data, place.ctypes.data, stop.ctypes.data)
        dt = (time.perf_counter() - t0) * 1e6
        host_us = dt if host_us is None else min(host_us, dt)
    if place.tobytes() != want[0].tobytes() or hs.tobytes() != want[1].tobytes():
        raise SystemExit("the host loop's outputs differ from the model")
    print(f"measured: {n} records, max_id {max_id}, {shape}", file=sys.stderr, flush=True)
    counts = np.bincount(want[0]["verdict"], minlength=16)
    seg_len = np.diff(sstart.astype(np.int64))[ssid <= max_id]
    walk, pat = med["walk_us"] - med["reset_us"], med["pattern_us"] - med["reset_us"]
    return {
        "case": f"{n} records, max_id {max_id}, {shape}{', HIP graph' if graph else ''}",
        "launches_per_window": a.launches, "rounds": a.rounds,
        **{k: round(v, 2) for k, v in med.items()},
        "spread_us": spread,
        "host_us": round(host_us, 1),
        "stream_segments": int(len(seg_len)), "longest_segment": int(seg_len.max()) if len(seg_len) else 0,
        "verdicts": {rm.RCV_VERDICTS[k]: int(c) for k, c in enumerate(counts) if c},
        "share_deferred": round(float(counts[1:7].sum()) / n, 4),
        "walk_less_reset_us": round(walk, 2),
        "frac_of_pattern": round(pat / walk, 3),
        "price_of_front": round(walk / med["front_us"], 3),
        "host_over_walk": round(host_us / walk, 2),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--launches", type=int, default=20, help="launches per timed window")
    ap.add_argument("--warm-seconds", type=float, default=1.0)
    ap.add_argument("--sweep", action="store_true", help="also time the walk at other round lengths and take-over counts")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the MI355X only")
    from group_bench import Table
    from mtcp_amd import gpu
    P = pattern_lib()
    line = {
        "tool": "tools/rcvwalk_bench.py",
        "device": torch.cuda.get_device_name(0),
        "round_len": gpu.Context.rcvwalk_short_len(),
        "method": f"HIP events around {args.launches} launches (2 for the heavy stream), median of {args.rounds} "
                  f"alternating rounds (5 for the heavy stream) after {args.warm_seconds} s of untimed launches, one "
                  "process; every timed walk and pattern launch is preceded by a device copy that puts the state "
                  "array back (reset_us, subtracted in the ratios); no counter or trace run stands behind any figure",
        "yardsticks": "pattern_us (tools/rcvwalk_pattern.hip): same loads and stores on the same grids, no "
                      "comparisons, no fragment work; front_us: the rx, lookup and group launches; host_us: the same "
                      "step function as a plain loop on one host core, best of 3; share_deferred",
    }
    with gpu.Context(0) as ctx:
        t = Table(ctx, args.n, 65536, 17)
        line["c3_64k_streams_in_order"] = run(args, P, t, args.n, 65535, "in_order", False, args.sweep)
        line["c3_64k_streams_delayed"] = run(args, P, t, args.n, 65535, "delayed", False, False)
        line["c3_half_one_stream"] = run(args, P, t, args.n, 65535, "half_one_stream", False, args.sweep, 2, 5)
        line["small_4096_graph"] = run(args, P, t, 4096, 65535, "in_order", True, False)
        t.close()
        t = Table(ctx, args.n, 16384, 15)
        line["c3_16k_streams_delayed"] = run(args, P, t, args.n, 16383, "delayed", False, args.sweep)
        t.close()
        flows = 1 << 20
        t = Table(ctx, args.n, flows, 21)
        line["c3_1m_streams"] = run(args, P, t, args.n, flows - 1, "in_order", False, False)
        t.close()
    text = json.dumps(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
