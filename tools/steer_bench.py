#!/usr/bin/env python3
"""Measures the steer passes (mtcp_amd/csrc/steer_kernels.hpp)
on the MI355X against their own memory pattern.

Workload: C3's bimodal batch (mtcp_gpu_pktgen_dev) through rx with the
Microsoft RSS key; the records rx wrote are steered.  In one process, HIP
events around `launches` launches, median of `rounds` alternating rounds after
one second of untimed launches, per case:

  (a) rx_us       the rx launch (mtcp_gpu_rx_chunk_dev);
  (b) steer_us    the steer passes (mtcp_gpu_steer_dev: count, scan, emit, or
                  the one workgroup of a batch of at most one tile);
  (c) pattern_us  tools/steer_pattern.hip: the same record-dword loads, parked
                  bytes, counts and 4 B index stores (8 B descriptors where
                  asked) on the same grids, index i stored at position i, no
                  ranking.

The lists are checked against numpy (a stable argsort of the destinations)
before anything is printed.  One JSON line: the three times, frac_of_pattern =
c / b and price_of_rx = b / a per case, and one CPU figure: numpy's stable
argsort of the same destinations on one core.  The yardstick is (c), never a
figure of the kernels under test.

    make tools/libsteer_pattern.so
    python tools/steer_bench.py [--n 1048576] [--out profiles/steer/bench_steer.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEY_MICROSOFT = bytes([
    0x6d, 0x5a, 0x56, 0xda, 0x25, 0x5b, 0x0e, 0xc2, 0x41, 0x67, 0x25, 0x3d, 0x43, 0xa3,
    0x8f, 0xb0, 0xd0, 0xca, 0x2b, 0xcb, 0xae, 0x7b, 0x30, 0xb4, 0x77, 0xcb, 0x2d, 0xa3,
    0x80, 0x30, 0xf2, 0x0c, 0x6a, 0x42, 0xb7, 0x3b, 0xbe, 0xac, 0x01, 0xfa])


def model(res, Q, flags):
    verdict, queue = res["verdict"].astype(np.int64), res["rss_queue"].astype(np.int64)
    rest = queue >= Q
    if flags & 1:
        rest |= (verdict == 4) | (verdict == 9) | (verdict >= 10)
    d = np.where(rest, Q, queue)
    start = np.zeros(Q + 2, np.uint32)
    start[1:] = np.cumsum(np.bincount(d, minlength=Q + 1))
    return d, np.argsort(d, kind="stable").astype(np.uint32), start


def run(args, n, Q, compact, gather, graph):
    import torch
    from mtcp_amd import DESC_DTYPE, STEER_DROP_BAD, gpu, pktgen

    dev = torch.device("cuda", 0)
    seed, flags = 42, STEER_DROP_BAD
    desc, nbytes = pktgen.layout(n, "bimodal", 6, seed)
    d_buf = torch.zeros((nbytes + 15) & ~15, dtype=torch.uint8, device=dev)
    d_desc = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
    gpu.pktgen_dev(d_buf, d_desc, n, 6, seed)
    torch.cuda.synchronize()
    P = ctypes.CDLL(os.path.join(ROOT, "tools", "libsteer_pattern.so")).steer_pattern_launch
    vp = ctypes.c_void_p
    P.argtypes = [vp, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, vp, vp, vp, vp, vp, vp]
    P.restype = ctypes.c_int

    with gpu.Context(0, rss=True, rss_key=KEY_MICROSOFT, rss_queues=Q, rss_endian=False,
                     compact=compact) as ctx:
        rec = ctx.record_size
        wb = ctx.steer_work_bytes(n)
        d_res = torch.zeros(n * rec, dtype=torch.uint8, device=dev)
        mk = lambda b: torch.zeros(b, dtype=torch.uint8, device=dev)
        d_idx, d_start, d_work, d_dout = mk(4 * n), mk(4 * (Q + 2)), mk(wb), mk(8 * n)
        p_idx, p_start, p_work, p_dout = mk(4 * n), mk(4 * (Q + 2)), mk(wb), mk(8 * n)
        st = torch.cuda.Stream(device=dev)
        h = st.cuda_stream

        def leg_rx():
            ctx.rx_chunk_dev(d_buf, d_desc, n, 6, d_res, stream=st)

        def leg_steer():
            ctx.steer_dev(d_res, n, d_idx, d_start, d_work, flags=flags, desc=d_desc if gather else None,
                          desc_out=d_dout if gather else None, stream=st)

        def leg_pattern():
            if P(d_res.data_ptr(), int(compact), n, Q, p_idx.data_ptr(), p_start.data_ptr(),
                 d_desc.data_ptr() if gather else None, p_dout.data_ptr() if gather else None,
                 p_work.data_ptr(), h) != 0:
                raise SystemExit("the pattern kernels did not launch")

        legs = {"rx_us": leg_rx, "steer_us": leg_steer, "pattern_us": leg_pattern}
        for f in legs.values():
            f()
        st.synchronize()
        # correctness first: nothing is printed for lists that are wrong
        res = d_res.cpu().numpy().view(ctx.result_dtype)
        dests, want_idx, want_start = model(res, Q, flags)
        got_idx, got_start = d_idx.cpu().numpy().view(np.uint32), d_start.cpu().numpy().view(np.uint32)
        if not np.array_equal(got_idx, want_idx) or not np.array_equal(got_start, want_start):
            raise SystemExit("the lists differ from numpy's stable partition")
        if gather and d_dout.cpu().numpy().view(DESC_DTYPE).tobytes() != desc[want_idx].tobytes():
            raise SystemExit("the gathered descriptors differ from desc[idx]")
        if graph:                                 # `launches` launches of each leg in a HIP graph
            graphs = {}
            for k, f in legs.items():
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=st):
                    for _ in range(args.launches):
                        f()
                graphs[k] = g
            window = {k: g.replay for k, g in graphs.items()}
        else:
            def many(f):
                def go():
                    for _ in range(args.launches):
                        f()
                return go
            window = {k: many(f) for k, f in legs.items()}
        t_end = time.monotonic() + args.warm_seconds            # untimed launches first
        while time.monotonic() < t_end:
            with torch.cuda.stream(st):
                for w in window.values():
                    w()
            st.synchronize()
        times = {k: [] for k in legs}
        for _ in range(args.rounds):                            # alternating: a, b, c, a, b, c, ...
            for k, w in window.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.cuda.stream(st):
                    e0.record(st)
                    w()
                    e1.record(st)
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / args.launches)
        rx_kernel = ctx.last_kernel
    med = {k: statistics.median(v) for k, v in times.items()}
    ntiles = -(-n // gpu.Context.steer_tile())
    return {
        "case": f"{n} records of {rec} B, Q = {Q}{', desc_out' if gather else ''}{', HIP graph' if graph else ''}",
        "rx_kernel": rx_kernel,
        "launches_per_steer": 1 if ntiles == 1 else 3,
        **{k: round(v, 2) for k, v in med.items()},
        "spread_us": {k: [round(min(v), 2), round(max(v), 2)] for k, v in times.items()},
        "lists_used": int((np.diff(want_start.astype(np.int64)) > 0).sum()),
        "frac_of_pattern": round(med["pattern_us"] / med["steer_us"], 3),
        "price_of_rx": round(med["steer_us"] / med["rx_us"], 3),
    }, dests


def cpu_figure(dests, reps=5):
    """numpy's stable argsort of the destination bytes (one core): what the
    model does, not mTCP code."""
    d8 = dests.astype(np.uint8)
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        np.argsort(d8, kind="stable")
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return round(best * 1e6, 1)


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
    cases = {
        "c3_q16": (args.n, 16, False, False, False),
        "c3_q16_compact": (args.n, 16, True, False, False),
        "c3_q16_desc": (args.n, 16, False, True, False),
        "c3_q16_compact_desc": (args.n, 16, True, True, False),
        "c3_q128": (args.n, 128, False, False, False),
        "small_4096_graph": (4096, 16, False, False, True),
        "small_4096_desc_graph": (4096, 16, False, True, True),
    }
    line = {
        "tool": "tools/steer_bench.py",
        "device": torch.cuda.get_device_name(0),
        "method": f"HIP events around {args.launches} launches, median of {args.rounds} alternating rounds "
                  f"after {args.warm_seconds} s of untimed launches, one process",
        "yardstick": "pattern_us (tools/steer_pattern.hip): same loads and stores on the same grids, no ranking",
    }
    dests = None
    for name, c in cases.items():
        line[name], d = run(args, *c)
        if name == "c3_q16":
            dests = d
    line["cpu_numpy_stable_argsort_1core_us"] = cpu_figure(dests)
    line["cpu_note"] = f"np.argsort(kind='stable') of the {len(dests)} destination bytes of c3_q16, best of 5, one core"
    text = json.dumps(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
