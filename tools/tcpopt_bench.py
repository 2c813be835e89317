#!/usr/bin/env python3
"""Measures the option kernel (mtcp_amd/csrc/tcpopt_kernels.hpp)
on the MI355X against its own memory pattern.

Workloads: C2's batch (n x 1500 B from mtcp_gpu_pktgen_dev: half the frames
carry NOP NOP TS) and C3's bimodal batch.  In one process, HIP events,
alternating rounds after warm-up, per workload:

  (a) rx_us       the rx launch (mtcp_gpu_rx_chunk_dev);
  (b) tcpopt_us   the option launch (mtcp_gpu_rx_tcpopt_chunk_dev);
  (c) pattern_us  the pattern ceiling: tools/tcpopt_pattern.hip, the same
                  record, descriptor and frame-piece loads and 16 B stores
                  on the same grid, with no walk.

Every option record is checked against a numpy expectation (the two
generated shapes, pktgen.hip gen_headers) before anything is printed.  One
JSON line: the three times, the counted bytes (descriptors + record sectors +
128 B per frame with options + 16 B out), frac_of_pattern = c / b and
price_of_rx = b / a.  The yardstick is (c), never (b) itself.

    make tools/libtcpopt_pattern.so
    python tools/tcpopt_bench.py [--n 1048576] [--rounds 15] [--out profiles/tcpopt/bench_tcpopt.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def expectation(torch, d_buf, desc, res):
    """Option records from the two generated shapes: doff 8 frames carry
    01 01 08 0a + ts_val + ts_ref at bytes 54..65, doff 5 frames nothing;
    flags are ACK [| PSH], so only the timestamp walk runs."""
    from mtcp_amd import TCPOPT_DTYPE
    from mtcp_amd._types import TCPOPT_TS_FOUND
    ok = res["verdict"] == 0
    if not set(np.unique(res["ihl_doff"][ok])) <= {0x55, 0x85} or (res["tcp_flags"][ok] & 0x06).any():
        raise SystemExit("the generated batch has shapes this tool does not know")
    ts = np.nonzero(ok & (res["ihl_doff"] == 0x85))[0]
    want = np.zeros(len(desc), dtype=TCPOPT_DTYPE)
    pos = torch.from_numpy((desc["offset"][ts].astype(np.int64) << 6)).to(d_buf.device)[:, None] + \
        torch.arange(54, 66, device=d_buf.device)
    b = d_buf[pos].cpu().numpy().astype(np.uint32)
    if not (b[:, 0:4] == (1, 1, 8, 10)).all():
        raise SystemExit("a doff 8 frame does not start its options with NOP NOP TS")
    want["ts_val"][ts] = (b[:, 4] << 24) | (b[:, 5] << 16) | (b[:, 6] << 8) | b[:, 7]
    want["ts_ref"][ts] = (b[:, 8] << 24) | (b[:, 9] << 16) | (b[:, 10] << 8) | b[:, 11]
    want["flags"][ts] = TCPOPT_TS_FOUND
    return want, len(ts)


def run(args, size, compact):
    import torch
    from mtcp_amd import TCPOPT_DTYPE, gpu, pktgen

    dev = torch.device("cuda", 0)
    n, seed = args.n, 42
    desc, nbytes = pktgen.layout(n, size, 6, seed)
    d_buf = torch.zeros((nbytes + 15) & ~15, dtype=torch.uint8, device=dev)
    d_desc = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
    gpu.pktgen_dev(d_buf, d_desc, n, 6, seed)
    torch.cuda.synchronize()
    P = ctypes.CDLL(os.path.join(ROOT, "tools", "libtcpopt_pattern.so")).tcpopt_pattern_launch
    vp = ctypes.c_void_p
    P.argtypes = [vp, ctypes.c_uint64, vp, ctypes.c_uint32, ctypes.c_uint32, vp, ctypes.c_int, vp,
                  ctypes.c_uint32, vp]
    P.restype = ctypes.c_int
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    blocks = min((n + 255) // 256, num_cu * 8)            # mtcp_gpu.hip launch_tcpopt

    with gpu.Context(0, compact=compact) as ctx:
        rec = ctx.record_size
        d_res = torch.zeros(n * rec, dtype=torch.uint8, device=dev)
        d_opt = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
        d_pat = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
        st = torch.cuda.Stream(device=dev)
        h = st.cuda_stream

        def leg_rx():
            ctx.rx_chunk_dev(d_buf, d_desc, n, 6, d_res, stream=st)

        def leg_opt():
            ctx.rx_tcpopt_chunk_dev(d_buf, d_desc, n, 6, d_res, d_opt, stream=st)

        def leg_pattern():
            if P(d_buf.data_ptr(), d_buf.numel(), d_desc.data_ptr(), n, 6, d_res.data_ptr(), int(compact),
                 d_pat.data_ptr(), blocks, h) != 0:
                raise SystemExit("the pattern kernel did not launch")

        legs = {"rx_us": leg_rx, "tcpopt_us": leg_opt, "pattern_us": leg_pattern}
        for _ in range(args.warmup):
            for f in legs.values():
                f()
        st.synchronize()
        rx_kernel = ctx.last_kernel
        # correctness first: nothing is printed for records that are wrong
        res = d_res.cpu().numpy().view(ctx.result_dtype)
        want, with_opts = expectation(torch, d_buf, desc, res)
        got = d_opt.cpu().numpy().view(TCPOPT_DTYPE)
        if got.tobytes() != want.tobytes():
            bad = np.nonzero(got.view(np.uint8).reshape(n, 16) != want.view(np.uint8).reshape(n, 16))[0]
            raise SystemExit(f"option records differ from the expectation at packets {np.unique(bad)[:10]}")
        times = {k: [] for k in legs}
        for _ in range(args.rounds):                      # alternating: a, b, c, a, b, c, ...
            for k, f in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(args.launches):
                    f()
                e1.record(st)
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / args.launches)
    med = {k: statistics.median(v) for k, v in times.items()}
    counted = 8 * n + rec * n + 128 * with_opts + 16 * n
    return {
        "workload": f"{n} x {size}{' compact' if compact else ''}",
        "rx_kernel": rx_kernel,
        **{k: round(v, 2) for k, v in med.items()},
        "spread_us": {k: [round(min(v), 2), round(max(v), 2)] for k, v in times.items()},
        "frames_with_options": with_opts,
        "counted_bytes": counted,
        "tcpopt_gbps_counted": round(counted / med["tcpopt_us"] / 1e3, 1),
        "pattern_gbps_counted": round(counted / med["pattern_us"] / 1e3, 1),
        "frac_of_pattern": round(med["pattern_us"] / med["tcpopt_us"], 3),
        "price_of_rx": round(med["tcpopt_us"] / med["rx_us"], 3),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--launches", type=int, default=20, help="launches per timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the MI355X only")
    line = {
        "tool": "tools/tcpopt_bench.py",
        "device": torch.cuda.get_device_name(0),
        "method": f"HIP events around {args.launches} launches, median of {args.rounds} alternating rounds "
                  f"after {args.warmup} warm-up rounds, one process",
        "yardstick": "pattern_us (tools/tcpopt_pattern.hip): same loads and stores, no walk",
        "c2": run(args, 1500, False),
        "c3": run(args, "bimodal", False),
        "c3_compact": run(args, "bimodal", True),
    }
    text = json.dumps(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
