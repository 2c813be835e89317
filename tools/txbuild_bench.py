#!/usr/bin/env python3
"""Measures the frame builder (mtcp_amd/csrc/txbuild_kernels.hpp)
on the MI355X against its own memory pattern and against what the tree did
before it: the tx fill over frames a CPU has assembled.

In one process, HIP events around `launches` launches, median of `rounds`
alternating rounds after one second of untimed launches, per case:

  (b) build_us    mtcp_gpu_tx_build_dev: segment records in, frames out;
  (c) pattern_us  tools/txbuild_pattern.hip: the same record, descriptor, link
                  and payload loads and the same frame stores on the same
                  grid, no sums, no shifts, no header shuffles;
  (a) fill_us     mtcp_gpu_tx_fill_dev over the frames just built: the sum
                  alone, which is all the device took over before.

Cases (uniform segments, TCP_FLAG_ACK | TCP_FLAG_PSH, or pure ACKs):
  mss         payload 1 448 B (FlushTCPSendingBuffer's mss - 12, tcp_out.c:360),
              consecutive source offsets, 1 536 B slots
  mss_odd     the same with a random source byte alignment per segment
  jumbo       payload 8 948 B with max_mss 8 960, 9 216 B slots
  acks        payload 0, 128 B slots
  mss_4096    4 096 x 1 448 B

Every frame of every case, and every status byte, is compared with the model
(tests/txbuild_model.py build_uniform, pinned on the reference's frames by
tests/test_txbuild_model.py) before anything is printed.  One JSON line: the
three times, frac_of_pattern = c / b, the counted bytes (56 + payload_len read
and frame_len + 1 written per segment, computed here from the shapes) and the
rate they give over build_us.  The yardstick is (c), never a figure of the
kernel under test.

    make tools/libtxbuild_pattern.so
    python tools/txbuild_bench.py [--out profiles/txbuild/bench_txbuild.json]
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

CHECK_BLOCK = 1 << 14          # segments per block of the model check


def make_case(n, plen, slot, scattered, seed=3):
    from mtcp_amd import DESC_DTYPE, TX_LINK_DTYPE, TX_SEG_DTYPE
    from mtcp_amd._types import TXB_FLAG_ACK, TXB_FLAG_PSH
    rng = np.random.default_rng(seed)
    seg = np.zeros(n, TX_SEG_DTYPE)
    for f in ("saddr", "daddr", "seq", "ack", "ts_val", "ts_ecr"):
        seg[f] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    for f in ("sport", "dport", "window", "ip_id"):
        seg[f] = rng.integers(0, 1 << 16, n)
    seg["link"] = rng.integers(0, 4, n)
    seg["flags"] = TXB_FLAG_ACK | (TXB_FLAG_PSH if plen else 0)
    seg["payload_len"] = plen
    stride = plen + 16 if scattered else plen
    seg["payload_off"] = np.arange(n, dtype=np.uint64) * np.uint64(stride)
    if scattered:
        seg["payload_off"] += rng.integers(0, 16, n, dtype=np.uint64)
    links = np.zeros(4, TX_LINK_DTYPE)
    links["dst"], links["src"] = rng.integers(0, 256, (4, 6)), rng.integers(0, 256, (4, 6))
    desc = np.zeros(n, DESC_DTYPE)
    desc["offset"] = np.arange(n, dtype=np.uint64) * np.uint64(slot >> 6)
    desc["len"] = 66 + plen
    return seg, links, desc, int(seg["payload_off"][-1]) + plen


def check(seg, d_payload, links, d_buf, d_status, n, slot, L):
    """Every frame and every status byte against the model, block by block."""
    from tests import txbuild_model as m
    status = d_status.cpu().numpy()
    if status.any():
        bad = np.flatnonzero(status)
        raise SystemExit(f"{len(bad)} segments of the case were not built: first {bad[0]} with status "
                         f"{status[bad[0]]}, statuses seen {np.unique(status).tolist()}")
    payload = d_payload.cpu().numpy()
    frames = d_buf.view(n, slot)
    for at in range(0, n, CHECK_BLOCK):
        part = seg[at:at + CHECK_BLOCK]
        want = m.build_uniform(part.astype(m.SEG_DTYPE), payload, links.astype(m.LINK_DTYPE))
        got = frames[at:at + len(part), :L].cpu().numpy()
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)[0]
            raise SystemExit(f"segment {at + bad[0]}: frame byte {bad[1]} differs from the model")


def run(args, name, n, plen, slot, scattered, max_mss):
    import torch
    from mtcp_amd import gpu
    dev = torch.device("cuda", 0)
    seg, links, desc, payload_bytes = make_case(n, plen, slot, scattered)
    L = 66 + plen
    up = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(dev)
    d_seg, d_links, d_desc = up(seg), up(links), up(desc)
    g = torch.Generator(device=dev).manual_seed(5)
    d_payload = torch.randint(0, 256, (payload_bytes,), dtype=torch.uint8, device=dev, generator=g)
    d_buf = torch.zeros(n * slot, dtype=torch.uint8, device=dev)
    p_buf = torch.zeros(n * slot, dtype=torch.uint8, device=dev)
    d_status = torch.full((n,), 0xA5, dtype=torch.uint8, device=dev)
    p_status = torch.full((n,), 0xA5, dtype=torch.uint8, device=dev)
    P = ctypes.CDLL(os.path.join(ROOT, "tools", "libtxbuild_pattern.so")).txbuild_pattern_launch
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    P.argtypes = [vp, u32, vp, u64, vp, u32, vp, u64, vp, u32, vp, ctypes.c_int, vp]
    P.restype = ctypes.c_int
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    st = torch.cuda.Stream(device=dev)
    h = st.cuda_stream
    torch.cuda.synchronize()                 # the fills above run on another stream than the legs
    with gpu.Context(0) as ctx:
        def leg_build():
            ctx.tx_build_dev(d_seg, n, d_payload, d_links, d_buf, d_desc, 6, d_status, max_mss=max_mss, stream=st)

        def leg_pattern():
            if P(d_seg.data_ptr(), n, d_payload.data_ptr(), payload_bytes, d_links.data_ptr(), len(links),
                 p_buf.data_ptr(), n * slot, d_desc.data_ptr(), 6, p_status.data_ptr(), num_cu, h) != 0:
                raise SystemExit("the pattern kernel did not launch")

        def leg_fill():
            ctx.tx_fill_dev(d_buf, d_desc, n, 6, stream=st)

        leg_build()
        st.synchronize()
        build_kernel = ctx.last_kernel
        check(seg, d_payload, links, d_buf, d_status, n, slot, L)     # nothing is printed for wrong frames
        legs = {"build_us": leg_build, "pattern_us": leg_pattern, "fill_us": leg_fill}
        for f in legs.values():
            f()
        st.synchronize()
        fill_kernel = ctx.last_kernel
        if p_status.cpu().numpy().any():
            raise SystemExit("the pattern kernel skipped a segment")

        def many(f):
            def go():
                for _ in range(args.launches):
                    f()
            return go
        window = {k: many(f) for k, f in legs.items()}
        t_end = time.monotonic() + args.warm_seconds            # untimed launches first
        while time.monotonic() < t_end:
            for w in window.values():
                w()
            st.synchronize()
        times = {k: [] for k in legs}
        for _ in range(args.rounds):                            # alternating: b, c, a, b, c, a, ...
            for k, w in window.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                w()
                e1.record(st)
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / args.launches)
        leg_build()                                             # the frames after the timed fills: still the model's
        st.synchronize()
        check(seg, d_payload, links, d_buf, d_status, n, slot, L)
    med = {k: statistics.median(v) for k, v in times.items()}
    rd, wr = n * (56 + plen), n * (L + 1)
    return {
        "case": f"{name}: {n} segments, payload {plen} B, {slot} B slots"
                f"{', random source alignment' if scattered else ''}",
        "build_kernel": build_kernel, "fill_kernel": fill_kernel,
        **{k: round(v, 2) for k, v in med.items()},
        "spread_us": {k: [round(min(v), 2), round(max(v), 2)] for k, v in times.items()},
        "counted_bytes_read": rd, "counted_bytes_written": wr,
        "build_counted_GBps": round((rd + wr) / med["build_us"] / 1e3, 1),
        "frac_of_pattern": round(med["pattern_us"] / med["build_us"], 3),
        "build_over_fill": round(med["build_us"] / med["fill_us"], 3),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--launches", type=int, default=20, help="launches per timed window")
    ap.add_argument("--warm-seconds", type=float, default=1.0)
    ap.add_argument("--cases", default="mss,mss_odd,jumbo,acks,mss_4096")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the MI355X only")
    cases = {
        "mss": (args.n, 1448, 1536, False, 0),
        "mss_odd": (args.n, 1448, 1536, True, 0),
        "jumbo": (args.n // 2, 8948, 9216, False, 8960),
        "acks": (args.n, 0, 128, False, 0),
        "mss_4096": (4096, 1448, 1536, False, 0),
    }
    line = {
        "tool": "tools/txbuild_bench.py",
        "device": torch.cuda.get_device_name(0),
        "method": f"HIP events around {args.launches} launches, median of {args.rounds} alternating rounds "
                  f"after {args.warm_seconds} s of untimed launches, one process; every frame checked against "
                  "tests/txbuild_model.py first",
        "yardstick": "pattern_us (tools/txbuild_pattern.hip): same loads and stores on the same grid, "
                     "no sums, shifts or shuffles",
        "counted_bytes": "56 + payload_len read and frame_len + 1 written per segment",
    }
    for name in args.cases.split(","):
        line[name] = run(args, name, *cases[name])
        print(f"# {name}: {json.dumps(line[name])}", file=sys.stderr, flush=True)
    text = json.dumps(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
