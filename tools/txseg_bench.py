#!/usr/bin/env python3
"""Measures the segment passes (mtcp_amd/csrc/txseg_kernels.hpp)
on the MI355X against their own memory pattern, against the build launch that
follows them and against one host core writing the same records.

In one process, HIP events around `launches` launches, median of `rounds`
alternating rounds after one second of untimed launches, per case:

  (a) build_us    mtcp_gpu_tx_build_dev over the seg_cap records just written;
  (b) segment_us  mtcp_gpu_tx_segment_dev: bursts in; records, descriptors,
                  results and totals out (all its launches);
  (c) pattern_us  tools/txseg_pattern.hip: the same loads and stores on the
                  same grids, no arithmetic, no search;
      host_us     one core, a plain C loop that writes the same records and
                  descriptors (tools/txseg_pattern.hip txseg_host_loop; wall
                  clock, median of 5 runs after one).

Cases (about `--n` segments each, packed 64 B aligned slots, seg_cap = the
total rounded up to 1 024):
  bursts_64k   64 KiB bursts at mss 1460 (46 segments each)
  single       one-segment bursts of 1..1448 B
  loguniform   burst lengths log-uniform from 1 B to 256 KiB
  stopped      64 KiB bursts, a quarter of them stopped by their window
  one_wg       4 096 records from 89 bursts: the one-workgroup form

Every record, descriptor, result and total of every case is compared with the
model (tests/txseg_model.py: FlushTCPSendingBuffer's loop restated literally),
the host loop's records too, and the builder's status bytes must all be BUILT,
before anything is printed.  One JSON line: the times, frac_of_pattern = c / b,
segment_over_build = b / a, the upload a caller saves (56 B per segment
against 64 B per burst) and the fan-out.

    make tools/libtxseg_pattern.so
    python tools/txseg_bench.py [--out profiles/txseg/bench_txseg.json]
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

PAYLOAD_BYTES = 64 << 20
OFF_SHIFT = 6


def make_case(name, n_seg, seed=3):
    from tests import txseg_model as m
    rng = np.random.default_rng(seed)
    if name in ("bursts_64k", "stopped", "one_wg"):
        n = 89 if name == "one_wg" else max(1, n_seg // 46)
        ln = np.full(n, 65536, dtype=np.int64)
    elif name == "single":
        n = n_seg
        ln = rng.integers(1, 1449, n)
    elif name == "loguniform":
        mean_segs = 15.6                                   # of these lengths at 1 448 B per segment
        n = max(1, int(n_seg / mean_segs))
        ln = np.exp(rng.uniform(0, np.log(256 << 10), n)).astype(np.int64)
    else:
        raise SystemExit(f"unknown case {name}")
    b = m.random_bursts(n, seed, PAYLOAD_BYTES, n_links=4, mss_choices=(1460,), p_stop=0, p_empty=0)
    b["len"] = ln
    b["payload_off"] = rng.integers(0, PAYLOAD_BYTES - (256 << 10), n)
    window = b["in_flight"].astype(np.int64) + ln
    if name == "stopped":
        stopped = np.arange(n) % 4 == 1
        window[stopped] -= (ln[stopped] * rng.random(int(stopped.sum()))).astype(np.int64)
    b["window"] = b["peer_wnd"] = window
    return b


def differ(name, got, want):
    if got.tobytes() == want.tobytes():
        return
    size = want.dtype.itemsize
    a, b = got.view(np.uint8).reshape(-1, size), want.view(np.uint8).reshape(-1, size)
    i = int(np.flatnonzero((a != b).any(axis=1))[0])
    raise SystemExit(f"{name} differ from the model first at {i}: {got.view(want.dtype)[i]} against {want[i]}")


def run(args, name):
    import torch
    from mtcp_amd import DESC_DTYPE, TX_BURST_DTYPE, TX_BURST_RESULT_DTYPE, TX_LINK_DTYPE, TX_SEG_DTYPE, gpu
    from tests import txseg_model as m
    dev = torch.device("cuda", 0)
    bursts = make_case(name, 4096 if name == "one_wg" else args.n)
    n = len(bursts)
    roomy = dict(payload_bytes=PAYLOAD_BYTES, n_links=4, buf_off=0, buf_len=1 << 40, off_shift=OFF_SHIFT, slot_bytes=0,
                 max_mss=0)
    # the host plan only sizes seg_cap and the frame buffer
    _, total0 = gpu.Context.tx_segment_plan(bursts.astype(TX_BURST_DTYPE), PAYLOAD_BYTES, 4, 0, 1 << 40, OFF_SHIFT,
                                               0, 1 << 26)
    cap = 4096 if name == "one_wg" else (int(total0[0]) + 1023) // 1024 * 1024
    buf_len = (int(total0[1]) + 4095) // 4096 * 4096
    kw = dict(roomy, buf_len=buf_len, seg_cap=cap)
    t0 = time.monotonic()
    want = m.expand(bursts, **kw)                       # the model, not the plan, is what the outputs are held to
    model_s = time.monotonic() - t0
    k = int(want[3][0])
    rng = np.random.default_rng(5)
    links = np.zeros(4, TX_LINK_DTYPE)
    links["dst"], links["src"] = rng.integers(0, 256, (4, 6)), rng.integers(0, 256, (4, 6))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    d_burst, d_links = up(bursts), up(links)
    g = torch.Generator(device=dev).manual_seed(5)
    d_payload = torch.randint(0, 256, (PAYLOAD_BYTES,), dtype=torch.uint8, device=dev, generator=g)
    d_buf = torch.zeros(buf_len, dtype=torch.uint8, device=dev)
    mk = lambda nbytes: torch.full((max(nbytes, 16),), 0xA5, dtype=torch.uint8, device=dev)
    d_seg, d_desc, d_res, d_total, d_status = mk(48 * cap), mk(8 * cap), mk(16 * n), mk(16), mk(cap)
    p_seg, p_desc, p_res, p_total = mk(48 * cap), mk(8 * cap), mk(16 * n), mk(16)
    wbytes = gpu.Context.tx_segment_work_bytes(n)
    d_work, p_work = mk(wbytes), mk(wbytes)
    lib = ctypes.CDLL(os.path.join(ROOT, "tools", "libtxseg_pattern.so"))
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    P = lib.txseg_pattern_launch
    P.argtypes, P.restype = [vp, u32, vp, vp, u32, vp, vp, vp, vp], ctypes.c_int
    H = lib.txseg_host_loop
    H.argtypes, H.restype = [vp, u32, u64, u32, vp, vp], u64
    st = torch.cuda.Stream(device=dev)
    h = st.cuda_stream
    torch.cuda.synchronize()                 # the fills above run on another stream than the legs

    def check(ctx):
        st.synchronize()
        differ("records", d_seg.cpu().numpy()[:48 * cap].view(TX_SEG_DTYPE), want[0].astype(TX_SEG_DTYPE))
        differ("descriptors", d_desc.cpu().numpy()[:8 * cap].view(DESC_DTYPE), want[1].astype(DESC_DTYPE))
        differ("results", d_res.cpu().numpy()[:16 * n].view(TX_BURST_RESULT_DTYPE),
               want[2].astype(TX_BURST_RESULT_DTYPE))
        differ("totals", d_total.cpu().numpy()[:16].view(np.uint64), want[3])

    with gpu.Context(0) as ctx:
        def leg_segment():
            ctx.tx_segment_dev(d_burst, n, PAYLOAD_BYTES, 4, 0, buf_len, OFF_SHIFT, 0, d_seg, d_desc, cap, d_res,
                               d_total, d_work, stream=st)

        def leg_pattern():
            if P(d_burst.data_ptr(), n, p_seg.data_ptr(), p_desc.data_ptr(), cap, p_res.data_ptr(),
                 p_total.data_ptr(), p_work.data_ptr(), h) != 0:
                raise SystemExit("the pattern kernels did not launch")

        def leg_build():
            ctx.tx_build_dev(d_seg, cap, d_payload, d_links, d_buf, d_desc, OFF_SHIFT, d_status, stream=st)

        leg_segment()
        seg_kernel = ctx.last_kernel
        check(ctx)                                              # nothing is printed for wrong records
        leg_build()
        st.synchronize()
        build_kernel = ctx.last_kernel
        status = d_status.cpu().numpy()[:cap]
        if status[:k].any() or not (status[k:] == 1).all():
            raise SystemExit("the builder did not build exactly the emitted records")
        legs = {"segment_us": leg_segment, "pattern_us": leg_pattern, "build_us": leg_build}
        for f in legs.values():
            f()
        st.synchronize()

        def many(f):
            def go():
                for _ in range(args.launches):
                    f()
            return go
        window = {key: many(f) for key, f in legs.items()}
        t_end = time.monotonic() + args.warm_seconds            # untimed launches first
        while time.monotonic() < t_end:
            for w in window.values():
                w()
            st.synchronize()
        times = {key: [] for key in legs}
        for _ in range(args.rounds):                            # alternating: b, c, a, b, c, a, ...
            for key, w in window.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                w()
                e1.record(st)
                e1.synchronize()
                times[key].append(e0.elapsed_time(e1) * 1e3 / args.launches)
        leg_segment()                                           # after the timed launches: still the model's
        check(ctx)
    # one host core, the same records
    hb = np.ascontiguousarray(bursts.astype(TX_BURST_DTYPE))
    h_seg, h_desc = np.zeros(cap, TX_SEG_DTYPE), np.zeros(cap, DESC_DTYPE)
    host = []
    for i in range(6):
        t0 = time.perf_counter()
        wrote = H(hb.ctypes.data, n, 0, OFF_SHIFT, h_seg.ctypes.data, h_desc.ctypes.data)
        host.append((time.perf_counter() - t0) * 1e6)
    if wrote != k:
        raise SystemExit(f"the host loop wrote {wrote} records, the model {k}")
    differ("host records", h_seg[:k], want[0][:k].astype(TX_SEG_DTYPE))
    differ("host descriptors", h_desc[:k], want[1][:k].astype(DESC_DTYPE))
    med = {key: statistics.median(v) for key, v in times.items()}
    host_us = statistics.median(host[1:])
    return {
        "case": f"{name}: {n} bursts, {k} segments, seg_cap {cap}",
        "segment_kernel": seg_kernel, "build_kernel": build_kernel,
        "fan_out": round(k / n, 2),
        **{key: round(v, 2) for key, v in med.items()},
        "spread_us": {key: [round(min(v), 2), round(max(v), 2)] for key, v in times.items()},
        "frac_of_pattern": round(med["pattern_us"] / med["segment_us"], 3),
        "segment_over_build": round(med["segment_us"] / med["build_us"], 3),
        "segment_ns_per_segment": round(med["segment_us"] * 1e3 / max(k, 1), 3),
        "host_us": round(host_us, 1), "host_spread_us": [round(min(host[1:]), 1), round(max(host[1:]), 1)],
        "host_ns_per_segment": round(host_us * 1e3 / max(k, 1), 2),
        "upload_bytes_records": 56 * k, "upload_bytes_bursts": 64 * n, "upload_bytes_saved": 56 * k - 64 * n,
        "model_seconds": round(model_s, 1),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1 << 20, help="segments per case")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--launches", type=int, default=20, help="launches per timed window")
    ap.add_argument("--warm-seconds", type=float, default=1.0)
    ap.add_argument("--cases", default="bursts_64k,single,loguniform,stopped,one_wg")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the MI355X only")
    line = {
        "tool": "tools/txseg_bench.py",
        "device": torch.cuda.get_device_name(0),
        "method": f"HIP events around {args.launches} launches, median of {args.rounds} alternating rounds "
                  f"after {args.warm_seconds} s of untimed launches, one process; every record, descriptor, result "
                  "and total checked against tests/txseg_model.py first; host_us: wall clock of one core's plain "
                  "C loop, median of 5",
        "yardstick": "pattern_us (tools/txseg_pattern.hip): same loads and stores on the same grids, "
                     "no arithmetic, no search",
    }
    for name in args.cases.split(","):
        line[name] = run(args, name)
        print(f"# {name}: {json.dumps(line[name])}", file=sys.stderr, flush=True)
    text = json.dumps(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
