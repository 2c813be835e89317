#!/usr/bin/env python3
"""Measures the batched application read (SURVEY §8 f17,
mtcp_amd/csrc/rcvread_kernels.hpp) on the MI355X against its yardsticks.

Workload: every stream holds one merged run at a random head_offset and a random
16 B phase of the arena, and one request reads it in full into a destination
range at a random phase.  The run lengths are those the receive copy's bench
leaves (tools/rcvcopy_bench.py: C3's bimodal batch, 1 M frames of 64 B and
1500 B over 65 536 streams, 16 segments a stream), drawn from that distribution
here rather than produced through the chain.  In one process, HIP events around
`launches` launches, median of `rounds` alternating rounds after a second of
untimed launches, per leg:

  (a) read_us     a device copy that puts the records back, then
                  mtcp_gpu_rcvread_dev (clear, claim, plan, scan, copy);
  (b) pattern_us  the same record copy, then tools/rcvread_pattern.hip: the copy
                  units' loads and stores on the copy kernel's grid, no plan, no
                  search, no shift;
  (c) reset_us    the record copy alone;
  (d) memcpy_us   what INTEGRATION §5 prescribes without this row: one
                  hipMemcpyAsync per stream into pinned host memory and one
                  wait each, host wall time over the first `--memcpy-streams`
                  runs, scaled to the leg's streams.

Legs: 65 536 streams of C3's runs; 1 M streams of one segment each; 4 096
requests as one captured launch set; 4 096 streams of which one in 64 holds a
1 MiB run; the 65 536-stream leg with the destination in registered host
memory.  Every output of every leg is compared with the expectation (all
requests READ in full, every destination byte) and a sample of 2 048 requests with
tests/rcvread_model.py before anything is printed.  One JSON line.

    make tools/librcvread_pattern.so
    python tools/rcvread_bench.py [--out profiles/rcvread/bench_rcvread.json]
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


def pattern_lib():
    P = ctypes.CDLL(os.path.join(ROOT, "tools", "librcvread_pattern.so"))
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    P.rcvread_pattern_dev.argtypes = [vp, u32, vp, u64, vp, u64, u32, vp]
    P.rcvread_pattern_dev.restype = ctypes.c_int
    return P


def bimodal(rng, k):
    """Payload bytes of k frames of C3's batch: 64 B and 1500 B frames, 54 B of headers."""
    return np.where(rng.random(k) < 0.5, 10, 1446)


def run(args, P, ctx, name, lens, graph=False, host_dst=False):
    import torch
    from group_bench import timed
    from mtcp_amd import gpu
    from mtcp_amd._lib import lib
    from mtcp_amd._types import RCVREAD_REQ_DTYPE, RCVREAD_RES_DTYPE
    from tests import rcvread_cases as rc
    from tests import rcvread_model as rm

    L, dev = lib(), torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    rng = np.random.default_rng(len(lens))
    n = len(lens)
    heads = rng.integers(0, 64, n)
    sizes = (heads + lens + 2047) // 2048 * 2048
    b = rc.direct(rng, sizes, lens, heads, eff_mss=1448)
    # the requests in a random order of the streams; the destination ranges at random phases, 16-79 bytes apart
    sid = rng.permutation(n).astype(np.int64)
    ln = lens[sid]
    off = np.cumsum(rng.integers(16, 80, n) + ln) - ln
    dst_bytes = int((off[-1] + ln[-1] + 4096 + 15) // 16 * 16)   # the last range must hold MIN(len, size), not copylen
    req = np.zeros(n, RCVREAD_REQ_DTYPE)
    req["sid"], req["len"], req["dst_off"] = sid, 1 << 20, off
    d_req, d_state0, d_rbuf0, d_tx0 = up(req), up(b.state), up(b.rbuf), up(b.tx)
    d_state, d_rbuf, d_tx, d_snd, d_arena = up(b.state), up(b.rbuf), up(b.tx), up(b.snd), up(b.arena)
    d_rres, d_total = torch.zeros(16 * n, dtype=torch.uint8, device=dev), torch.zeros(16, dtype=torch.uint8, device=dev)
    wb = gpu.Context.rcvread_work_bytes(n, n - 1)
    d_work = torch.zeros(wb, dtype=torch.uint8, device=dev)
    if host_dst:
        h_dst = np.zeros(dst_bytes + 64, np.uint8)
        h_dst = h_dst[(-h_dst.ctypes.data) % 64:][:dst_bytes]
        gpu.host_register(h_dst)
        dst_ptr, d_pdst = h_dst.ctypes.data, None
        h_pdst = np.zeros(dst_bytes + 64, np.uint8)
        h_pdst = h_pdst[(-h_pdst.ctypes.data) % 64:][:dst_bytes]
        gpu.host_register(h_pdst)
        pdst_ptr = h_pdst.ctypes.data
    else:
        d_dst = torch.zeros(dst_bytes, dtype=torch.uint8, device=dev)
        d_pdst = torch.zeros(dst_bytes, dtype=torch.uint8, device=dev)
        dst_ptr, pdst_ptr = d_dst.data_ptr(), d_pdst.data_ptr()

    def reset():
        with torch.cuda.stream(st):
            d_state.copy_(d_state0, non_blocking=True)
            d_rbuf.copy_(d_rbuf0, non_blocking=True)
            d_tx.copy_(d_tx0, non_blocking=True)

    def leg_read():
        reset()
        rc_ = L.mtcp_gpu_rcvread_dev(ctx._h, d_req.data_ptr(), n, n - 1, d_state.data_ptr(), d_rbuf.data_ptr(),
                                     d_tx.data_ptr(), d_snd.data_ptr(), d_arena.data_ptr(), len(b.arena), dst_ptr,
                                     dst_bytes, d_rres.data_ptr(), d_total.data_ptr(), d_work.data_ptr(), wb,
                                     st.cuda_stream)
        if rc_ != 0:
            raise SystemExit(f"{name}: mtcp_gpu_rcvread_dev returned {rc_}")

    leg_read()
    st.synchronize()
    # correctness first: nothing is printed for outputs that are wrong
    src = (b.rbuf["data_off"].astype(np.int64) + heads)[sid]
    rres = d_rres.cpu().numpy().view(RCVREAD_RES_DTYPE)
    got_dst = h_dst if host_dst else d_dst.cpu().numpy()
    # every range byte for byte, and the 16 bytes in front of and behind it untouched
    dst_ok = all(got_dst[o:o + k].tobytes() == b.arena[s:s + k].tobytes() and not got_dst[o - 16:o].any() and
                 not got_dst[o + k:o + k + 16].any() for o, s, k in zip(off.tolist(), src.tolist(), ln.tolist()))
    state, rbuf = d_state.cpu().numpy().view(b.state.dtype), d_rbuf.cpu().numpy().view(b.rbuf.dtype)
    ok = (rres["verdict"] == rm.READ).all() and (rres["copylen"] == ln).all() and (rres["sid"] == sid).all() and \
        (rres["rcv_wnd"] == sizes[sid]).all() and (rres["flags"] == np.where(sizes[sid] > 1448, 6, 4)).all() and \
        dst_ok and (state["merged_len"] == 0).all() and (state["nfrag"] == 0).all() and \
        (state["head_seq"] == b.state["head_seq"] + lens.astype(np.uint32)).all() and \
        (rbuf["head_offset"] == heads + lens).all() and (rbuf["last_len"] == 0).all() and \
        d_total.cpu().numpy().view(np.uint64).tolist() == [n, int(lens.sum())]
    pick = np.sort(rng.choice(n, min(n, 2048), replace=False))
    sub = rc.Batch(b.state, b.rbuf, b.tx, b.snd, b.arena)
    sub.req, sub.dst = req[pick], np.zeros(dst_bytes, np.uint8)
    w_state, w_rbuf, w_tx, w_dst, w_rres, _ = sub.expect()
    s_ids = sid[pick]
    ok = ok and rres[pick].tobytes() == w_rres.tobytes() and state[s_ids].tobytes() == w_state[s_ids].tobytes() and \
        rbuf[s_ids].tobytes() == w_rbuf[s_ids].tobytes() and \
        d_tx.cpu().numpy().view(b.tx.dtype)[s_ids].tobytes() == w_tx[s_ids].tobytes()
    for q in sub.req[:256]:
        o, k = int(q["dst_off"]), int(lens[int(q["sid"])])
        ok = ok and (got_dst[o:o + k] == w_dst[o:o + k]).all()
    if not ok:
        raise SystemExit(f"{name}: the read's outputs differ from the model")
    # the pattern's units: as the copy cuts the runs
    first = off >> 4
    pieces = ((off + ln + 15) >> 4) - first
    upr = (pieces + 255) // 256
    r_of = np.repeat(np.arange(n), upr)
    k_of = np.arange(int(upr.sum())) - np.repeat(np.cumsum(upr) - upr, upr)
    units = np.zeros((len(r_of), 4), np.uint32)
    units[:, 0], units[:, 1] = (src[r_of] >> 4) + 256 * k_of, first[r_of] + 256 * k_of
    units[:, 2] = np.minimum(pieces[r_of] - 256 * k_of, 256)
    d_units = up(units)
    cu8 = torch.cuda.get_device_properties(0).multi_processor_count * 8

    def leg_pattern():
        reset()
        if P.rcvread_pattern_dev(d_units.data_ptr(), len(units), d_arena.data_ptr(), len(b.arena), pdst_ptr, dst_bytes,
                                 cu8, st.cuda_stream) != 0:
            raise SystemExit("the pattern kernel did not launch")

    leg_pattern()
    st.synchronize()
    med, spread = timed(args, {"read_us": leg_read, "pattern_us": leg_pattern, "reset_us": reset}, st, graph)
    # INTEGRATION §5 without this row: a copy and a wait per stream
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
    m = min(n, args.memcpy_streams)
    pinned = torch.empty(int(off[m - 1] + ln[m - 1]) + 64, dtype=torch.uint8, pin_memory=True)
    base, abase, sh = pinned.data_ptr(), d_arena.data_ptr(), st.cuda_stream
    srcs, offs, lns = src[:m].tolist(), off[:m].tolist(), ln[:m].tolist()
    walls = []
    for _ in range(3):
        t0 = time.perf_counter()
        for s, o, k in zip(srcs, offs, lns):
            hip.hipMemcpyAsync(base + o, abase + s, k, 2, sh)
            hip.hipStreamSynchronize(sh)
        walls.append((time.perf_counter() - t0) * 1e6 * n / m)
    if pinned.numpy()[offs[0]:offs[0] + lns[0]].tobytes() != b.arena[srcs[0]:srcs[0] + lns[0]].tobytes():
        raise SystemExit(f"{name}: the per-stream copy brought other bytes")
    if host_dst:
        st.synchronize()
        gpu.host_unregister(h_dst), gpu.host_unregister(h_pdst)
    print(f"measured: {name}", file=sys.stderr, flush=True)
    read, pat = med["read_us"] - med["reset_us"], med["pattern_us"] - med["reset_us"]
    nbytes = int(lens.sum())
    return {
        "case": f"{n} streams, {nbytes} bytes, {len(units)} units{', HIP graph' if graph else ''}"
                f"{', destination in registered host memory' if host_dst else ''}",
        "launches_per_window": args.launches, "rounds": args.rounds,
        **{k: round(v, 2) for k, v in med.items()}, "spread_us": spread,
        "read_less_reset_us": round(read, 2), "pattern_less_reset_us": round(pat, 2),
        "frac_of_pattern": round(pat / read, 3),
        "tb_per_s_read_plus_write": round(2 * nbytes / read / 1e6, 3),
        "memcpy_per_stream_us": round(min(walls), 1), "memcpy_spread_us": [round(min(walls), 1), round(max(walls), 1)],
        "memcpy_streams_timed": m, "memcpy_over_read": round(min(walls) / read, 1),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--launches", type=int, default=20, help="launches per timed window")
    ap.add_argument("--warm-seconds", type=float, default=1.0)
    ap.add_argument("--memcpy-streams", type=int, default=4096)
    ap.add_argument("--cases", default="all", help="comma-separated case names, or all")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the MI355X only")
    from mtcp_amd import gpu
    P = pattern_lib()
    line = {
        "tool": "tools/rcvread_bench.py",
        "device": torch.cuda.get_device_name(0),
        "method": f"HIP events around {args.launches} launches, median of {args.rounds} alternating rounds after "
                  f"{args.warm_seconds} s of untimed launches, one process; every timed read and pattern launch is "
                  "preceded by device copies that put the records back (reset_us, subtracted in the ratios); no counter "
                  "or trace run stands behind any figure",
        "yardsticks": "pattern_us (tools/rcvread_pattern.hip): the copy units' loads and stores on the copy kernel's "
                      "grid, no plan, no search, no shift; memcpy_per_stream_us: one hipMemcpyAsync into pinned host "
                      "memory and one wait per stream, host wall time over memcpy_streams_timed runs scaled to the leg, "
                      "best of 3 with the spread",
    }
    want = None if args.cases == "all" else set(args.cases.split(","))
    rng = np.random.default_rng(5)
    c3 = bimodal(rng, 65536 * 16).reshape(65536, 16).sum(axis=1)
    heavy = bimodal(rng, 4096)
    heavy[::64] = 1 << 20
    legs = (("c3_64k_streams", c3, False, False), ("one_segment_1m_streams", bimodal(rng, 1 << 20), False, False),
            ("small_4096_graph", bimodal(rng, 4096 * 16).reshape(4096, 16).sum(axis=1), True, False),
            ("one_in_64_holds_1mib", heavy, False, False), ("c3_64k_streams_host_dst", c3, False, True))
    with gpu.Context(0) as ctx:
        for name, lens, graph, host_dst in legs:
            if want is None or name in want:
                line[name] = run(args, P, ctx, name, lens.astype(np.int64), graph, host_dst)
                if args.out:                          # after every leg: a run that ends early leaves what it measured
                    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                    with open(args.out, "w") as f:
                        f.write(json.dumps(line) + "\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
