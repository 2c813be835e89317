#!/usr/bin/env python3
"""Measures the receive copy (mtcp_amd/csrc/rcvcopy_kernels.hpp)
on the MI355X against its yardsticks.

Workload: the batch of tools/rcvwalk_bench.py (C3's bimodal frames through rx,
tuples from a pool the device flow table holds, looked up, grouped, sequence
numbers rewritten per stream) walked by mtcp_gpu_rcvwalk_dev; the copy's inputs
are the walk's own placement records.  Every stream has a receive buffer in one
arena that holds its share.  In one process, HIP events around `launches`
launches, median of `rounds` alternating rounds after a second of untimed
launches, per case:

  (a) front_us    the rx, lookup, group and walk launches in front (the walk
                  with the device copy that puts its state array back);
  (b) copy_us     a device copy that puts the buffer records back, then
                  mtcp_gpu_rcvcopy_dev (prep, plan, front, ordered);
  (c) pattern_us  the same record copy, then tools/rcvcopy_pattern.hip: the
                  loads and stores of the copyable packets on the front
                  kernel's grid and the destination's grid, no plan, no shift,
                  no ordering;
  (d) reset_us    the record copy alone;
  (e) host_us     one host core doing the same copies with memcpy from the
                  staged frames, best of 3 and the spread (a shared host).

Cases: 65 536 streams in order, one segment in eight delayed, 1 M streams, one
segment in eight a retransmission that overlaps its predecessor, half the
streams compacting a 1 KiB window, 4 096 records as one captured launch set,
half the batch one stream.  Every output of every case is compared with
tests/rcvcopy_model.py before anything is printed.  One JSON line.

    make tools/librcvcopy_pattern.so tools/librcvwalk_pattern.so tools/libgroup_pattern.so
    python tools/rcvcopy_bench.py [--n 1048576] [--out profiles/rcvcopy/bench_rcvcopy.json]
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

WINDOW = 1024                                          # the compacting streams' bytes of before the batch


def pattern_lib():
    P = ctypes.CDLL(os.path.join(ROOT, "tools", "librcvcopy_pattern.so"))
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    P.rcvcopy_pattern_dev.argtypes = [vp, u64, vp, u32, vp, u64, ctypes.c_int, vp]
    P.rcvcopy_pattern_dev.restype = ctypes.c_int
    P.rcvcopy_group_of.argtypes = [u64, u32]
    P.rcvcopy_group_of.restype = ctypes.c_int
    P.rcvcopy_host_memcpy.argtypes = [vp, vp, vp, vp, u32, vp]
    P.rcvcopy_host_memcpy.restype = None
    return P


def retransmit(res, sid, max_id, rng):
    """One segment in eight (never a stream's first) starts up to 64 bytes
    inside its predecessor; what follows moves down with it, so the stream
    stays in order."""
    n = len(res)
    on = sid <= max_id
    order = np.argsort(np.where(on, sid, max_id + 1), kind="stable")
    s = sid[order]
    first = np.ones(n, bool)
    first[1:] = s[1:] != s[:-1]
    ln = res["payload_len"][order].astype(np.int64)
    prev = np.concatenate([[0], ln[:-1]])
    k = np.where((rng.random(n) < 1 / 8) & ~first & on[order], np.minimum(np.minimum(prev, ln), 64), 0)
    shift = np.cumsum(k)
    shift -= np.maximum.accumulate(np.where(first, shift, 0))       # k is 0 at a stream's first packet
    out = res.copy()
    out["seq"][order] = (res["seq"][order].astype(np.int64) - shift) & 0xFFFFFFFF
    return out


def delay(res, desc, sid, max_id, rng):
    """One segment in eight changes places with one 1-8 places later in its
    stream's list: the records and the descriptors move together, the frames
    stay where they are."""
    n = len(res)
    on = sid <= max_id
    order = np.argsort(np.where(on, sid, max_id + 1), kind="stable")
    s = sid[order]
    a = np.nonzero((rng.random(n) < 1 / 8) & on[order])[0]
    b = np.minimum(a + rng.integers(1, 9, len(a)), n - 1)
    perm = np.arange(n)
    for x, y in zip(a.tolist(), b.tolist()):
        if s[x] == s[y]:
            perm[x], perm[y] = perm[y], perm[x]
    out_res, out_desc = res.copy(), desc.copy()
    out_res[order], out_desc[order] = res[order[perm]], desc[order[perm]]
    return out_res, out_desc


def run(args, P, t, n, max_id, shape, graph, launches=None, rounds=None):
    import torch
    from group_bench import timed
    from rcvwalk_bench import walk_inputs
    from mtcp_amd import gpu
    from mtcp_amd._types import DESC_DTYPE, RCV_BUF_DTYPE, RCV_PLACE_DTYPE, RESULT_DTYPE
    from tests import rcvcopy_model as cm

    ctx, dev = t.ctx, t.dev
    st = torch.cuda.Stream(device=dev)
    mk = lambda b: torch.zeros(max(b, 16), dtype=torch.uint8, device=dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    rng = np.random.default_rng(n + max_id)
    sid = t.want_sid[:n].copy()
    if shape == "half_one_stream":
        sid = np.where((rng.random(n) < 0.5) & (sid <= max_id), 7, sid).astype(np.uint32)
    res0 = t.d_look.cpu().numpy().view(RESULT_DTYPE)[:n]
    res, opt, state = walk_inputs(res0, sid, max_id, False, rng)
    desc = t.d_desc.cpu().numpy().view(DESC_DTYPE)[:n].copy()
    if shape == "retransmitted":
        res = retransmit(res, sid, max_id, rng)
    if shape == "delayed":
        res, desc = delay(res, desc, sid, max_id, rng)
    d_desc = up(desc)
    # the buffers: each holds its stream's share; the compacting ones a window in front and head_offset > 0
    total = np.zeros(max_id + 2, np.int64)
    np.add.at(total, np.where(sid <= max_id, sid, max_id + 1), res["payload_len"].astype(np.int64))
    total = total[:-1]
    compacting = (np.arange(max_id + 1) % 2 == 0) & (total > 0) if shape == "half_compacting" else np.zeros(max_id + 1, bool)
    head = np.where(compacting, rng.integers(1, 65, max_id + 1), 0)
    window = np.where(compacting, WINDOW, 0)
    size = np.where(compacting, head + window + total, (np.maximum(total, 1) + 2047) // 2048 * 2048)
    if size.max() > 1 << 30:
        raise SystemExit("a stream's share does not fit the largest buffer")
    state["size"] = size
    state["merged_len"] = window
    state["head_seq"] = state["rcv_nxt"] - window.astype(np.uint32)
    state["rcv_wnd"] = size - window
    state["nfrag"] = compacting
    state["frag"]["seq"][:, 0] = np.where(compacting, state["head_seq"], 0)
    state["frag"]["len"][:, 0] = window
    rbuf = np.zeros(max_id + 1, RCV_BUF_DTYPE)
    pitch = (size + 64 + 15) // 16 * 16 + rng.integers(0, 16, max_id + 1)      # data_off at any alignment
    rbuf["data_off"] = 64 + np.cumsum(pitch) - pitch
    rbuf["size"], rbuf["head_offset"], rbuf["tail_offset"], rbuf["last_len"] = size, head, head + window, window
    arena_bytes = int((rbuf["data_off"][-1] + size[-1] + 64 + 15) // 16 * 16)
    d_sid, d_res, d_opt, d_state0, d_rbuf0 = up(sid), up(res), up(opt), up(state), up(rbuf)
    gwb, wwb = gpu.Context.group_work_bytes(n, max_id), gpu.Context.rcvwalk_work_bytes(n, max_id)
    cwb = gpu.Context.rcvcopy_work_bytes(n, max_id)
    d_idx, d_ssid, d_sstart, d_nseg, d_gwork = mk(4 * n), mk(4 * n), mk(4 * n + 4), mk(4), mk(gwb)
    d_look_sid, d_state, d_place, d_stop, d_wwork = mk(4 * n), mk(64 * (max_id + 1)), mk(16 * n), mk(4 * n), mk(wwb)
    d_rbuf, d_cstat, d_cwork = mk(32 * (max_id + 1)), mk(n), mk(cwb)
    d_arena = torch.full((arena_bytes,), 0x5A, dtype=torch.uint8, device=dev)
    d_parena = torch.zeros(arena_bytes, dtype=torch.uint8, device=dev)
    buf_len = t.d_buf.numel()

    def leg_front():
        ctx.rx_chunk_dev(t.d_buf, t.d_desc, n, 6, t.d_res, stream=st)
        t.tab.lookup_dev(t.d_look, n, d_look_sid, None, stream=st)
        ctx.group_dev(d_sid, n, max_id, d_idx, d_ssid, d_sstart, d_nseg, d_gwork, stream=st)
        with torch.cuda.stream(st):
            d_state.copy_(d_state0, non_blocking=True)
        ctx.rcvwalk_dev(d_res, d_opt, n, max_id, d_idx, d_ssid, d_sstart, d_nseg, d_state, d_place, d_stop, d_wwork,
                        stream=st)

    def reset():
        with torch.cuda.stream(st):
            d_rbuf.copy_(d_rbuf0, non_blocking=True)

    def leg_copy():
        reset()
        ctx.rcvcopy_dev(t.d_buf, d_desc, 6, d_res, d_place, n, max_id, d_idx, d_ssid, d_sstart, d_nseg, d_stop,
                        d_rbuf, d_arena, d_cstat, d_cwork, stream=st)

    leg_front()
    st.synchronize()
    # correctness first: nothing is printed for outputs that are wrong
    m = int(d_nseg.cpu().numpy().view(np.uint32)[0])
    u32 = lambda x, k: x.cpu().numpy().view(np.uint32)[:k].copy()
    idx, ssid, sstart, stop = u32(d_idx, n), u32(d_ssid, m), u32(d_sstart, m + 1), u32(d_stop, m)
    place = d_place.cpu().numpy().view(RCV_PLACE_DTYPE)[:n].copy()
    buf = t.d_buf.cpu().numpy()
    arena0 = np.full(arena_bytes, 0x5A, np.uint8)
    w_arena, w_rbuf, w_cstat, mask, info = cm.copy(buf, desc, 6, res, place, max_id, idx, ssid, sstart, stop, rbuf, arena0)
    leg_copy()
    st.synchronize()
    if d_cstat.cpu().numpy()[:n].tobytes() != w_cstat.tobytes() or \
            d_rbuf.cpu().numpy()[:32 * (max_id + 1)].tobytes() != w_rbuf.tobytes() or \
            ((d_arena.cpu().numpy() != w_arena) & mask).any():
        raise SystemExit(f"{shape}: the copy's outputs differ from the model")
    # the copies as the pattern and the host core take them: list order, final places
    copied = (w_cstat == cm.FRONT) | (w_cstat == cm.ORDERED)
    ihl_doff = res["ihl_doff"].astype(np.int64)
    src = (desc["offset"].astype(np.int64) << 6) + 14 + 4 * ((ihl_doff & 15) + (ihl_doff >> 4))
    s_of = np.minimum(sid, max_id).astype(np.int64)
    dst = w_rbuf["data_off"][s_of].astype(np.int64) + w_rbuf["head_offset"][s_of] + place["put_off"]
    ln = np.where(copied, place["put_len"], 0).astype(np.int64)
    p_of = np.minimum(idx, n - 1)
    l_src, l_dst, l_len = src[p_of], np.where(ln[p_of] > 0, dst[p_of], 0), ln[p_of]
    runs = np.zeros((n, 4), np.uint32)
    runs[:, 0], runs[:, 1], runs[:, 2] = l_src & 0xFFFFFFFF, l_src >> 32, l_dst >> 4
    runs[:, 3] = np.where(l_len > 0, ((l_dst + l_len + 15) >> 4) - (l_dst >> 4), 0)
    d_runs = up(runs)
    group = P.rcvcopy_group_of(buf_len, n)

    def leg_pattern():
        reset()
        if P.rcvcopy_pattern_dev(t.d_buf.data_ptr(), buf_len, d_runs.data_ptr(), n, d_parena.data_ptr(), arena_bytes, group,
                                 st.cuda_stream) != 0:
            raise SystemExit("the pattern kernel did not launch")

    leg_pattern()
    st.synchronize()
    a = argparse.Namespace(**vars(args))
    a.launches, a.rounds = launches or args.launches, rounds or args.rounds
    legs = {"front_us": leg_front, "copy_us": leg_copy, "pattern_us": leg_pattern, "reset_us": reset}
    med, spread = timed(a, legs, st, graph)
    host, h_arena = [], np.zeros(arena_bytes, np.uint8)
    a_src, a_dst, a_len = (np.ascontiguousarray(x) for x in (l_src.astype(np.uint64), l_dst.astype(np.uint64), l_len.astype(np.uint32)))
    for _ in range(3):
        t0 = time.perf_counter()
        P.rcvcopy_host_memcpy(buf.ctypes.data, a_src.ctypes.data, a_dst.ctypes.data, a_len.ctypes.data, n, h_arena.ctypes.data)
        host.append((time.perf_counter() - t0) * 1e6)
    print(f"measured: {n} records, max_id {max_id}, {shape}", file=sys.stderr, flush=True)
    copy, pat = med["copy_us"] - med["reset_us"], med["pattern_us"] - med["reset_us"]
    nbytes = int(ln.sum())
    seg_len = np.diff(sstart.astype(np.int64))[ssid <= max_id]
    return {
        "case": f"{n} records, max_id {max_id}, {shape}{', HIP graph' if graph else ''}",
        "launches_per_window": a.launches, "rounds": a.rounds, "group_width": group,
        **{k: round(v, 2) for k, v in med.items()},
        "spread_us": spread,
        "host_us": round(min(host), 1), "host_spread_us": [round(min(host), 1), round(max(host), 1)],
        "stream_segments": int(len(seg_len)), "longest_segment": int(seg_len.max()) if len(seg_len) else 0,
        "status": {k: int(c) for k, c in zip(("NONE", "FRONT", "ORDERED", "BAD_BUF", "BAD_SRC", "BAD_RANGE"), info["classes"])},
        "streams_compacted": info["compacted"],
        "share_ordered": round(float(info["classes"][cm.ORDERED]) / max(int(copied.sum()), 1), 4),
        "payload_bytes": nbytes,
        "copy_less_reset_us": round(copy, 2),
        "frac_of_pattern": round(pat / copy, 3),
        "tb_per_s_read_plus_write": round(2 * nbytes / copy / 1e6, 3),
        "share_of_8_tb_per_s": round(2 * nbytes / copy / 1e6 / 8, 3),
        "price_of_front": round(copy / med["front_us"], 3),
        "host_over_copy": round(min(host) / copy, 2),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=10, help="launches per timed window")
    ap.add_argument("--warm-seconds", type=float, default=1.0)
    ap.add_argument("--cases", default="all", help="comma-separated case names, or all")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the MI355X only")
    from group_bench import Table
    from mtcp_amd import gpu
    P = pattern_lib()
    line = {
        "tool": "tools/rcvcopy_bench.py",
        "device": torch.cuda.get_device_name(0),
        "method": f"HIP events around {args.launches} launches (2 for the heavy stream), median of {args.rounds} "
                  f"alternating rounds (5 for the heavy stream) after {args.warm_seconds} s of untimed launches, one "
                  "process; every timed copy and pattern launch is preceded by a device copy that puts the buffer "
                  "records back (reset_us, subtracted in the ratios); no counter or trace run stands behind any figure",
        "yardsticks": "pattern_us (tools/rcvcopy_pattern.hip): the copyable packets' loads and stores on the same grids, "
                      "no plan, no shift, no ordering; front_us: rx, lookup, group and walk; host_us: one host core, "
                      "memcpy from the staged frames, best of 3 with the spread; 8 TB/s counts read plus write",
    }
    want = None if args.cases == "all" else set(args.cases.split(","))
    on = lambda name: want is None or name in want

    def save():                                            # after every case: a long run that ends early leaves what it measured
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(line) + "\n")
    with gpu.Context(0) as ctx:
        t = Table(ctx, args.n, 65536, 17)
        for name, shape, graph, n, lr in (("c3_64k_streams_in_order", "in_order", False, args.n, (None, None)),
                                          ("c3_64k_streams_delayed", "delayed", False, args.n, (None, None)),
                                          ("c3_64k_streams_retransmitted", "retransmitted", False, args.n, (None, None)),
                                          ("c3_64k_streams_half_compacting", "half_compacting", False, args.n, (None, None)),
                                          ("c3_half_one_stream", "half_one_stream", False, args.n, (2, 5)),
                                          ("small_4096_graph", "in_order", True, 4096, (None, None))):
            if on(name):
                line[name] = run(args, P, t, n, 65535, shape, graph, *lr)
                save()
        t.close()
        if on("c3_1m_streams"):
            flows = 1 << 20
            t = Table(ctx, args.n, flows, 21)
            line["c3_1m_streams"] = run(args, P, t, args.n, flows - 1, "in_order", False)
            t.close()
    save()
    print(json.dumps(line))


if __name__ == "__main__":
    main()
