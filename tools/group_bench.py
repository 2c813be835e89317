#!/usr/bin/env python3
"""Measures the group passes (mtcp_amd/csrc/group_kernels.hpp)
on the MI355X against their own memory pattern.

Workload: C3's bimodal batch (mtcp_gpu_pktgen_dev) through rx; the records rx
wrote get their 4-tuples replaced by draws from a pool of keys of which the
device flow table holds `flows` (one in sixteen draws is a key it does not
hold: a MISS); the lookup's stream ids are grouped.  In one process, HIP events
around `launches` launches, median of `rounds` alternating rounds after one
second of untimed launches, per case:

  (a) front_us    the rx launch and the lookup launch in front
                  (mtcp_gpu_rx_chunk_dev, mtcp_gpu_flowtab_lookup_dev);
  (b) group_us    the group passes (mtcp_gpu_group_dev: count, scan, emit per
                  digit, then the segment table; or the one workgroup of a
                  batch of at most one tile);
  (c) pattern_us  tools/group_pattern.hip: the same loads and stores per pass
                  on the same grids, pair i stored at position i, no ranking.

Cases: 65 536 streams (max_id 65 535, 17 key bits) and 1 M streams (max_id
1 048 575, 21 key bits), three digits each, from the lookup; the first with half of the batch
rewritten to one stream, and with every id MISS; 4 096 records in one launch
(HIP graph).  Every output of every case is compared with tests/group_model.py
before anything is printed.  One JSON line; frac_of_pattern = c / b,
price_of_front = b / a.  For scale, numpy's stable argsort of the same keys on
one core.  The yardstick is (c), never a figure of the kernels under test.

    make tools/libgroup_pattern.so
    python tools/group_bench.py [--n 1048576] [--out profiles/group/bench_group.json]
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

MISS, NONE = 0xFFFFFFFE, 0xFFFFFFFF


def pattern_lib():
    P = ctypes.CDLL(os.path.join(ROOT, "tools", "libgroup_pattern.so"))
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    P.group_pattern_launch.argtypes = [vp, u32, u32, vp, vp, vp, vp, vp, vp, vp]
    P.group_pattern_launch.restype = ctypes.c_int
    P.group_pattern_sorted_off.argtypes = [u32, u32]
    P.group_pattern_sorted_off.restype = ctypes.c_uint64
    return P


def timed(args, legs, st, graph):
    """Median and spread per leg: alternating rounds of `launches` launches."""
    import torch
    if graph:
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
    t_end = time.monotonic() + args.warm_seconds
    while time.monotonic() < t_end:
        with torch.cuda.stream(st):
            for w in window.values():
                w()
        st.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, w in window.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(st):
                e0.record(st)
                w()
                e1.record(st)
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / args.launches)
    med = {k: statistics.median(v) for k, v in times.items()}
    return med, {k: [round(min(v), 2), round(max(v), 2)] for k, v in times.items()}


class Table:
    """The C3 batch, its rx records with tuples drawn from a key pool, and a
    device table holding `flows` of the pool's keys (ids: a permutation)."""

    def __init__(self, ctx, n, flows, cap_log2):
        import torch
        from mtcp_amd import RESULT_DTYPE, gpu, pktgen
        from tests import flowtab_model as fm
        self.ctx, self.n, self.flows = ctx, n, flows
        self.dev, seed = torch.device("cuda", 0), 42
        rng = np.random.default_rng(flows)
        desc, nbytes = pktgen.layout(n, "bimodal", 6, seed)
        self.d_buf = torch.zeros((nbytes + 15) & ~15, dtype=torch.uint8, device=self.dev)
        self.d_desc = torch.from_numpy(desc.view(np.uint8).copy()).to(self.dev)
        gpu.pktgen_dev(self.d_buf, self.d_desc, n, 6, seed)
        self.d_res = torch.zeros(n * 40, dtype=torch.uint8, device=self.dev)
        ctx.rx_chunk_dev(self.d_buf, self.d_desc, n, 6, self.d_res)
        torch.cuda.synchronize()
        extra = flows // 16 + 16
        pool = np.unique(rng.integers(0, 256, ((flows + extra) * 9 // 8, 12), dtype=np.uint8), axis=0)
        pool = pool[rng.permutation(len(pool))[:flows + extra]]
        ids = rng.permutation(flows).astype(np.uint32)
        res = self.d_res.cpu().numpy().view(RESULT_DTYPE).copy()
        which = np.where(rng.random(n) < 1 / 16, flows + rng.integers(0, extra, n), rng.integers(0, flows, n))
        e = fm.entries(pool[which], 0)
        res["daddr"], res["saddr"], res["dport"], res["sport"] = e["saddr"], e["daddr"], e["sport"], e["dport"]
        self.d_look = torch.from_numpy(res.view(np.uint8).copy()).to(self.dev)
        self.want_sid = np.where(which < flows, ids[np.minimum(which, flows - 1)], MISS).astype(np.uint32)
        self.want_sid[res["verdict"] != 0] = NONE
        self.tab = gpu.FlowTable(ctx, cap_log2)
        self.tab.update(ins=fm.entries(pool[:flows], ids))
        st = self.tab.stats()
        if st != {"live": flows, "tombs": 0, "insert_failed": 0, "remove_missed": 0}:
            raise SystemExit(f"the table's counters are wrong: {st}")

    def close(self):
        self.tab.close()


def run(args, P, t, n, max_id, shape, graph):
    import torch
    from mtcp_amd import gpu
    from tests import group_model as gm

    ctx, dev = t.ctx, t.dev
    st = torch.cuda.Stream(device=dev)
    h = st.cuda_stream
    mk = lambda b: torch.zeros(max(b, 16), dtype=torch.uint8, device=dev)
    d_sid = mk(4 * n)
    t.tab.lookup_dev(t.d_look, n, d_sid, None, stream=st)
    st.synchronize()
    sid = d_sid.cpu().numpy().view(np.uint32)[:n].copy()
    if not np.array_equal(sid, t.want_sid[:n]):
        raise SystemExit("the lookup's answers differ from the construction")
    rng = np.random.default_rng(n)
    if shape == "half_one_stream":
        sid = np.where(rng.random(n) < 0.5, 7, sid).astype(np.uint32)
    elif shape == "all_miss":
        sid = np.full(n, MISS, np.uint32)
    g_sid = torch.from_numpy(sid.view(np.uint8).copy()).to(dev)      # what the group legs read
    wb = gpu.Context.group_work_bytes(n, max_id)
    d_idx, d_ssid, d_sstart, d_nseg, d_work = mk(4 * n), mk(4 * n), mk(4 * n + 4), mk(4), mk(wb)
    p_idx, p_ssid, p_sstart, p_nseg, p_work = mk(4 * n), mk(4 * n), mk(4 * n + 4), mk(4), mk(wb)
    tiled = n > gpu.Context.group_tile()
    sorted_ptr = d_work.data_ptr() + P.group_pattern_sorted_off(n, max_id) if tiled else None
    d_look_sid = mk(4 * n)

    def leg_front():
        ctx.rx_chunk_dev(t.d_buf, t.d_desc, n, 6, t.d_res, stream=st)
        t.tab.lookup_dev(t.d_look, n, d_look_sid, None, stream=st)

    def leg_group():
        ctx.group_dev(g_sid, n, max_id, d_idx, d_ssid, d_sstart, d_nseg, d_work, stream=st)

    def leg_pattern():
        if P.group_pattern_launch(g_sid.data_ptr(), n, max_id, p_idx.data_ptr(), p_ssid.data_ptr(),
                                  p_sstart.data_ptr(), p_nseg.data_ptr(), p_work.data_ptr(), sorted_ptr, h) != 0:
            raise SystemExit("the pattern kernels did not launch")

    legs = {"front_us": leg_front, "group_us": leg_group, "pattern_us": leg_pattern}
    for f in legs.values():
        f()
    st.synchronize()
    # correctness first: nothing is printed for lists that are wrong
    want_idx, want_ssid, want_sstart = gm.group(sid, max_id)
    m = int(d_nseg.cpu().numpy().view(np.uint32)[0])
    u32 = lambda x, k: x.cpu().numpy().view(np.uint32)[:k]
    if m != len(want_ssid) or not np.array_equal(u32(d_idx, n), want_idx) or \
            not np.array_equal(u32(d_ssid, m), want_ssid) or not np.array_equal(u32(d_sstart, m + 1), want_sstart):
        raise SystemExit("the lists differ from the model")
    med, spread = timed(args, legs, st, graph)
    key_bits = (max_id + 2).bit_length()
    passes = -(-key_bits // 8)
    return {
        "case": f"{n} ids, max_id {max_id}, {shape}{', HIP graph' if graph else ''}",
        "key_bits": key_bits, "digits": passes,
        "launches_per_group": 3 * passes + 3 if tiled else 1,
        **{k: round(v, 2) for k, v in med.items()},
        "spread_us": spread,
        "segments": m,
        "frac_of_pattern": round(med["pattern_us"] / med["group_us"], 3),
        "price_of_front": round(med["group_us"] / med["front_us"], 3),
    }, sid


def cpu_figure(sid, max_id, reps=3):
    """numpy's stable argsort of the mapped keys (one core): what the model
    does, not mTCP code."""
    from tests import group_model as gm
    k = gm.key(sid, max_id).astype(np.uint32)
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        np.argsort(k, kind="stable")
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
    from mtcp_amd import gpu
    P = pattern_lib()
    line = {
        "tool": "tools/group_bench.py",
        "device": torch.cuda.get_device_name(0),
        "method": f"HIP events around {args.launches} launches, median of {args.rounds} alternating rounds "
                  f"after {args.warm_seconds} s of untimed launches, one process",
        "yardstick": "pattern_us (tools/group_pattern.hip): same loads and stores per pass on the same grids, "
                     "pair i at position i, no ranking",
    }
    with gpu.Context(0) as ctx:
        t = Table(ctx, args.n, 65536, 17)
        line["c3_64k_streams"], sid = run(args, P, t, args.n, 65535, "lookup", False)
        line["c3_half_one_stream"], _ = run(args, P, t, args.n, 65535, "half_one_stream", False)
        line["c3_all_miss"], _ = run(args, P, t, args.n, 65535, "all_miss", False)
        line["small_4096_graph"], _ = run(args, P, t, 4096, 65535, "lookup", True)
        t.close()
        line["cpu_numpy_stable_argsort_1core_us"] = cpu_figure(sid, 65535)
        line["cpu_note"] = f"np.argsort(kind='stable') of the {len(sid)} u32 keys of c3_64k_streams, best of 3, one core"
        flows = 1 << 20
        t = Table(ctx, args.n, flows, 21)
        line["c3_1m_streams"], _ = run(args, P, t, args.n, flows - 1, "lookup", False)
        t.close()
    text = json.dumps(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
