#!/usr/bin/env python3
"""Measures the device flow table (mtcp_amd/csrc/
flowtab_kernels.hpp) on the MI355X against its own memory pattern.

Workload: C3's bimodal batch (mtcp_gpu_pktgen_dev) through rx; the records rx
wrote get their 4-tuples replaced by draws from a pool of 2 x `flows` keys, of
which the table holds the first half (about half of the TCP_OK records hit).
In one process, HIP events around `launches` launches, median of `rounds`
alternating rounds after one second of untimed launches, per case:

  (a) rx_us       the rx launch in front (mtcp_gpu_rx_chunk_dev);
  (b) lookup_us   mtcp_gpu_flowtab_lookup_dev (sid and bins written);
  (c) pattern_us  tools/flowtab_pattern.hip: the same record loads on the same
                  grid, one 16 B gather at a pseudo-random slot per TCP_OK
                  record, the same stores; no hashing, comparing or probing;
  group_us        the lookup kernel with 1, 2 and 4 slots loaded per probe
                  step on an identical table image (the library ships one of
                  them: "group" in the output).

Cases: tables of 65 536 flows (cap 2^17) and 1 M flows (cap 2^21), each fresh
and after churn has left a quarter of the slots TOMB; 4 096 records in one
launch (HIP graph); and an update of 64 K removes plus 64 K inserts (no
pattern: its traffic is the probes themselves).  Every answer is compared with
tests/flowtab_model.py before anything is printed.  One JSON line;
frac_of_pattern = c / b, price_of_rx = b / a.  For scale, one host core walks
a chained table over the same records (flowtab_cpu_walk: a restatement of
fhash.c:103-121 written for this tool, not mTCP code).

    make tools/libflowtab_pattern.so
    python tools/flowtab_bench.py [--n 1048576] [--out profiles/flowtab/bench_flowtab.json]
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
    P = ctypes.CDLL(os.path.join(ROOT, "tools", "libflowtab_pattern.so"))
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    P.flowtab_pattern_launch.argtypes = [vp, u32, vp, u32, vp, vp, vp]
    P.flowtab_lookup_group_launch.argtypes = [ctypes.c_int, vp, u32, vp, u32, vp, vp, vp]
    P.flowtab_build.argtypes = [vp, u32, vp, u32, vp, u32, vp, vp]
    P.flowtab_cpu_walk.argtypes = [vp, u32, vp, u32, vp, ctypes.c_int]
    P.flowtab_cpu_walk.restype = ctypes.c_double
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


class Workload:
    """The C3 batch, its rx records and the lookup records made from them."""

    def __init__(self, n):
        import torch
        from mtcp_amd import gpu, pktgen
        self.n, self.dev, seed = n, torch.device("cuda", 0), 42
        self.desc, nbytes = pktgen.layout(n, "bimodal", 6, seed)
        self.d_buf = torch.zeros((nbytes + 15) & ~15, dtype=torch.uint8, device=self.dev)
        self.d_desc = torch.from_numpy(self.desc.view(np.uint8).copy()).to(self.dev)
        gpu.pktgen_dev(self.d_buf, self.d_desc, n, 6, seed)
        self.d_res = torch.zeros(n * 40, dtype=torch.uint8, device=self.dev)
        torch.cuda.synchronize()


def run_lookup(args, P, ctx, wl, n, flows, cap_log2, churn, graph):
    import torch
    from mtcp_amd import RESULT_DTYPE, gpu
    from tests import flowtab_model as fm

    dev, st = wl.dev, torch.cuda.Stream(device=wl.dev)
    h = st.cuda_stream
    rng = np.random.default_rng(flows + churn)
    junk_n = (1 << cap_log2) // 4 if churn else 0
    pool = np.unique(rng.integers(0, 256, (2 * flows + junk_n + (2 * flows + junk_n) // 8, 12), dtype=np.uint8), axis=0)
    pool = pool[rng.permutation(len(pool))[:2 * flows + junk_n]]
    keys, junk = pool[:2 * flows], pool[2 * flows:]
    ids = rng.permutation(flows).astype(np.uint32)
    ent = fm.entries(keys[:flows], ids)
    junk_ent = fm.entries(junk, np.arange(junk_n, dtype=np.uint32) + flows)
    # the rx records of the first n frames, their tuples replaced by pool keys
    ctx.rx_chunk_dev(wl.d_buf, wl.d_desc, n, 6, wl.d_res, stream=st)
    st.synchronize()
    res = wl.d_res[:n * 40].cpu().numpy().view(RESULT_DTYPE).copy()
    which = rng.integers(0, 2 * flows, n)
    e = fm.entries(keys[which], 0)
    res["daddr"], res["saddr"], res["dport"], res["sport"] = e["saddr"], e["daddr"], e["sport"], e["dport"]
    d_look = torch.from_numpy(res.view(np.uint8).copy()).to(dev)
    mk = lambda b: torch.zeros(max(b, 16), dtype=torch.uint8, device=dev)
    d_sid, d_bins, p_sid, p_bins, g_sid, g_bins = (mk(4 * n) for _ in range(6))
    # churn: the junk pairs go in with the real ones and are removed again
    both = np.concatenate([ent, junk_ent])[rng.permutation(flows + junk_n)] if churn else ent
    d_both, d_junk = torch.from_numpy(both.view(np.uint8).copy()).to(dev), torch.from_numpy(
        junk_ent.view(np.uint8).copy()).to(dev) if churn else None
    img, img_stats = mk(16 << cap_log2), mk(16)            # the table image of the group-size legs
    if P.flowtab_build(img.data_ptr(), cap_log2, d_both.data_ptr(), len(both),
                       d_junk.data_ptr() if churn else None, junk_n, img_stats.data_ptr(), h) != 0:
        raise SystemExit("flowtab_build did not launch")
    with gpu.FlowTable(ctx, cap_log2) as tab:
        tab.update_dev(None, 0, d_both, len(both), stream=st)
        if churn:
            tab.update_dev(d_junk, junk_n, None, 0, stream=st)
        st.synchronize()
        stats = tab.stats()
        if stats != {"live": flows, "tombs": junk_n, "insert_failed": 0, "remove_missed": 0}:
            raise SystemExit(f"the table's counters are wrong: {stats}")
        if img_stats.cpu().numpy().view(np.uint32).tolist() != [flows, junk_n, 0, 0]:
            raise SystemExit("the table image's counters are wrong")

        def leg_rx():
            ctx.rx_chunk_dev(wl.d_buf, wl.d_desc, n, 6, wl.d_res, stream=st)

        def leg_lookup():
            tab.lookup_dev(d_look, n, d_sid, d_bins, stream=st)

        def leg_pattern():
            if P.flowtab_pattern_launch(d_look.data_ptr(), n, img.data_ptr(), cap_log2, p_sid.data_ptr(),
                                        p_bins.data_ptr(), h) != 0:
                raise SystemExit("the pattern kernel did not launch")

        def leg_group(G):
            def go():
                if P.flowtab_lookup_group_launch(G, d_look.data_ptr(), n, img.data_ptr(), cap_log2, g_sid.data_ptr(),
                                                 g_bins.data_ptr(), h) != 0:
                    raise SystemExit("the group kernel did not launch")
            return go

        legs = {"rx_us": leg_rx, "lookup_us": leg_lookup, "pattern_us": leg_pattern,
                "group1_us": leg_group(1), "group2_us": leg_group(2), "group4_us": leg_group(4)}
        # correctness first: nothing is printed for answers that are wrong
        model = fm.FlowTable()
        model.update(ins=ent)
        want = model.lookup(res)
        by_construction = np.where(which < flows, ids[np.minimum(which, flows - 1)], MISS).astype(np.uint32)
        by_construction[res["verdict"] != 0] = NONE
        if not np.array_equal(want, by_construction):
            raise SystemExit("the model's answers differ from the construction")
        for G in (1, 2, 4):
            leg_group(G)()
            st.synchronize()
            if not np.array_equal(g_sid.cpu().numpy().view(np.uint32)[:n], want):
                raise SystemExit(f"group {G}: answers differ from the model")
        leg_lookup()
        leg_pattern()
        st.synchronize()
        if not np.array_equal(d_sid.cpu().numpy().view(np.uint32)[:n], want):
            raise SystemExit("the answers differ from the model")
        import oracle
        if not np.array_equal(d_bins.cpu().numpy().view(np.uint32)[:n], oracle.flow_bins(res)):
            raise SystemExit("the bins differ from the oracle")
        med, spread = timed(args, legs, st, graph)
    ok = res["verdict"] == 0
    out = {
        "case": f"{n} records, {flows} flows in cap 2^{cap_log2}{', a quarter of the slots TOMB' if churn else ''}"
                f"{', HIP graph' if graph else ''}",
        "hit_fraction_of_tcp_ok": round(float((want[ok] < MISS).mean()), 3),
        **{k: round(v, 2) for k, v in med.items()},
        "spread_us": spread,
        "frac_of_pattern": round(med["pattern_us"] / med["lookup_us"], 3),
        "price_of_rx": round(med["lookup_us"] / med["rx_us"], 3),
    }
    return out, res, ent


def run_update(args, ctx, wl, cap_log2, flows, batch):
    """`batch` removes plus `batch` inserts per launch on a table of `flows`
    flows: launches alternate between removing A / inserting B and the
    reverse, so the table holds `flows` pairs before every launch."""
    import torch
    from mtcp_amd import gpu
    from tests import flowtab_model as fm

    st = torch.cuda.Stream(device=wl.dev)
    rng = np.random.default_rng(99)
    pool = np.unique(rng.integers(0, 256, (flows + 2 * batch + flows, 12), dtype=np.uint8), axis=0)
    pool = pool[rng.permutation(len(pool))[:flows + batch]]
    base = fm.entries(pool[:flows - batch], np.arange(flows - batch, dtype=np.uint32))
    A = fm.entries(pool[flows - batch:flows], np.arange(batch, dtype=np.uint32) + flows)
    B = fm.entries(pool[flows:], np.arange(batch, dtype=np.uint32) + 2 * flows)
    up = lambda a: torch.from_numpy(a.view(np.uint8).copy()).to(wl.dev)
    d_base, d_A, d_B = up(base), up(A), up(B)
    with gpu.FlowTable(ctx, cap_log2) as tab:
        tab.update_dev(None, 0, d_base, len(base), stream=st)
        tab.update_dev(None, 0, d_A, batch, stream=st)
        flip = [0]

        def leg_update():
            d, i = (d_A, d_B) if flip[0] == 0 else (d_B, d_A)
            flip[0] ^= 1
            tab.update_dev(d, batch, i, batch, stream=st)

        med, spread = timed(args, {"update_us": leg_update}, st, False)
        st.synchronize()
        stats = tab.stats()
        if stats["live"] != flows or stats["insert_failed"] or stats["remove_missed"]:
            raise SystemExit(f"the update case's counters are wrong: {stats}")
        # and the table answers as the model does after an even number of launches
        if flip[0]:
            leg_update()
        model = fm.FlowTable()
        model.update(ins=np.concatenate([base, A]))
        from mtcp_amd import RESULT_DTYPE
        e = fm.entries(pool, 0)
        res = np.zeros(len(pool), dtype=RESULT_DTYPE)
        res["daddr"], res["saddr"], res["dport"], res["sport"] = e["saddr"], e["daddr"], e["sport"], e["dport"]
        if not np.array_equal(tab.lookup(res), model.lookup(res)):
            raise SystemExit("after the updates the answers differ from the model")
    return {"case": f"{batch} removes + {batch} inserts per launch, {flows} flows in cap 2^{cap_log2} (two launches: "
                    f"remove, insert)", "update_us": round(med["update_us"], 2), "spread_us": spread,
            "tombs_at_end": stats["tombs"]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--launches", type=int, default=20, help="launches per timed window")
    ap.add_argument("--warm-seconds", type=float, default=1.0)
    ap.add_argument("--skip-large", action="store_true", help="leave out the 1 M-flow tables")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the MI355X only")
    from mtcp_amd import gpu
    P = pattern_lib()
    wl = Workload(args.n)
    cases = {"flows_64k": (args.n, 65536, 17, False, False), "flows_64k_tombs": (args.n, 65536, 17, True, False),
             "small_4096_graph": (4096, 65536, 17, False, True)}
    if not args.skip_large:
        cases.update({"flows_1m": (args.n, 1 << 20, 21, False, False),
                      "flows_1m_tombs": (args.n, 1 << 20, 21, True, False)})
    line = {
        "tool": "tools/flowtab_bench.py",
        "device": torch.cuda.get_device_name(0),
        "method": f"HIP events around {args.launches} launches, median of {args.rounds} alternating rounds "
                  f"after {args.warm_seconds} s of untimed launches, one process",
        "yardstick": "pattern_us (tools/flowtab_pattern.hip): same record loads and stores on the same grid, one "
                     "16 B gather per TCP_OK record, no hashing, comparing or probing",
    }
    with gpu.Context(0) as ctx:
        for name, c in cases.items():
            line[name], res, ent = run_lookup(args, P, ctx, wl, *c)
            if name == "flows_64k":
                sid = np.zeros(len(res), np.uint32)
                best = P.flowtab_cpu_walk(res.ctypes.data, len(res), ent.ctypes.data, len(ent), sid.ctypes.data, 5)
                from tests import flowtab_model as fm
                m = fm.FlowTable()
                m.update(ins=ent)
                if not np.array_equal(sid, m.lookup(res)):
                    raise SystemExit("the CPU walk's answers differ from the model")
                line["cpu_chained_walk_1core_us"] = round(best * 1e6, 1)
                line["cpu_note"] = (f"one host core, a chained table of 131072 bins over the {len(res)} records of "
                                    "flows_64k, best of 5 (a restatement of fhash.c:103-121 for this tool)")
        line["update_64k"] = run_update(args, ctx, wl, 18, 131072, 65536)
    text = json.dumps(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
