#!/usr/bin/env python3
"""Measures the batched application write (SURVEY §8 f18,
mtcp_amd/csrc/sndwrite_kernels.hpp) on the MI355X against its yardsticks.

Workload: every stream has a send buffer that holds some unacknowledged bytes
at a random head_off and a random 16 B phase of the arena, and one request
writes a run from a source range at a random phase behind them.  The run
lengths are those the other rows' benches use (C3's bimodal batch: frames of
64 B and 1500 B, 16 segments a stream).  In one process, HIP events around
`launches` launches, median of `rounds` alternating rounds after a second of
untimed launches, per leg:

  (a) write_us    a device copy that puts the records back, then
                  mtcp_gpu_sndwrite_dev (clear, claim, plan, scan, move, copy);
  (b) pattern_us  the same record copy, then tools/sndwrite_pattern.hip: the
                  copy units' loads and stores on the copy kernel's grid, no
                  plan, no search, no shift, no move;
  (c) reset_us    the record copy alone;
  (d) memcpy_us   what INTEGRATION §6 prescribes without this row: one
                  hipMemcpyAsync per stream out of pinned host memory and one
                  wait each, host wall time over the first `--memcpy-streams`
                  writes, scaled to the leg's streams.

Legs: 65 536 streams of C3's runs; 1 M streams of one MSS each; 4 096 requests
as one captured launch set; 65 536 streams of which half compact; 4 096 streams
of which one in 64 takes 1 MiB; the 65 536-stream leg with the source in
registered host memory; 16 384 streams through mtcp_gpu_write_send_dev (rows
f15, f8 and f7) to frames.  Every output of every leg is compared with the
expectation (all requests WRITTEN in full, every chunk byte) and a sample of
2 048 requests with tests/sndwrite_model.py before anything is printed.  One
JSON line.

    make tools/libsndwrite_pattern.so
    python tools/sndwrite_bench.py [--out profiles/sndwrite/bench_sndwrite.json]
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

MSS = 1448


def pattern_lib():
    P = ctypes.CDLL(os.path.join(ROOT, "tools", "libsndwrite_pattern.so"))
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    P.sndwrite_pattern_dev.argtypes = [vp, u32, vp, u64, vp, u64, u32, vp]
    P.sndwrite_pattern_dev.restype = ctypes.c_int
    return P


def bimodal(rng, k):
    """Payload bytes of k frames of C3's batch: 64 B and 1500 B frames, 54 B of headers."""
    return np.where(rng.random(k) < 0.5, 10, 1446)


def lay_out(rng, lens, compact):
    """n streams for one write of lens[i] bytes each.  compact[i]: the write
    passes the chunk's end, so SBPut moves the held bytes down first."""
    from mtcp_amd._types import ACK_STATE_DTYPE, DATAGEN_STATE_DTYPE
    n = len(lens)
    held = rng.integers(1, 600, n)
    head = np.minimum(rng.integers(16, 300, n), lens)  # a compacting chunk ends 8 bytes behind the run: head_off fits
    # not compacting: tail_off + len stays below size (tcp_send_buffer.c:130); compacting: it passes size by head - 8
    size = np.where(compact, held + lens + 8, (head + held + lens) // 256 * 256 + 256)
    span = size
    phase = rng.integers(0, 16, n)
    off = np.cumsum(span + 80 + 16) - span - 16
    off = (off // 16) * 16 + 64 + phase
    arena_bytes = int((off[-1] + size[-1] + 64 + 15) // 16 * 16)
    snd, dtx = np.zeros(n, ACK_STATE_DTYPE), np.zeros(n, DATAGEN_STATE_DTYPE)
    seq = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    snd["sb_head_seq"], snd["snd_una"], snd["snd_nxt"] = seq, seq, seq
    snd["sb_len"], snd["sb_size"], snd["snd_wnd"] = held, size, size - held
    snd["mss"], snd["eff_mss"], snd["tcp_state"], snd["has_sndbuf"] = 1460, MSS, 4, 1
    snd["cwnd"], snd["peer_wnd"], snd["rto"] = 1 << 20, 1 << 20, 200
    dtx["sb_off"], dtx["sb_base_seq"] = off, seq - head.astype(np.uint32)
    return snd, dtx, off, head, held, size, arena_bytes


def run(args, P, ctx, name, lens, graph=False, host_src=False, compact_half=False, send=False):
    import torch
    from group_bench import timed
    from mtcp_amd import gpu
    from mtcp_amd._lib import lib
    from mtcp_amd._types import SNDWRITE_REQ_DTYPE, SNDWRITE_RES_DTYPE
    from tests import sndwrite_model as sm

    L, dev = lib(), torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    rng = np.random.default_rng(len(lens) + compact_half)
    n = len(lens)
    compact = (np.arange(n) % 2 == 0) if compact_half else np.zeros(n, bool)
    snd, dtx, off, head, held, size, arena_bytes = lay_out(rng, lens, compact)
    to_put = np.minimum(lens, size - held)
    assert (to_put == lens).all()
    moved = compact & (head + held + lens >= size)
    assert (moved == compact).all()
    arena = rng.integers(0, 256, arena_bytes, dtype=np.uint8)
    # the requests in a random order of the streams; the source ranges at random phases, 16-79 bytes apart
    sid = rng.permutation(n).astype(np.int64)
    ln = lens[sid]
    soff = np.cumsum(rng.integers(16, 80, n) + ln) - ln
    src_bytes = int((soff[-1] + ln[-1] + 64 + 15) // 16 * 16)
    src = rng.integers(0, 256, src_bytes, dtype=np.uint8)
    req = np.zeros(n, SNDWRITE_REQ_DTYPE)
    req["sid"], req["len"], req["src_off"] = sid, ln, soff
    d_req, d_snd0, d_dtx0 = up(req), up(snd), up(dtx)
    d_snd, d_dtx, d_arena, d_parena = up(snd), up(dtx), up(arena), up(arena)
    zeros = lambda k: torch.zeros(k, dtype=torch.uint8, device=dev)
    d_wres, d_total = zeros(16 * n), zeros(16)
    d_sid, d_start, d_stop, d_nseg = zeros(4 * n), zeros(4 * n + 4), zeros(4 * n), zeros(4)
    wb = gpu.Context.sndwrite_work_bytes(n, n - 1)
    d_work = zeros(wb)
    if host_src:
        h_src = np.zeros(src_bytes + 64, np.uint8)
        h_src = h_src[(-h_src.ctypes.data) % 64:][:src_bytes]
        h_src[:] = src
        gpu.host_register(h_src)
        src_ptr = h_src.ctypes.data
    else:
        d_src = up(src)
        src_ptr = d_src.data_ptr()

    def reset():
        with torch.cuda.stream(st):
            d_snd.copy_(d_snd0, non_blocking=True)
            d_dtx.copy_(d_dtx0, non_blocking=True)

    def leg_write():
        reset()
        rc_ = L.mtcp_gpu_sndwrite_dev(ctx._h, d_req.data_ptr(), n, n - 1, d_snd.data_ptr(), d_dtx.data_ptr(), src_ptr,
                                      src_bytes, d_arena.data_ptr(), arena_bytes, d_wres.data_ptr(), d_sid.data_ptr(),
                                      d_start.data_ptr(), d_stop.data_ptr(), d_nseg.data_ptr(), d_total.data_ptr(),
                                      d_work.data_ptr(), wb, st.cuda_stream)
        if rc_ != 0:
            raise SystemExit(f"{name}: mtcp_gpu_sndwrite_dev returned {rc_}")

    leg_write()
    st.synchronize()
    # correctness first: nothing is printed for outputs that are wrong
    wres = d_wres.cpu().numpy().view(SNDWRITE_RES_DTYPE)
    got = d_arena.cpu().numpy()
    dst = np.where(compact, off + held, off + head + held)       # where the run went
    win = np.where(compact, off, off + head)                     # where the held bytes are now
    old = off + head
    ok = True
    for i, (d, w, o, h, s, k) in enumerate(zip(dst[sid].tolist(), win[sid].tolist(), old[sid].tolist(), held[sid].tolist(),
                                               soff.tolist(), ln.tolist())):
        ok = ok and got[d:d + k].tobytes() == src[s:s + k].tobytes() and got[w:w + h].tobytes() == arena[o:o + h].tobytes()
    guard = np.ones(arena_bytes, bool)
    for o, s in zip(off.tolist(), size.tolist()):
        guard[o:o + s] = False
    ok = ok and (got[guard] == arena[guard]).all()
    g_snd, g_dtx = d_snd.cpu().numpy().view(snd.dtype), d_dtx.cpu().numpy().view(dtx.dtype)
    want_flags = np.where(size - held - lens > 0, 1, 0) | 2 | np.where(compact, 4, 0)
    ok = ok and (wres["verdict"] == sm.WRITTEN).all() and (wres["written"] == ln).all() and (wres["sid"] == sid).all() and \
        (wres["snd_wnd"] == (size - held - lens)[sid]).all() and (wres["flags"] == want_flags[sid]).all() and \
        (g_snd["sb_len"] == held + lens).all() and (g_snd["snd_wnd"] == size - held - lens).all() and \
        (g_dtx["on_send_list"] == 1).all() and \
        (g_dtx["sb_base_seq"] == np.where(compact, snd["sb_head_seq"], dtx["sb_base_seq"])).all() and \
        d_total.cpu().numpy().view(np.uint64).tolist() == [n, int(lens.sum())] and \
        (d_sid.cpu().numpy().view(np.uint32) == sid).all() and not d_start.cpu().numpy().any() and \
        not d_stop.cpu().numpy().any() and int(d_nseg.cpu().numpy().view(np.uint32)[0]) == n
    # a sample through the model, on the host's copy of the arena (its chunks alone are compared)
    pick = np.sort(rng.choice(n, min(n, 2048), replace=False))
    m_snd, m_dtx, m_arena = snd.copy(), dtx.copy(), arena
    w_wres = sm.write(req[pick], n - 1, m_snd, m_dtx, src, m_arena)[0]
    s_ids = sid[pick]
    ok = ok and wres[pick].tobytes() == w_wres.tobytes() and g_snd[s_ids].tobytes() == m_snd[s_ids].tobytes() and \
        g_dtx[s_ids].tobytes() == m_dtx[s_ids].tobytes()
    for s in s_ids[:512].tolist():
        ok = ok and got[off[s]:off[s] + size[s]].tobytes() == m_arena[off[s]:off[s] + size[s]].tobytes()
    if not ok:
        raise SystemExit(f"{name}: the write's outputs differ from the model")
    # the pattern's units: as the copy cuts the runs
    dq = dst[sid]
    first = dq >> 4
    pieces = ((dq + ln + 15) >> 4) - first
    upr = (pieces + 255) // 256
    r_of = np.repeat(np.arange(n), upr)
    k_of = np.arange(int(upr.sum())) - np.repeat(np.cumsum(upr) - upr, upr)
    units = np.zeros((len(r_of), 4), np.uint32)
    units[:, 0], units[:, 1] = (soff[r_of] >> 4) + 256 * k_of, first[r_of] + 256 * k_of
    units[:, 2] = np.minimum(pieces[r_of] - 256 * k_of, 256)
    d_units = up(units)
    cu8 = torch.cuda.get_device_properties(0).multi_processor_count * 8

    def leg_pattern():
        reset()
        if P.sndwrite_pattern_dev(d_units.data_ptr(), len(units), src_ptr, src_bytes, d_parena.data_ptr(), arena_bytes,
                                  cu8, st.cuda_stream) != 0:
            raise SystemExit("the pattern kernel did not launch")

    leg_pattern()
    st.synchronize()
    legs = {"write_us": leg_write, "pattern_us": leg_pattern, "reset_us": reset}
    out = {}
    if send:
        from mtcp_amd._types import DATAGEN_RES_DTYPE
        from tests import rtosweep_model as rs
        from tests import txbuild_model as xm
        from tests.test_gpu_datagen import LINKS
        state, tx, _ = rs.send_side(n, 3)
        seg_cap = int(((held + lens + MSS - 1) // MSS).sum()) + 64
        d_state, d_tx0, d_tx, d_links = up(state), up(tx), up(tx), up(LINKS)
        d_idx, d_seg, d_desc = zeros(4 * n), zeros(48 * seg_cap), zeros(8 * seg_cap)
        d_dres, d_dtotal, d_status, d_image = zeros(16 * n), zeros(16), zeros(seg_cap), zeros(seg_cap * rs.SLOT)
        dwb = gpu.Context.datagen_work_bytes(n, n - 1)
        d_dwork = zeros(dwb)

        def reset_send():
            reset()
            with torch.cuda.stream(st):
                d_tx.copy_(d_tx0, non_blocking=True)

        def leg_send():
            reset_send()
            rc_ = L.mtcp_gpu_write_send_dev(
                ctx._h, d_req.data_ptr(), n, n - 1, d_snd.data_ptr(), d_dtx.data_ptr(), src_ptr, src_bytes,
                d_arena.data_ptr(), arena_bytes, d_wres.data_ptr(), d_sid.data_ptr(), d_start.data_ptr(),
                d_stop.data_ptr(), d_nseg.data_ptr(), d_total.data_ptr(), d_work.data_ptr(), wb, d_idx.data_ptr(),
                d_state.data_ptr(), d_tx.data_ptr(), 1000, d_links.data_ptr(), rs.N_LINKS, d_image.data_ptr(), 0,
                seg_cap * rs.SLOT, 0, rs.SLOT, 0, 0, d_seg.data_ptr(), d_desc.data_ptr(), seg_cap, d_dres.data_ptr(),
                d_dtotal.data_ptr(), d_status.data_ptr(), d_dwork.data_ptr(), dwb, st.cuda_stream)
            if rc_ != 0:
                raise SystemExit(f"{name}: mtcp_gpu_write_send_dev returned {rc_}")

        leg_send()
        st.synchronize()
        dres = d_dres.cpu().numpy().view(DATAGEN_RES_DTYPE)
        frames = int(d_dtotal.cpu().numpy().view(np.uint64)[0])
        if not ((dres["status"] == 9).all() and (dres["bytes"] == (held + lens)[sid]).all() and
                frames == int(((held + lens + MSS - 1) // MSS).sum()) and (d_status.cpu().numpy()[:frames] == xm.BUILT).all()):
            raise SystemExit(f"{name}: write_send's frames differ from the expectation")
        legs.update({"write_send_us": leg_send, "reset_send_us": reset_send})
        out["frames"] = frames
    med, spread = timed(args, legs, st, graph)
    # INTEGRATION §6 without this row: a copy and a wait per stream
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
    m = min(n, args.memcpy_streams)
    pinned = torch.empty(int(soff[m - 1] + ln[m - 1]) + 64, dtype=torch.uint8, pin_memory=True)
    pinned.numpy()[:] = src[:len(pinned)]
    base, abase, sh = pinned.data_ptr(), d_parena.data_ptr(), st.cuda_stream
    srcs, dsts, lns = soff[:m].tolist(), dq[:m].tolist(), ln[:m].tolist()
    walls = []
    for _ in range(3):
        t0 = time.perf_counter()
        for s, d, k in zip(srcs, dsts, lns):
            hip.hipMemcpyAsync(abase + d, base + s, k, 1, sh)
            hip.hipStreamSynchronize(sh)
        walls.append((time.perf_counter() - t0) * 1e6 * n / m)
    if d_parena[dsts[0]:dsts[0] + lns[0]].cpu().numpy().tobytes() != src[srcs[0]:srcs[0] + lns[0]].tobytes():
        raise SystemExit(f"{name}: the per-stream copy brought other bytes")
    if host_src:
        st.synchronize()
        gpu.host_unregister(h_src)
    print(f"measured: {name}", file=sys.stderr, flush=True)
    write, pat = med["write_us"] - med["reset_us"], med["pattern_us"] - med["reset_us"]
    nbytes = int(lens.sum())
    out.update({
        "case": f"{n} streams, {nbytes} bytes, {len(units)} units, {int(compact.sum())} compacting"
                f"{', HIP graph' if graph else ''}{', source in registered host memory' if host_src else ''}",
        "launches_per_window": args.launches, "rounds": args.rounds,
        **{k: round(v, 2) for k, v in med.items()}, "spread_us": spread,
        "write_less_reset_us": round(write, 2), "pattern_less_reset_us": round(pat, 2),
        "frac_of_pattern": round(pat / write, 3),
        "tb_per_s_read_plus_write": round(2 * nbytes / write / 1e6, 3),
        "memcpy_per_stream_us": round(min(walls), 1), "memcpy_spread_us": [round(min(walls), 1), round(max(walls), 1)],
        "memcpy_streams_timed": m, "memcpy_over_write": round(min(walls) / write, 1),
    })
    if send:
        out["write_send_less_reset_us"] = round(med["write_send_us"] - med["reset_send_us"], 2)
    return out


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
        "tool": "tools/sndwrite_bench.py",
        "device": torch.cuda.get_device_name(0),
        "method": f"HIP events around {args.launches} launches, median of {args.rounds} alternating rounds after "
                  f"{args.warm_seconds} s of untimed launches, one process; every timed write and pattern launch is "
                  "preceded by device copies that put the records back (reset_us, subtracted in the ratios); no counter "
                  "or trace run stands behind any figure",
        "yardsticks": "pattern_us (tools/sndwrite_pattern.hip): the copy units' loads and stores on the copy kernel's "
                      "grid, no plan, no search, no shift, no move; memcpy_per_stream_us: one hipMemcpyAsync out of "
                      "pinned host memory and one wait per stream, host wall time over memcpy_streams_timed writes "
                      "scaled to the leg, best of 3 with the spread",
    }
    want = None if args.cases == "all" else set(args.cases.split(","))
    rng = np.random.default_rng(5)
    c3 = bimodal(rng, 65536 * 16).reshape(65536, 16).sum(axis=1)
    heavy = bimodal(rng, 4096)
    heavy[::64] = 1 << 20
    legs = (("c3_64k_streams", c3, {}), ("one_mss_1m_streams", np.full(1 << 20, MSS), {}),
            ("small_4096_graph", bimodal(rng, 4096 * 16).reshape(4096, 16).sum(axis=1), {"graph": True}),
            ("c3_64k_streams_half_compacting", c3, {"compact_half": True}),
            ("one_in_64_takes_1mib", heavy, {}), ("c3_64k_streams_host_src", c3, {"host_src": True}),
            ("write_send_16k_streams", np.full(16384, MSS), {"send": True}))
    with gpu.Context(0) as ctx:
        for name, lens, kw in legs:
            if want is None or name in want:
                line[name] = run(args, P, ctx, name, lens.astype(np.int64), **kw)
                if args.out:                          # after every leg: a run that ends early leaves what it measured
                    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                    with open(args.out, "w") as f:
                        f.write(json.dumps(line) + "\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
