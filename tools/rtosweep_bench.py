"""The retransmission-timeout sweep (include/mtcp_gpu_rtosweep.h, DESIGN §8 row
f16) timed on the device: one process, HIP events around windows of launches on
one stream, the median window per launch.

The streams are made at the call's input level: ESTABLISHED senders with two
full segments buffered (mss 1460) and their timers armed; the due ones have a
ts_rto at or just behind cur_ts.  Legs, at every size of --sizes (the
three-launch form) and at 4 096 streams (the one-workgroup form):

    none     no stream is due, every stream is on the RTO list: the pass every
             tick pays while every sender has data in flight
    idle     no stream is on the RTO list (on_rto 0)
    1in64    every 64th stream is due, cap = their number
    all      every stream is due, cap = streams

per leg:
    reset_us     the copies that put d_snd and d_dtx back (in every other
                 figure; subtracted in the *_net figures)
    sweep_us     mtcp_gpu_rto_sweep_dev
    cond_us      the sweep's three launches with tools/rtosweep_pattern.hip's
                 count kernel, whose due test loads ts_rto only where on_rto
                 is 1, behind that load (three-launch form only)
    pattern_us   tools/rtosweep_pattern.hip's two kernels around the sweep's
                 scan: the same loads and stores on the same grids without the
                 step arithmetic and the ranking (three-launch form only)
and for 1in64:
    datagen_us   mtcp_gpu_datagen_dev (row f15) alone over the table the sweep
                 wrote: a batch with the same number of streams
    send_us      mtcp_gpu_rto_send_dev: the sweep, row f15 and the frame builder

Correctness first: before anything is timed the sweep's bytes (d_snd, d_dtx,
d_rto, d_seg_sid, d_seg_start, d_seg_stop, d_nseg, d_total) are compared with
tests/rtosweep_model.py in full, for the library's call and for the variant.

    python tools/rtosweep_bench.py [--sizes 65536,1048576] [--out profiles/rtosweep/bench_rtosweep.json]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mtcp_amd._types import (ACK_STATE_DTYPE, ACKGEN_STATE_DTYPE, DATAGEN_STATE_DTYPE, RCV_STATE_DTYPE,  # noqa: E402
                             RTO_REC_DTYPE, TX_LINK_DTYPE)
from tests import rtosweep_model as rm  # noqa: E402

CUR_TS = 0x12345678
MSS, SEG, SLOT = 1460, 1448, 1536


def make(n, kind, seed=7):
    rng = np.random.default_rng(seed)
    snd = np.zeros(n, dtype=ACK_STATE_DTYPE)
    snd["sb_head_seq"] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    snd["snd_una"] = snd["sb_head_seq"]
    snd["snd_nxt"] = snd["snd_una"] + 2 * SEG
    snd["sb_len"], snd["sb_size"] = 2 * SEG, 1 << 16
    snd["cwnd"], snd["peer_wnd"] = 4 * SEG + rng.integers(0, 9000, n), 4 * SEG + rng.integers(0, 9000, n)
    snd["mss"], snd["eff_mss"], snd["tcp_state"], snd["has_sndbuf"], snd["on_rto"] = MSS, SEG, 4, 1, 1
    snd["rto"], snd["srtt"], snd["rttvar"] = rng.integers(1, 3000, n), rng.integers(0, 1 << 12, n), rng.integers(1, 200, n)
    snd["nrtx"] = rng.integers(0, 6, n)
    snd["ts_rto"] = CUR_TS + 1 + rng.integers(0, 3000, n)
    due = np.arange(n) if kind == "all" else np.arange(0, n, 64) if kind == "1in64" else np.zeros(0, np.int64)
    snd["ts_rto"][due] = CUR_TS - rng.integers(0, 3, len(due))
    if kind == "idle":
        snd["on_rto"] = 0
    dtx = np.zeros(n, dtype=DATAGEN_STATE_DTYPE)
    dtx["sb_off"] = 1 + (np.arange(n, dtype=np.uint64) >> 6) * (2 * SEG + 2)      # the due streams' buffers, apart
    dtx["sb_base_seq"] = snd["sb_head_seq"]
    return snd, dtx, len(due)


def pattern_lib():
    P = ctypes.CDLL(os.path.join(ROOT, "tools", "librtosweep_pattern.so"))
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    P.rtosweep_cond.argtypes = [u32, vp, vp, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp]
    P.rtosweep_pattern.argtypes = [u32, vp, vp, u32, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    P.rtosweep_cond.restype = P.rtosweep_pattern.restype = ctypes.c_int
    return P


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="65536,1048576")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--launches", type=int, default=20, help="launches per timed window")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch

    from mtcp_amd import gpu
    P = pattern_lib()
    dev = torch.device("cuda", 0)
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    zeros = lambda k: torch.zeros(k, dtype=torch.uint8, device=dev)
    raw = lambda t_: ctypes.c_void_p(t_.data_ptr())
    sizes = [int(s) for s in args.sizes.split(",")]
    line = {"sizes": sizes, "launches": args.launches, "rounds": args.rounds, "mss": MSS, "slot_bytes": SLOT}
    st = torch.cuda.Stream(device=dev)
    h = ctypes.c_void_p(st.cuda_stream)
    links = np.zeros(3, dtype=TX_LINK_DTYPE)
    links["dst"][:, 0], links["src"][:, 0] = 2, 2

    def timed(leg):
        times = []
        for _ in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(args.launches):
                leg()
            e1.record(st)
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3 / args.launches)
        times.sort()
        return round(times[len(times) // 2], 2), round((times[-1] - times[0]) / times[len(times) // 2], 3)

    class Leg:
        def __init__(self, ctx, n, kind):
            self.ctx, self.n, self.kind = ctx, n, kind
            self.snd, self.dtx, self.due = make(n, kind)
            self.cap = cap = max(self.due, 1)
            self.d_snd, self.d_dtx, self.snd0, self.dtx0 = (to_dev(a) for a in (self.snd, self.dtx, self.snd, self.dtx))
            self.outs = (zeros(16 * cap), zeros(4 * cap), zeros(4 * cap + 4), zeros(4 * cap), zeros(4), zeros(16))
            wb = gpu.Context.rto_sweep_work_bytes(n - 1, cap)
            self.work, self.scratch = zeros(wb), zeros(wb)
            self.many = n > gpu.Context.rto_sweep_tile() or cap > gpu.Context.rto_sweep_tile()

        def reset(self):
            with torch.cuda.stream(st):
                self.d_snd.copy_(self.snd0, non_blocking=True)
                self.d_dtx.copy_(self.dtx0, non_blocking=True)

        def sweep(self):
            self.reset()
            self.ctx.rto_sweep_dev(self.n - 1, self.d_snd, self.d_dtx, CUR_TS, self.cap, *self.outs, self.work, stream=st)

        def cond(self):
            self.reset()
            if P.rtosweep_cond(self.n - 1, raw(self.d_snd), raw(self.d_dtx), CUR_TS, self.cap,
                                  *(raw(o) for o in self.outs), raw(self.work), h) != 0:
                raise SystemExit("the variant did not launch")

        def pattern(self):
            self.reset()
            if P.rtosweep_pattern(self.n - 1, raw(self.d_snd), raw(self.d_dtx), CUR_TS, self.cap,
                                  0 if self.kind == "all" else 6, *(raw(o) for o in self.outs), raw(self.work),
                                  raw(self.scratch), h) != 0:
                raise SystemExit("the pattern kernels did not launch")

        def check(self):
            want = rm.sweep(self.snd, self.dtx, CUR_TS, self.cap)
            for what, fn in (("sweep", self.sweep), ("cond", self.cond)):
                for o in self.outs:
                    o.fill_(0xA5)
                torch.cuda.synchronize()
                fn()
                st.synchronize()
                m = want[6]
                got = (self.d_snd, self.d_dtx, self.outs[0][:16 * m], self.outs[1][:4 * m], self.outs[2], self.outs[3])
                for g, e, name in zip(got, want, ("snd", "dtx", "rto", "seg_sid", "seg_start", "seg_stop")):
                    if g.cpu().numpy().tobytes() != e.tobytes():
                        raise SystemExit(f"{what}, {self.n} streams, {self.kind}: {name} differs from the model")
                if int(self.outs[4].cpu().numpy().view(np.uint32)[0]) != m or \
                        self.outs[5].cpu().numpy().view(np.uint64).tolist() != want[7].tolist():
                    raise SystemExit(f"{what}, {self.n} streams, {self.kind}: nseg or total differs from the model")
            if want[6] != self.due:
                raise SystemExit("the leg's due streams are not what the model finds")
            self.sweep()                                       # the pattern reads the sweep's masks from the workspace
            st.synchronize()

    class SendLeg(Leg):
        """The 1in64 leg with the send side behind it."""

        def __init__(self, ctx, n):
            super().__init__(ctx, n, "1in64")
            rng = np.random.default_rng(3)
            state, tx = np.zeros(n, dtype=RCV_STATE_DTYPE), np.zeros(n, dtype=ACKGEN_STATE_DTYPE)
            state["rcv_wnd"], state["tcp_state"], tx["has_rcvbuf"], tx["wscale_mine"] = 1 << 20, 4, 1, 7
            tx["link"] = rng.integers(0, 3, n)
            self.state, self.tx, self.tx0, self.links = to_dev(state), to_dev(tx), to_dev(tx), to_dev(links)
            cap = self.cap
            self.seg_cap = 2 * cap + 8
            self.pbytes = int(cap * (2 * SEG + 2) + 64)
            self.payload, self.idx = zeros(self.pbytes), zeros(4 * cap)
            self.seg, self.desc, self.dres = zeros(48 * self.seg_cap), zeros(8 * self.seg_cap), zeros(16 * cap)
            self.dtotal, self.status, self.image = zeros(16), zeros(self.seg_cap), zeros(SLOT * self.seg_cap)
            self.dwork = zeros(gpu.Context.datagen_work_bytes(cap, n - 1))

        def reset(self):
            super().reset()
            with torch.cuda.stream(st):
                self.tx.copy_(self.tx0, non_blocking=True)

        def send(self):
            self.reset()
            self.ctx.rto_send_dev(self.n - 1, self.d_snd, self.d_dtx, CUR_TS, self.cap, *self.outs, self.work, self.idx,
                                  self.state, self.tx, self.payload, self.links, self.image, 0, 6, SLOT, self.seg,
                                  self.desc, self.seg_cap, self.dres, self.dtotal, self.status, self.dwork, stream=st)

        def keep_swept(self):
            """After a sweep: its states, for row f15 alone."""
            self.snd1, self.dtx1 = self.d_snd.clone(), self.d_dtx.clone()

        def datagen(self):
            """Row f15 alone over the table and the states the sweep left (put back by copies of reset's size)."""
            with torch.cuda.stream(st):
                self.d_snd.copy_(self.snd1, non_blocking=True)
                self.d_dtx.copy_(self.dtx1, non_blocking=True)
                self.tx.copy_(self.tx0, non_blocking=True)
            o = self.outs
            self.ctx.datagen_dev(None, None, self.cap, self.n - 1, self.idx, o[1], o[2], o[4], o[3], self.state,
                                 self.d_snd, self.tx, self.d_dtx, CUR_TS, self.pbytes, 3, 0, SLOT * self.seg_cap, 6, SLOT,
                                 self.seg, self.desc, self.seg_cap, self.dres, self.dtotal, self.dwork, stream=st)

        def check_send(self):
            self.send()
            st.synchronize()
            total = self.dtotal.cpu().numpy().view(np.uint64)
            if int(total[0]) != self.due:                      # one full segment a stream: cwnd = mss
                raise SystemExit(f"rto_send_dev emitted {int(total[0])} records for {self.due} streams")

    with gpu.Context(0) as ctx:
        for n in sizes + [4096]:
            for kind in ("none", "idle", "1in64", "all"):
                leg = SendLeg(ctx, n) if kind == "1in64" else Leg(ctx, n, kind)
                leg.check()
                name = f"n{n}_{kind}_"
                line[name + "due"], line[name + "form"] = leg.due, "three launches" if leg.many else "one workgroup"
                legs = {"reset_us": leg.reset, "sweep_us": leg.sweep}
                if leg.many:
                    legs["cond_us"], legs["pattern_us"] = leg.cond, leg.pattern
                if kind == "1in64":
                    leg.check_send()
                    leg.sweep()
                    st.synchronize()
                    leg.keep_swept()
                    legs["datagen_us"], legs["send_us"] = leg.datagen, leg.send
                for key, fn in legs.items():
                    line[name + key], line[name + key + "_spread"] = timed(fn)
                r = line[name + "reset_us"]
                for key in legs:
                    if key != "reset_us":
                        line[name + key + "_net"] = round(line[name + key] - r, 2)
                del leg
                torch.cuda.empty_cache()
    print(json.dumps(line))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
