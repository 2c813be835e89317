"""The retransmission-timeout sweep on the GPU (include/mtcp_gpu_rtosweep.h,
mtcp_amd/csrc/rtosweep_kernels.hpp): every byte of d_snd, d_dtx,
d_rto[:handled], d_seg_sid[:handled], d_seg_start, d_seg_stop, d_nseg and
d_total of every case is compared with tests/rtosweep_model.py; none is sampled.

Guard regions sit behind every output, the workspace is exactly sized and
pre-filled, d_rto and d_seg_sid past handled keep their sentinel, bytes 88-127
of every send state and every stream that is not handled keep every byte.
Stream counts around the wave, the workgroup and the one-workgroup tile with due
streams at every edge, each through the one-workgroup launch and (cap above the
tile, as tests/test_gpu_txseg.py forces its many-launch form with seg_cap) the
three-launch form; the cap at 1, due - 1, due and due + 1 with a second sweep
for the rest; the reference's fixture as mirrors; records of random bytes; two
workspace fills; the host-memory form; the error returns; and
mtcp_gpu_rto_send_dev down to frames that parse as TCP_OK."""
import numpy as np
import pytest

from mtcp_amd._types import (ACK_STATE_DTYPE, ACKGEN_STATE_DTYPE, DATAGEN_RES_DTYPE, DATAGEN_STATE_DTYPE, DESC_DTYPE,
                             RESULT_DTYPE, RTO_REC_DTYPE, TX_SEG_DTYPE)
from tests import datagen_model as dm
from tests import rtosweep_model as rm
from tests import txbuild_model as xm
from tests.test_gpu_datagen import DEV, LINKS, SENT, Guarded, to_dev

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

EINVAL = -22
ONE, MANY = "rto_one_kernel", "rto_emit_kernel"
TILE = 4096                                  # rtosweep_kernels.hpp kRtoTile
MAX_CAP, MAX_ID = 1 << 24, 0xFFFFFFEF        # MTCP_GPU_TXSEG_MAX_BURSTS, MTCP_GPU_FLOWTAB_MAX_ID
CASES = rm.load_fixture()


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")
    from mtcp_amd import gpu as g
    assert g.Context.rto_sweep_tile() == TILE
    return g


@pytest.fixture(scope="module")
def ctx(gpu):
    with gpu.Context(0) as c:
        yield c


def streams(n, seed, cur_ts):
    """n ESTABLISHED streams, none due: on the RTO list with ts_rto ahead of
    cur_ts, off it with ts_rto behind, or with on_rto 2 (not 1) and ts_rto
    behind."""
    rng = np.random.default_rng(seed)
    snd, dtx = np.zeros(n, dtype=ACK_STATE_DTYPE), np.zeros(n, dtype=DATAGEN_STATE_DTYPE)
    for f in ("snd_nxt", "snd_una", "snd_wnd", "snd_wl1", "snd_wl2", "last_ack_seq", "ssthresh", "mdev", "mdev_max",
              "rtt_seq", "sb_head_seq"):
        snd[f] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    snd["peer_wnd"], snd["cwnd"] = rng.integers(0, 1 << 20, n), rng.integers(0, 1 << 20, n)
    snd["rto"], snd["srtt"], snd["rttvar"] = rng.integers(1, 3000, n), rng.integers(0, 1 << 16, n), rng.integers(0, 4096, n)
    mss = rng.choice([13, 536, 1460, 9000], n)
    snd["mss"], snd["eff_mss"], snd["sb_len"], snd["sb_size"] = mss, mss - 12, rng.integers(0, 8192, n), 8192
    snd["tcp_state"], snd["saw_timestamp"], snd["wscale_peer"] = 4, 1, rng.integers(0, 15, n)
    snd["dup_acks"], snd["nrtx"], snd["has_sndbuf"] = rng.integers(0, 256, n), rng.integers(0, 18, n), rng.random(n) < 0.9
    snd["user"] = rng.integers(0, 256, (n, 40))
    kind = rng.integers(0, 3, n)
    snd["on_rto"] = np.choose(kind, [1, 0, 2])
    ahead = rng.integers(1, 3000, n)
    snd["ts_rto"] = (cur_ts + np.where(kind == 0, ahead, -ahead)) & rm.M32
    dtx["sb_off"], dtx["sb_base_seq"] = rng.integers(0, 1 << 40, n), snd["sb_head_seq"]
    dtx["on_send_list"], dtx["on_control_list"] = rng.integers(0, 2, n), rng.random(n) < 0.05
    return snd, dtx


def make_due(snd, ids, cur_ts, rng):
    ids = np.asarray(ids, dtype=np.int64)
    snd["on_rto"][ids] = 1
    snd["ts_rto"][ids] = (cur_ts - rng.integers(0, 4, len(ids)) * rng.integers(0, 1 << 20, len(ids))) & rm.M32


class Call:
    """The device arrays of one sweep, the outputs guarded."""

    def __init__(self, gpu, snd, dtx, cap, work_fill=SENT):
        self.n, self.cap = len(snd), cap
        self.snd, self.dtx = Guarded(128 * self.n, snd), Guarded(16 * self.n, dtx)
        self.rto, self.seg_sid = Guarded(16 * cap), Guarded(4 * cap)
        self.seg_start, self.seg_stop = Guarded(4 * cap + 4), Guarded(4 * cap)
        self.nseg, self.total = Guarded(4), Guarded(16)
        self.wb = gpu.Context.rto_sweep_work_bytes(self.n - 1, cap)
        assert self.wb > 0
        self.work = Guarded(self.wb, work_fill)

    def outs(self):
        return (self.rto.t, self.seg_sid.t, self.seg_start.t, self.seg_stop.t, self.nseg.t, self.total.t)

    def run(self, ctx, cur_ts, stream=None):
        ctx.rto_sweep_dev(self.n - 1, self.snd.t, self.dtx.t, cur_ts, self.cap, *self.outs(), self.work.t, stream=stream)

    def check(self, want, what=""):
        torch.cuda.synchronize()
        for name in ("snd", "dtx", "rto", "seg_sid", "seg_start", "seg_stop", "nseg", "total", "work"):
            assert getattr(self, name).guard_intact(), f"{what}: bytes behind {name} were written"
        snd, dtx, rec, seg_sid, seg_start, seg_stop, nseg, total = want
        got = (self.snd.numpy(ACK_STATE_DTYPE), self.dtx.numpy(DATAGEN_STATE_DTYPE), self.rto.numpy(RTO_REC_DTYPE),
               self.seg_sid.numpy(np.uint32), self.seg_start.numpy(np.uint32), self.seg_stop.numpy(np.uint32),
               self.nseg.numpy(np.uint32), self.total.numpy(np.uint64))
        assert int(got[6][0]) == nseg and got[7].tolist() == total.tolist(), (what, got[6], got[7], nseg, total)
        for g, e, name in zip(got, (snd, dtx, rec, seg_sid, seg_start, seg_stop), ("snd", "dtx", "rto", "seg_sid",
                                                                                   "seg_start", "seg_stop")):
            g = g[:nseg] if name in ("rto", "seg_sid") else g
            if g.tobytes() != e.tobytes():
                bad = [i for i in range(len(e)) if g[i].tobytes() != e[i].tobytes()]
                raise AssertionError(f"{what}: {len(bad)} of {len(e)} {name} records differ, first at {bad[0]}: "
                                     f"{g[bad[0]]} want {e[bad[0]]}")
        assert (got[2][nseg:].view(np.uint8) == SENT).all() and (got[3][nseg:].view(np.uint8) == SENT).all(), \
            f"{what}: entries past handled were written"
        return got


def sweep(gpu, ctx, snd, dtx, cur_ts, cap, kernel=None, what="", work_fill=SENT):
    want = rm.sweep(snd, dtx, cur_ts, cap)
    c = Call(gpu, snd, dtx, cap, work_fill)
    c.run(ctx, cur_ts)
    got = c.check(want, what)
    if kernel:
        assert ctx.last_kernel == kernel, (what, ctx.last_kernel)
    return want, got


def edge_ids(n):
    """Both sides of every wave edge and tile edge, the first and the last id."""
    e = {0, n - 1}
    for k in list(range(64, n, 64)) + list(range(TILE, n, TILE)) + list(range(1024, n, 1024)):
        e |= {k - 1, k}
    return sorted(i for i in e if 0 <= i < n)


COUNTS = [1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 3 * TILE + 5]


@pytest.mark.parametrize("n,form", [(n, f) for n in COUNTS for f in ("one", "many") if f == "many" or n <= TILE])
def test_stream_counts_and_where_the_due_streams_sit(gpu, ctx, n, form):
    cap = min(n, TILE) if form == "one" else TILE + 1 + n       # a cap above the tile forces the three launches
    kernel = ONE if form == "one" else MANY
    cur_ts = 0xFFFFFFF0 if n % 2 else 12345                     # some past the 2^32 wrap of cur_ts - ts_rto
    base = streams(n, n, cur_ts)
    rng = np.random.default_rng(n)
    patterns = {"none": [], "all": range(n), "first": [0], "last": [n - 1], "edges": edge_ids(n),
                "random": np.flatnonzero(rng.random(n) < 0.3)}
    for name, ids in patterns.items():
        snd, dtx = base[0].copy(), base[1].copy()
        make_due(snd, list(ids), cur_ts, rng)
        want, _ = sweep(gpu, ctx, snd, dtx, cur_ts, cap, kernel, f"{n} streams, {name} due, {form}")
        assert want[6] == min(len(list(ids)), cap) and int(want[7][0]) == len(list(ids))


@pytest.mark.parametrize("n,form", [(257, "one"), (TILE, "one"), (TILE + 1, "many"), (3 * TILE + 5, "many")])
def test_the_cap_and_a_second_sweep_for_the_rest(gpu, ctx, n, form):
    cur_ts = 777
    snd, dtx = streams(n, 100 + n, cur_ts)
    rng = np.random.default_rng(n)
    ids = np.unique(np.concatenate([edge_ids(n), np.flatnonzero(rng.random(n) < 0.01)]))
    make_due(snd, ids, cur_ts, rng)
    snd["nrtx"][ids] = rng.integers(0, 16, len(ids))            # all RETRANSMIT: a handled stream leaves the list
    snd["tcp_state"][ids], dtx["on_control_list"][ids] = 4, 0
    due = len(ids)
    assert due > 3
    for cap in (1, due - 1, due, due + 1):
        want, got = sweep(gpu, ctx, snd, dtx, cur_ts, cap, ONE if form == "one" else MANY, f"{n} streams, cap {cap}")
        assert want[6] == min(due, cap) and want[3].tolist() == ids[:cap].tolist()
        rest = ids[cap:]
        assert got[0][rest].tobytes() == snd[rest].tobytes() and got[1][rest].tobytes() == dtx[rest].tobytes()
        want2, _ = sweep(gpu, ctx, got[0].copy(), got[1].copy(), cur_ts, due, None, f"{n} streams, behind cap {cap}")
        assert want2[3].tolist() == rest.tolist()


def rebased(cur_ts, call=0):
    """Every stream of every fixture case as it stood before the case's first
    call, in one array: ts_rto moved so that the case's cur_ts becomes cur_ts."""
    recs = []
    for c in CASES:
        t = c["calls"][call][0]
        recs += [dict(b, ts_rto=(b["ts_rto"] - t + cur_ts) & rm.M32) for b in c["before"]]
    return rm.mirrors(recs)


def test_the_fixture_as_mirrors(gpu, ctx):
    for fam in (0, 1):                                          # every call, at the fixture's own times
        for i, c in enumerate(c for c in CASES if c["family"] == fam):
            snd, dtx = rm.mirrors(c["before"])
            for k, (cur_ts, recs) in enumerate(c["calls"]):
                want, got = sweep(gpu, ctx, snd, dtx, cur_ts, len(snd), ONE, f"family {fam} case {i} call {k}")
                assert set(want[3].tolist()) == {j for j, a in enumerate(recs) if a["fired"]}
                snd, dtx = got[0].copy(), got[1].copy()
    for cur_ts in (5000, 0xFFFFFFFF, 3):
        snd, dtx = rebased(cur_ts)
        fired = [bool(a["fired"]) for c in CASES for a in c["calls"][0][1]]
        for cap, kernel in ((len(snd), ONE), (TILE + 1, MANY)):
            want, _ = sweep(gpu, ctx, snd, dtx, cur_ts, cap, kernel, f"all cases at {cur_ts:#x}")
            assert want[3].tolist() == np.flatnonzero(fired).tolist()
            assert {rm.DEFER_STATE, rm.LOST, rm.RETRANSMIT} <= set(want[2]["verdict"].tolist())


def test_random_bytes_and_two_workspace_fills(gpu, ctx):
    rng = np.random.default_rng(7)
    for n, cap, kernel in ((3000, 3000, ONE), (2 * TILE + 77, 3 * TILE, MANY), (2 * TILE + 77, 50, MANY)):
        raw = rng.integers(0, 256, (n, 128), dtype=np.uint8)
        raw[:, 85] = rng.integers(0, 3, n)                      # on_rto 0, 1, 2
        raw[::3, 80] = 4                                        # a share ESTABLISHED
        raw[::2, 87] = 0
        snd = raw.view(ACK_STATE_DTYPE).reshape(-1).copy()
        sane = rng.random(n) < 0.5                              # a share past the BAD test
        snd["eff_mss"][sane] |= 1
        snd["wscale_peer"][sane] &= 31
        snd["sb_size"][sane] &= (1 << 30) - 1
        snd["sb_len"][sane] = snd["sb_len"][sane] % np.maximum(snd["sb_size"][sane], 1)
        snd["nrtx"][::5] = rng.integers(0, 19, len(snd[::5]))
        cur_ts = int(rng.integers(0, 1 << 32))
        dtx = rng.integers(0, 256, (n, 16), dtype=np.uint8).view(DATAGEN_STATE_DTYPE).reshape(-1).copy()
        ok = rng.random(n) < 0.8
        dtx["rsvd"][ok] = 0
        dtx["on_send_list"][ok] &= 1
        dtx["on_control_list"][ok] &= 1
        outs = []
        for fill in (0xFF, 0x00):
            want, got = sweep(gpu, ctx, snd, dtx, cur_ts, cap, kernel, f"random bytes, workspace {fill:#x}", fill)
            outs.append([a.tobytes() for a in got])
        assert outs[0] == outs[1]
        if cap >= n:
            assert set(want[2]["verdict"].tolist()) == {rm.BAD, rm.DEFER_STATE, rm.LOST, rm.RETRANSMIT}


def test_host_form_without_and_with_a_wait_limit(gpu, ctx):
    rng = np.random.default_rng(31)
    for n, cap in ((300, 40), (TILE + 9, TILE + 1)):
        cur_ts = 0xFFFFFFFE
        snd, dtx = streams(n, 31, cur_ts)
        make_due(snd, np.flatnonzero(rng.random(n) < 0.2), cur_ts, rng)
        want = rm.sweep(snd, dtx, cur_ts, cap)
        for limit in (0, 30_000_000):
            ctx.wait_limit = limit
            try:
                s, d = snd.copy(), dtx.copy()
                rto, seg_sid, seg_start, seg_stop, total = ctx.rto_sweep(s, d, cur_ts, cap)
            finally:
                ctx.wait_limit = 0
            for g, e, name in zip((s, d, rto, seg_sid, seg_start, seg_stop, total), want[:6] + (want[7],),
                                  ("snd", "dtx", "rto", "seg_sid", "seg_start", "seg_stop", "total")):
                assert g.tobytes() == e.tobytes(), (n, limit, name)


class Send:
    """The device arrays of mtcp_gpu_rto_send_dev over fixture-like streams."""

    def __init__(self, gpu, snd, dtx, cap, seed):
        self.n, self.cap, self.seg_cap = len(snd), cap, 4 * len(snd)
        self.state, self.tx0, self.payload = rm.send_side(self.n, seed)
        self.c = Call(gpu, snd, dtx, cap)
        self.tx = Guarded(32 * self.n, self.tx0)
        self.d_state, self.d_payload, self.d_links = to_dev(self.state), to_dev(self.payload), to_dev(LINKS)
        self.idx = torch.full((4 * cap,), 0x5A, dtype=torch.uint8, device=DEV)      # any values: no entry is read
        self.seg, self.desc = Guarded(48 * self.seg_cap), Guarded(8 * self.seg_cap)
        self.dres, self.dtotal, self.status = Guarded(16 * cap), Guarded(16), Guarded(self.seg_cap)
        self.image = Guarded(self.seg_cap * rm.SLOT)
        self.work = Guarded(gpu.Context.datagen_work_bytes(cap, self.n - 1))

    def run(self, ctx, cur_ts):
        c = self.c
        ctx.rto_send_dev(self.n - 1, c.snd.t, c.dtx.t, cur_ts, self.cap, *c.outs(), c.work.t, self.idx, self.d_state,
                         self.tx.t, self.d_payload, self.d_links, self.image.t, 0, 0, rm.SLOT, self.seg.t, self.desc.t,
                         self.seg_cap, self.dres.t, self.dtotal.t, self.status.t, self.work.t)

    def check(self, sw, dg, what):
        torch.cuda.synchronize()
        seg, desc, dres, total, snd2, tx2, dtx2, _ = dg
        self.c.check((snd2, dtx2) + sw[2:], what)               # the states as the data generation left them
        for name in ("tx", "seg", "desc", "dres", "dtotal", "status", "image", "work"):
            assert getattr(self, name).guard_intact(), f"{what}: bytes behind {name} were written"
        m = len(dres)
        for g, e, name in ((self.seg.numpy(TX_SEG_DTYPE), seg, "seg"), (self.desc.numpy(DESC_DTYPE), desc, "desc"),
                           (self.dres.numpy(DATAGEN_RES_DTYPE)[:m], dres, "dres"),
                           (self.dtotal.numpy(np.uint64), total, "total"), (self.tx.numpy(ACKGEN_STATE_DTYPE), tx2, "tx")):
            assert g.tobytes() == e.tobytes(), (what, name)
        assert (self.dres.numpy()[16 * m:] == SENT).all(), what


def test_rto_send_dev_down_to_the_frames(gpu, ctx):
    import oracle
    cur_ts = 0xFFFFFF00
    snd, dtx = rebased(cur_ts)
    n = len(snd)
    s = Send(gpu, snd, dtx, n + 3, 5)
    s.image.t.zero_()
    sw, dg = rm.send(snd, dtx, cur_ts, s.cap, s.state, s.tx0, len(s.payload), s.seg_cap)
    s.run(ctx, cur_ts)
    s.check(sw, dg, "first round")
    seg, desc, dres, total, snd2, tx2, dtx2, _ = dg
    T = int(total[0])
    assert 50 < T < s.seg_cap and {dm.SENT, dm.WINDOW, dm.DEFERRED, dm.BAD_BURST} <= set(dres["status"].tolist())
    image, status = xm.build_frames(seg, s.payload, LINKS.view(xm.LINK_DTYPE), desc, np.zeros(s.image.nbytes, np.uint8))
    assert s.image.numpy().tobytes() == image.tobytes() and s.status.numpy().tobytes() == status.tobytes()
    # the built frames parsed again: TCP_OK, each stream's first at its snd_una of before the sweep
    r2 = torch.zeros(40 * s.seg_cap, dtype=torch.uint8, device=DEV)
    ctx.rx_chunk_dev(s.image.t, s.desc.t, s.seg_cap, 0, r2)
    torch.cuda.synchronize()
    res = r2.cpu().numpy().view(RESULT_DTYPE)[:T]
    ref = oracle.rx_chunk(image, desc[:T].astype(oracle.DESC_DTYPE), 0, None)
    assert (ref["verdict"] == 0).all() and res.tobytes() == ref.tobytes()
    sent = []
    for r, dr in zip(sw[2], dres):
        if dr["n_seg"]:
            assert r["verdict"] == rm.RETRANSMIT and res[int(dr["first_seg"])]["seq"] == snd[int(r["sid"])]["snd_una"]
            sent.append(int(r["sid"]))
    assert len(sent) > 50
    # a second sweep once every re-armed timer has run out: the same streams, nrtx one higher, the doubled rto
    off = max(int(r) for r in snd2["rto"][sent] if r < 1 << 30)
    cur2 = (cur_ts + off) & rm.M32
    c2 = Send(gpu, snd2, dtx2, n + 3, 5)
    c2.tx = Guarded(32 * n, tx2)
    c2.image.t.zero_()
    sw2, dg2 = rm.send(snd2, dtx2, cur2, c2.cap, s.state, tx2, len(s.payload), c2.seg_cap)
    c2.run(ctx, cur2)
    c2.check(sw2, dg2, "second round")
    rec1 = {int(r["sid"]): r for r in sw[2]}
    again = [int(r["sid"]) for r in sw2[2] if int(r["sid"]) in rec1 and rec1[int(r["sid"])]["verdict"] == rm.RETRANSMIT]
    assert set(again) <= set(sent) and {j for j in sent if snd2[j]["rto"] <= off} <= set(again) and len(again) > 50
    doubled = 0
    for r in sw2[2]:
        r1 = rec1.get(int(r["sid"]))
        if r1 is None or r1["verdict"] != rm.RETRANSMIT:
            continue
        if r["verdict"] == rm.LOST:
            assert r1["nrtx"] == 16
            continue
        assert r["verdict"] == rm.RETRANSMIT and r["nrtx"] == r1["nrtx"] + 1
        b = snd[int(r["sid"])]
        base = ((int(b["srtt"]) >> 3) + int(b["rttvar"])) & rm.M32
        if r1["nrtx"] < 7 and 0 < base < (1 << 20):
            assert int(r["rto"]) == 2 * int(r1["rto"])
            doubled += 1
    assert doubled > 20


def test_error_returns(gpu, ctx):
    """MTCP_GPU_EINVAL for each misuse the header lists, for every pointer of
    mtcp_gpu_rto_sweep_dev, mtcp_gpu_rto_send_dev and mtcp_gpu_rto_sweep; a
    refused call launches nothing and writes nothing.  MTCP_GPU_EIO on an
    abandoned context is not tested: a context is abandoned only by a call that
    outlasts its wait limit, which takes a stalled GPU."""
    from mtcp_amd._lib import lib
    L = lib()
    cur_ts, n, cap = 99, 300, 64
    rng = np.random.default_rng(41)
    snd, dtx = streams(n, 41, cur_ts)
    make_due(snd, np.flatnonzero(rng.random(n) < 0.3), cur_ts, rng)
    s = Send(gpu, snd, dtx, cap, 41)
    c = s.c
    room = Guarded(64)                                          # misaligned stand-ins, never dereferenced
    p = lambda t, off=0: t.data_ptr() + off

    def dev(cx=ctx._h, mx=n - 1, sn=p(c.snd.t), dt=p(c.dtx.t), cp=cap, ro=p(c.rto.t), ss=p(c.seg_sid.t),
            st=p(c.seg_start.t), sp=p(c.seg_stop.t), ns=p(c.nseg.t), to=p(c.total.t), w=p(c.work.t), wbytes=c.wb):
        return L.mtcp_gpu_rto_sweep_dev(cx, mx, sn, dt, cur_ts, cp, ro, ss, st, sp, ns, to, w, wbytes, None)

    def send(cx=ctx._h, mx=n - 1, sn=p(c.snd.t), dt=p(c.dtx.t), cp=cap, ro=p(c.rto.t), to=p(c.total.t), rw=p(c.work.t),
             rwbytes=c.wb, i=p(s.idx), sta=p(s.d_state), tx=p(s.tx.t), pl=p(s.d_payload), lk=p(s.d_links), nl=3,
             bf=p(s.image.t), bo=0, sh=0, sb=rm.SLOT, fl=0, sg=p(s.seg.t), scap=s.seg_cap, dr=p(s.dres.t),
             dto=p(s.dtotal.t), su=p(s.status.t), w=p(s.work.t), wbytes=s.work.nbytes):
        return L.mtcp_gpu_rto_send_dev(cx, mx, sn, dt, cur_ts, cp, ro, p(c.seg_sid.t), p(c.seg_start.t), p(c.seg_stop.t),
                                       p(c.nseg.t), to, rw, rwbytes, i, sta, tx, pl, len(s.payload), lk, nl, bf, bo,
                                       s.image.nbytes, sh, sb, 0, fl, sg, p(s.desc.t), scap, dr, dto, su, w, wbytes, None)

    h_snd, h_dtx = snd.copy(), dtx.copy()
    h = {k: np.full(sz, SENT, np.uint8) for k, sz in (("rto", 16 * cap), ("sid", 4 * cap), ("start", 4 * cap + 4),
                                                      ("stop", 4 * cap), ("nseg", 4), ("total", 16))}
    hp = lambda a: a.ctypes.data

    def host(cx=ctx._h, mx=n - 1, sn=hp(h_snd), dt=hp(h_dtx), cp=cap, ro=hp(h["rto"]), ss=hp(h["sid"]),
             st=hp(h["start"]), sp=hp(h["stop"]), ns=hp(h["nseg"]), to=hp(h["total"])):
        return L.mtcp_gpu_rto_sweep(cx, mx, sn, dt, cur_ts, cp, ro, ss, st, sp, ns, to)

    bad = {
        "ctx NULL": dev(cx=None), "snd NULL": dev(sn=None), "dtx NULL": dev(dt=None), "rto NULL": dev(ro=None),
        "seg_sid NULL": dev(ss=None), "seg_start NULL": dev(st=None), "seg_stop NULL": dev(sp=None),
        "nseg NULL": dev(ns=None), "total NULL": dev(to=None), "work NULL": dev(w=None),
        "snd misaligned by 64": dev(sn=p(c.snd.t, 64)), "dtx misaligned by 8": dev(dt=p(c.dtx.t, 8)),
        "rto misaligned by 8": dev(ro=p(c.rto.t, 8)), "seg_sid misaligned": dev(ss=p(room.t, 2)),
        "seg_start misaligned": dev(st=p(room.t, 1)), "seg_stop misaligned": dev(sp=p(room.t, 3)),
        "nseg misaligned": dev(ns=p(room.t, 2)), "total misaligned": dev(to=p(room.t, 4)),
        "work misaligned": dev(w=p(c.work.t, 8)), "cap 0": dev(cp=0), "cap too large": dev(cp=MAX_CAP + 1),
        "max_id too large": dev(mx=MAX_ID + 1), "work too small": dev(wbytes=c.wb - 1), "no work bytes": dev(wbytes=0),
        "send: ctx NULL": send(cx=None), "send: snd NULL": send(sn=None), "send: dtx NULL": send(dt=None),
        "send: rto NULL": send(ro=None), "send: total NULL": send(to=None), "send: sweep work NULL": send(rw=None),
        "send: sweep work too small": send(rwbytes=c.wb - 1), "send: cap 0": send(cp=0),
        "send: cap too large": send(cp=MAX_CAP + 1), "send: max_id too large": send(mx=MAX_ID + 1),
        "send: idx NULL": send(i=None), "send: state NULL": send(sta=None), "send: tx NULL": send(tx=None),
        "send: payload NULL": send(pl=None), "send: links NULL": send(lk=None), "send: buf NULL": send(bf=None),
        "send: seg NULL": send(sg=None), "send: dres NULL": send(dr=None), "send: data total NULL": send(dto=None),
        "send: status NULL": send(su=None), "send: work NULL": send(w=None),
        "send: work too small": send(wbytes=s.work.nbytes - 1), "send: tx misaligned": send(tx=p(s.tx.t, 16)),
        "send: links misaligned": send(lk=p(s.d_links, 2)), "send: unknown builder flags": send(fl=2),
        "send: seg_cap 0": send(scap=0), "send: off_shift 17": send(sh=17), "send: n_links 0": send(nl=0),
        "send: slot below 67": send(sb=66), "send: buf_off odd": send(bo=1),
        "host: ctx NULL": host(cx=None), "host: snd NULL": host(sn=None), "host: dtx NULL": host(dt=None),
        "host: rto NULL": host(ro=None), "host: seg_sid NULL": host(ss=None), "host: seg_start NULL": host(st=None),
        "host: seg_stop NULL": host(sp=None), "host: nseg NULL": host(ns=None), "host: total NULL": host(to=None),
        "host: cap 0": host(cp=0), "host: cap too large": host(cp=MAX_CAP + 1), "host: max_id too large": host(mx=MAX_ID + 1),
    }
    assert {k: v for k, v in bad.items() if v != EINVAL} == {}
    torch.cuda.synchronize()
    for g in (c.rto, c.seg_sid, c.seg_start, c.seg_stop, c.nseg, c.total, c.work, s.seg, s.desc, s.dres, s.dtotal,
              s.status, s.image, s.work):                       # none of these wrote anything
        assert (g.all == SENT).all().item()
    assert c.snd.numpy().tobytes() == snd.tobytes() and c.dtx.numpy().tobytes() == dtx.tobytes()
    assert s.tx.numpy().tobytes() == s.tx0.tobytes()
    assert all((a == SENT).all() for a in h.values()) and h_snd.tobytes() == snd.tobytes() and h_dtx.tobytes() == dtx.tobytes()
    wb = gpu.Context.rto_sweep_work_bytes
    assert wb(7, 0) == 0 and wb(7, MAX_CAP + 1) == 0 and wb(MAX_ID + 1, 7) == 0 and wb(MAX_ID, MAX_CAP) > 0
    want = rm.sweep(snd, dtx, cur_ts, cap)
    assert dev() == 0 and host() == 0                           # and the same arguments, valid, work
    c.check(want, "after the refused calls")
    for g, e in ((h_snd, want[0]), (h_dtx, want[1]), (h["rto"][:16 * want[6]], want[2]), (h["sid"][:4 * want[6]], want[3]),
                 (h["start"], want[4]), (h["stop"], want[5]), (h["total"], want[7])):
        assert g.tobytes() == e.tobytes()
    assert h["nseg"].view(np.uint32)[0] == want[6] and (h["rto"][16 * want[6]:] == SENT).all()
