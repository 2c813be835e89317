"""The batched application write on the GPU (include/mtcp_gpu_sndwrite.h,
mtcp_amd/csrc/sndwrite_kernels.hpp): every byte of d_wres, d_snd, d_dtx, the
arena (guard bands included), the table and d_total of every case is compared
with tests/sndwrite_model.py; none is sampled.

Every chunk and every source range has 64 B guard bands
(tests/sndwrite_cases.py), the outputs have guards behind them, the workspace
is exactly sized and holds 0xA5.  The reference-written fixture operation by
operation; every source alignment x destination alignment x length 1-48; the
lengths around one and two copy units; a 1 MiB write beside 1-byte writes;
compaction at the head_off and moved-length edges with the destination over the
old window; request counts around the wave and the plan workgroup; every verdict
in one batch; duplicates whose winner is BAD_REQ or EAGAIN; random bytes in
every record array; four workspace fills; sb_len == 0 with a stale sb_base_seq;
the source in registered host memory; write_send_dev down to frames that parse
again, the peer's ACK frames for half of them through rx, lookup, group, the
receive walk and the ACK walk, a second write that compacts and an RTO sweep
that retransmits from snd_una, with no host refresh; the captured write_send
set replayed twice; the
host form unbounded, bounded and behind a stalled GPU; every error return.  The
move has one form (a wave per request)."""
import time

import numpy as np
import pytest

import oracle
from mtcp_amd._types import (ACK_STATE_DTYPE, ACKGEN_STATE_DTYPE, DATAGEN_RES_DTYPE, DATAGEN_STATE_DTYPE, DESC_DTYPE,
                             FLOW_NONE, RESULT_DTYPE, SNDWRITE_COMPACTED, SNDWRITE_REQ_DTYPE, SNDWRITE_RES_DTYPE,
                             TX_SEG_DTYPE)
from tests import datagen_model as dm
from tests import group_model as gm
from tests import rtosweep_model as rs
from tests import sndwrite_cases as sc
from tests import sndwrite_model as sm
from tests import txbuild_model as xm
from tests.test_gpu_datagen import LINKS

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EINVAL, EIO, ETIMEDOUT = -22, -5, -110
GUARD = 4096
SENT = 0xA5
UNIT = sm.UNIT
WG = 256                                               # sndwrite_kernels.hpp: requests per plan workgroup


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")
    from mtcp_amd import gpu as g
    assert g.Context.sndwrite_tile() == UNIT
    return g


@pytest.fixture(scope="module")
def ctx(gpu):
    with gpu.Context(0) as c:
        yield c


def to_dev(a: np.ndarray):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)


class Guarded:
    """`nbytes` of device memory holding `fill` and a guard region of SENT behind it."""

    def __init__(self, nbytes, fill=SENT):
        self.nbytes = nbytes
        self.all = torch.full((nbytes + GUARD,), SENT, dtype=torch.uint8, device=DEV)
        self.t = self.all[:nbytes]
        if isinstance(fill, np.ndarray):
            self.t.copy_(to_dev(fill))
        elif fill != SENT:
            self.t.fill_(fill)

    def guard_intact(self):
        return bool((self.all[self.nbytes:] == SENT).all().item())

    def numpy(self, dtype=np.uint8):
        return self.t.cpu().numpy().view(dtype)


class Call:
    """The device arrays of one call on a sndwrite_cases.Batch, the outputs guarded."""
    OUT = ("snd", "dtx", "payload", "wres", "seg_sid", "seg_start", "seg_stop", "nseg", "total", "work")

    def __init__(self, gpu, b, work_fill=SENT):
        self.b, self.n = b, len(b.wreq)
        n = max(self.n, 1)
        self.wreq = to_dev(b.wreq) if self.n else torch.zeros(32, dtype=torch.uint8, device=DEV)
        self.snd, self.dtx = Guarded(b.snd.nbytes, b.snd), Guarded(b.dtx.nbytes, b.dtx)
        self.src, self.payload = to_dev(b.src), Guarded(len(b.payload), b.payload)
        self.wres, self.total = Guarded(16 * n), Guarded(16)
        self.seg_sid, self.seg_start, self.seg_stop, self.nseg = Guarded(4 * n), Guarded(4 * n + 4), Guarded(4 * n), Guarded(4)
        self.wb = gpu.Context.sndwrite_work_bytes(self.n, b.max_id)
        assert self.wb > 0
        self.work = Guarded(self.wb, work_fill)

    def outs(self):
        return (self.wres.t, self.seg_sid.t, self.seg_start.t, self.seg_stop.t, self.nseg.t, self.total.t, self.work.t)

    def run(self, ctx, stream=None, src=None, src_bytes=None):
        ctx.sndwrite_dev(self.wreq, self.n, self.b.max_id, self.snd.t, self.dtx.t, self.src if src is None else src,
                         self.payload.t, *self.outs(), src_bytes=src_bytes, stream=stream)

    def raw(self):
        n = self.n
        return (self.snd.numpy().copy(), self.dtx.numpy().copy(), self.payload.numpy().copy(),
                self.wres.numpy()[:16 * n].copy(), self.seg_sid.numpy()[:4 * n].copy(),
                self.seg_start.numpy()[:4 * n + 4].copy(), self.seg_stop.numpy()[:4 * n].copy(),
                self.nseg.numpy().copy(), self.total.numpy().copy())

    def check(self, want=None, what=""):
        b = self.b
        want = b.expect() if want is None else want
        for name in self.OUT:
            assert getattr(self, name).guard_intact(), f"{what}: bytes behind {name} were written"
        snd, dtx, payload, wres, seg_sid, seg_start, seg_stop, nseg, total = self.raw()
        w_snd, w_dtx, w_payload, w_wres, w_sid, w_start, w_stop, w_nseg, w_total = want
        got_r = wres.view(SNDWRITE_RES_DTYPE)
        if wres.tobytes() != w_wres.tobytes():
            bad = np.nonzero(got_r != w_wres)[0]
            raise AssertionError(f"{what}: {len(bad)} of {self.n} results differ, first {bad[0]}: {got_r[bad[0]]} want "
                                 f"{w_wres[bad[0]]} for {b.wreq[bad[0]]}")
        for name, g, w, dt in (("snd", snd, w_snd, ACK_STATE_DTYPE), ("dtx", dtx, w_dtx, DATAGEN_STATE_DTYPE)):
            if g.tobytes() != w.tobytes():
                k = np.nonzero(g.view(dt) != w)[0][0]
                raise AssertionError(f"{what}: {name} of stream {k}: {g.view(dt)[k]} want {w[k]}")
        bad = np.nonzero(payload != w_payload)[0]
        assert len(bad) == 0, f"{what}: {len(bad)} arena bytes differ, first at {bad[0]}: {payload[bad[0]]} want " \
                              f"{w_payload[bad[0]]} (chunks at {b.chunks[:4]}...)"
        assert seg_sid.view(np.uint32).tolist() == w_sid.tolist(), f"{what}: seg_sid"
        assert seg_start.view(np.uint32).tolist() == w_start.tolist() and seg_stop.view(np.uint32).tolist() == w_stop.tolist()
        assert nseg.view(np.uint32).tolist() == w_nseg.tolist(), f"{what}: nseg"
        assert total.view(np.uint64).tolist() == w_total.tolist(), f"{what}: totals"
        assert self.src.cpu().numpy().tobytes() == b.src.tobytes(), f"{what}: the source was written"
        return want


def run(gpu, ctx, b, what="", work_fill=SENT):
    c = Call(gpu, b, work_fill)
    c.run(ctx)
    torch.cuda.synchronize()
    c.check(what=what)
    return c


def verdicts_of(c):
    return c.raw()[3].view(SNDWRITE_RES_DTYPE)["verdict"]


# ---- the fixture ------------------------------------------------------------------------------------------
def test_the_fixture_operation_by_operation(gpu, ctx):
    """Every case of tests/golden/sndwrite_cases.bin is a stream.  A round takes
    every case to its next SBPut (the SBRemoves in between are the record updates
    the ACK walk makes) and runs those puts as one batch.  The GPU's bytes are
    the model's; the return value, the offsets and every byte of every chunk are
    the reference's."""
    cases = sm.load_fixture()
    bufs = [sm.SendBuf(c["size"], c["init_seq"]) for c in cases]
    b = sc.lay_out(bufs, rng=np.random.default_rng(0), stale_base=[c["init_seq"] ^ 0xBEEF for c in cases])
    pos, serial = [0] * len(cases), [0] * len(cases)
    rounds = checked = 0

    def against_the_reference(ci, op):
        off, size = b.chunks[ci]
        head, tail = sm.offsets_of(b.snd[ci], b.dtx[ci])
        h, t, ln, _, head_seq = op["after"]
        assert (head, int(b.snd["sb_len"][ci]), int(b.snd["sb_head_seq"][ci])) == (h, ln, head_seq), (rounds, ci)
        assert ln == 0 or tail == t
        assert (b.payload[off:off + size] == op["data"]).all(), (rounds, ci)

    while True:
        puts = {}
        for ci, c in enumerate(cases):
            while pos[ci] < len(c["ops"]) and c["ops"][pos[ci]]["kind"] == "rem":
                op = c["ops"][pos[ci]]
                if op["ret"] > 0:
                    b.snd["sb_head_seq"][ci] = (int(b.snd["sb_head_seq"][ci]) + op["ret"]) & sm.M32
                    b.snd["sb_len"][ci] -= op["ret"]
                against_the_reference(ci, op)
                pos[ci] += 1
            if pos[ci] < len(c["ops"]):
                puts[ci] = c["ops"][pos[ci]]
                pos[ci] += 1
        if not puts:
            break
        ids = sorted(puts)
        b.snd["snd_wnd"][ids] = [cases[ci]["size"] for ci in ids]          # open windows: SBPut's own clamp decides
        data = {k: sm.payload_bytes(ci, serial[ci], puts[ci]["len"]) for k, ci in enumerate(ids)}
        for ci in ids:
            serial[ci] += 1
        b.requests(ids, [puts[ci]["len"] for ci in ids], rng=np.random.default_rng(rounds), fill=lambda i, n: data[i])
        c = run(gpu, ctx, b, f"fixture round {rounds}")
        snd, dtx, payload, wres = c.raw()[:4]
        b.snd, b.dtx, b.payload = snd.view(ACK_STATE_DTYPE).copy(), dtx.view(DATAGEN_STATE_DTYPE).copy(), payload
        wres = wres.view(SNDWRITE_RES_DTYPE)
        for k, ci in enumerate(ids):
            op = puts[ci]
            assert int(wres["written"][k]) == max(op["ret"], 0), (rounds, ci)
            assert int(wres["verdict"][k]) == (sm.WRITTEN if op["ret"] > 0 else sm.FULL), (rounds, ci)
            against_the_reference(ci, op)
            checked += 1
        rounds += 1
    assert checked > 200 and rounds >= 10


# ---- alignment and length ---------------------------------------------------------------------------------
def test_every_alignment_and_short_length(gpu, ctx):
    """16 source x 16 destination alignments x lengths 1-48, one stream each."""
    rng = np.random.default_rng(1)
    sa, da, ln = (a.reshape(-1) for a in np.meshgrid(np.arange(16), np.arange(16), np.arange(1, 49), indexing="ij"))
    n = len(ln)
    held = rng.integers(1, 12, size=n)
    bufs = [sc.buffer(rng, 64, int(h)) for h in held]
    b = sc.lay_out(bufs, chunk_align=(da - held) & 15)
    b.requests(np.arange(n), ln, src_align=sa, rng=rng)
    assert (b.wreq["src_off"] % 16 == sa).all()
    assert ((b.dtx["sb_off"] + b.snd["sb_len"]) % 16 == da).all()
    c = run(gpu, ctx, b, "alignments")
    assert (verdicts_of(c) == sm.WRITTEN).all() and int(c.raw()[8].view(np.uint64)[0]) == n


def test_lengths_around_one_and_two_units(gpu, ctx):
    """to_put at the unit - 1, the unit, the unit + 1 and the same around two
    units, at destination phases 0, 1, 9 and 15 and source phases 0 and 7."""
    rng = np.random.default_rng(2)
    cases = [(ln, da, sa) for ln in (UNIT - 17, UNIT - 1, UNIT, UNIT + 1, 2 * UNIT - 16, 2 * UNIT - 1, 2 * UNIT, 2 * UNIT + 1)
             for da in (0, 1, 9, 15) for sa in (0, 7)]
    ln, da, sa = (np.array(x) for x in zip(*cases))
    bufs = [sc.buffer(rng, 3 * UNIT, 100) for _ in ln]
    b = sc.lay_out(bufs, chunk_align=(da - 100) & 15)
    b.requests(np.arange(len(ln)), ln, src_align=sa, rng=rng)
    c = run(gpu, ctx, b, "units")
    assert (verdicts_of(c) == sm.WRITTEN).all()
    want_units = [sm.units(int(d["sb_off"]) + 100, int(l)) for d, l in zip(b.dtx, ln)]
    assert {1, 2, 3} <= set(want_units)


def test_one_megabyte_write_beside_one_byte_writes(gpu, ctx):
    rng = np.random.default_rng(3)
    n = 65
    bufs = [sc.buffer(rng, (1 << 20) + 64 if i == 32 else 64, int(rng.integers(0, 60))) for i in range(n)]
    b = sc.lay_out(bufs, rng=rng)
    lens = np.ones(n, dtype=np.int64)
    lens[32] = 1 << 20
    b.requests(np.arange(n), lens, rng=rng)
    c = run(gpu, ctx, b, "1 MiB")
    assert c.raw()[8].view(np.uint64).tolist() == [n, (1 << 20) + 64]


def test_compaction_at_the_head_off_and_moved_length_edges(gpu, ctx):
    """The memmove of tcp_send_buffer.c:136 with the window at head_off 1, 15,
    16, 17 and size - 1 and 1, 15, 16, 17, 1 023-1 025 and 2 047-2 049 bytes
    long; every put fills the chunk, so its destination [len, size) lies over
    the old window [head_off, head_off + len)."""
    rng = np.random.default_rng(4)
    moved = (1, 15, 16, 17, 1023, 1024, 1025, 2047, 2048, 2049)
    shape = [(h, m, h + m + int(rng.integers(0, 40))) for h in (1, 15, 16, 17) for m in moved]
    shape += [(size - 1, 1, size) for size in (48, 64, 4096)] + [(3000, 1024, 4096), (5, 2048, 2053)]
    bufs = [sc.buffer(rng, size, m, head_off=h) for h, m, size in shape]
    b = sc.lay_out(bufs, rng=rng)
    b.requests(np.arange(len(shape)), [size for _, _, size in shape], rng=rng)
    c = run(gpu, ctx, b, "compaction")
    wres = c.raw()[3].view(SNDWRITE_RES_DTYPE)
    assert (wres["verdict"] == sm.WRITTEN).all() and (wres["flags"] & SNDWRITE_COMPACTED).all()
    assert (wres["written"] == [size - m for _, m, size in shape]).all() and (wres["snd_wnd"] == 0).all()


@pytest.mark.parametrize("n", [1, 63, 64, 65, WG - 1, WG, WG + 1, 3 * WG + 7])
def test_request_counts_around_the_wave_and_the_workgroup(gpu, ctx, n):
    rng = np.random.default_rng(100 + n)
    b = sc.random_batch(rng, max(n // 2, 1), n, sizes=(64, 256, 1024), dup=0.1)
    run(gpu, ctx, b, f"n={n}")


# ---- the verdict chain ---------------------------------------------------------------------------------
def test_every_verdict_in_one_batch(gpu, ctx):
    rng = np.random.default_rng(5)
    b = sc.random_batch(rng, 150, 400, dup=0.2)
    want = run(gpu, ctx, b, "verdicts").b.expect()
    assert set(want[3]["verdict"].tolist()) == set(range(1, 10))
    assert {1, 2, 4} <= {f & m for f in want[3]["flags"].tolist() for m in (1, 2, 4)}


def test_bad_requests_and_the_int_window(gpu, ctx):
    """sid above max_id, each reserved word, a flag bit, len above 2^31 - 1, the
    source range one byte past the region and at the exact fit; snd_wnd at 0, 1,
    2^31 - 1, 2^31 and 2^32 - 1."""
    rng = np.random.default_rng(6)
    bufs = [sc.buffer(rng, 256, 10) for _ in range(14)]
    wnd = [246] * 9 + [0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]
    b = sc.lay_out(bufs, rng=rng, snd_wnd=wnd)
    b.requests(np.arange(14), [10] * 9 + [100] * 5, rng=rng)
    b.wreq["sid"][0] = 14
    b.wreq["rsvd"][1, 0], b.wreq["rsvd"][2, 1], b.wreq["rsvd"][3, 2] = 1, 1 << 31, 7
    b.wreq["flags"][4] = 1
    b.wreq["len"][5] = 0x80000000
    end = len(b.src)
    b.wreq["src_off"][6], b.wreq["src_off"][7], b.wreq["src_off"][8] = end - 9, end - 10, (1 << 64) - 5
    want = run(gpu, ctx, b, "bad requests").b.expect()
    assert want[3]["verdict"].tolist() == [sm.BAD_REQ] * 7 + [sm.WRITTEN, sm.BAD_REQ, sm.EAGAIN, sm.WRITTEN, sm.WRITTEN,
                                                               sm.EAGAIN, sm.EAGAIN]
    assert want[3]["written"][[10, 11]].tolist() == [1, 100]


@pytest.mark.parametrize("winner", ["BAD_REQ", "EAGAIN", "WRITTEN"])
def test_duplicates(gpu, ctx, winner):
    """The lowest index of a sid wins whatever its own verdict is."""
    rng = np.random.default_rng(7)
    n = 70
    bufs = [sc.buffer(rng, 128, int(rng.integers(0, 100))) for _ in range(n)]
    wnd = [128 - x.len for x in bufs]
    if winner == "EAGAIN":
        wnd[5] = 0
    b = sc.lay_out(bufs, rng=rng, snd_wnd=wnd)
    sids = np.arange(n)
    sids[40], sids[69], sids[1] = 5, 5, 0
    b.requests(sids, rng.integers(1, 200, size=n), rng=rng)
    if winner == "BAD_REQ":
        b.wreq["rsvd"][5, 1] = 9
    want = run(gpu, ctx, b, winner).b.expect()
    assert np.nonzero(want[3]["verdict"] == sm.DUP)[0].tolist() == [1, 40, 69]
    assert want[3]["verdict"][5] == getattr(sm, winner)


def test_an_empty_buffer_with_a_stale_base_seq(gpu, ctx):
    """sb_len == 0: head_off is 0 whatever sb_base_seq holds, and the write sets sb_base_seq = sb_head_seq."""
    rng = np.random.default_rng(8)
    n = 40
    bufs = [sc.buffer(rng, 256, 0) for _ in range(n)]
    b = sc.lay_out(bufs, rng=rng, stale_base=rng.integers(0, 1 << 32, size=n).tolist())
    b.requests(np.arange(n), rng.integers(1, 300, size=n), rng=rng)
    c = run(gpu, ctx, b, "stale base")
    dtx = c.raw()[1].view(DATAGEN_STATE_DTYPE)
    assert (verdicts_of(c) == sm.WRITTEN).all() and (dtx["sb_base_seq"] == b.snd["sb_head_seq"]).all()


def test_random_bytes_in_every_record_array(gpu, ctx):
    rng = np.random.default_rng(9)
    seen = set()
    for trial in range(4):
        b = sc.random_records(rng, 96, 300, slot=2048, src_bytes=1 << 14)
        c = run(gpu, ctx, b, f"random records {trial}")
        seen |= set(verdicts_of(c).tolist())
    assert seen == set(range(1, 10)), seen


def test_four_workspace_fills_give_identical_bytes(gpu, ctx):
    rng = np.random.default_rng(10)
    b = sc.random_batch(rng, 50, 300, dup=0.3)
    outs = [run(gpu, ctx, b, f"fill {fill:#x}", work_fill=fill).raw() for fill in (0x00, 0xFF, SENT, 0x01)]
    for o in outs[1:]:
        for x, y in zip(outs[0], o):
            assert x.tobytes() == y.tobytes()


def test_the_source_in_registered_host_memory(gpu, ctx):
    rng = np.random.default_rng(11)
    b = sc.random_batch(rng, 40, 100, dup=0.1)
    c = Call(gpu, b)
    h = np.zeros(len(b.src) + 64, np.uint8)
    h = h[(-h.ctypes.data) % 64:][:len(b.src)]
    h[:] = b.src
    gpu.host_register(h)
    try:
        c.run(ctx, src=h.ctypes.data, src_bytes=len(h))
        torch.cuda.synchronize()
        c.check(what="host source")
        assert h.tobytes() == b.src.tobytes()
    finally:
        gpu.host_unregister(h)


# ---- the chain ---------------------------------------------------------------------------------------------
class Send:
    """The device arrays of mtcp_gpu_write_send_dev for a sndwrite_cases.Batch of n requests."""

    def __init__(self, gpu, b, seed, snd=None, dtx=None, payload=None, tx=None):
        self.b, self.n, self.ns = b, len(b.wreq), len(b.snd)
        self.seg_cap = 8 * self.n + 8
        self.state, self.tx0, _ = rs.send_side(self.ns, seed)
        if tx is not None:
            self.tx0 = tx
        self.c = Call(gpu, b)
        if snd is not None:                           # the records and the arena a call before this one left
            self.c.snd, self.c.dtx, self.c.payload = snd, dtx, payload
        self.tx = Guarded(32 * self.ns, self.tx0)
        self.d_state, self.d_links = to_dev(self.state), to_dev(LINKS)
        self.idx = torch.full((4 * self.n,), 0x5A, dtype=torch.uint8, device=DEV)     # any values: no entry is read
        self.seg, self.desc = Guarded(48 * self.seg_cap), Guarded(8 * self.seg_cap)
        self.dres, self.dtotal, self.status = Guarded(16 * self.n), Guarded(16), Guarded(self.seg_cap)
        self.image = Guarded(self.seg_cap * rs.SLOT, 0)
        self.work = Guarded(gpu.Context.datagen_work_bytes(self.n, self.ns - 1))
        self.r2 = torch.zeros(40 * self.seg_cap, dtype=torch.uint8, device=DEV)

    def run(self, ctx, cur_ts, stream=None):
        c = self.c
        ctx.write_send_dev(c.wreq, self.n, self.ns - 1, c.snd.t, c.dtx.t, c.src, c.payload.t, *c.outs(), self.idx,
                           self.d_state, self.tx.t, cur_ts, self.d_links, self.image.t, 0, 0, rs.SLOT, self.seg.t,
                           self.desc.t, self.seg_cap, self.dres.t, self.dtotal.t, self.status.t, self.work.t,
                           stream=stream)
        ctx.rx_chunk_dev(self.image.t, self.desc.t, self.seg_cap, 0, self.r2, stream=stream)

    def expect(self, snd, dtx, payload, tx, cur_ts):
        """The models chained: the write on (snd, dtx, payload), then the data generation over its table."""
        snd, dtx, payload = snd.copy(), dtx.copy(), payload.copy()
        w = sm.write(self.b.wreq, self.ns - 1, snd, dtx, self.b.src, payload)
        dg = dm.datagen(None, None, self.n, self.ns - 1, np.zeros(self.n, np.uint32), w[1], w[2], int(w[4][0]), w[3],
                        self.state, snd, tx, dtx, cur_ts, len(payload), rs.N_LINKS, 0, self.seg_cap * rs.SLOT, 0, rs.SLOT,
                        self.seg_cap)
        return w, dg, payload

    def check(self, w, dg, payload, what):
        """Every byte of both calls' outputs; returns the frames' records."""
        seg, desc, dres, total, snd2, tx2, dtx2, _ = dg
        self.c.check((snd2, dtx2, payload) + w, what)             # the records as the data generation left them
        for name in ("tx", "seg", "desc", "dres", "dtotal", "status", "image", "work"):
            assert getattr(self, name).guard_intact(), f"{what}: bytes behind {name} were written"
        for g, e, name in ((self.seg.numpy(TX_SEG_DTYPE), seg, "seg"), (self.desc.numpy(DESC_DTYPE), desc, "desc"),
                           (self.dres.numpy(DATAGEN_RES_DTYPE), dres, "dres"), (self.dtotal.numpy(np.uint64), total, "total"),
                           (self.tx.numpy(ACKGEN_STATE_DTYPE), tx2, "tx")):
            assert g.tobytes() == e.tobytes(), (what, name)
        T = int(total[0])
        image, status = xm.build_frames(seg, payload, LINKS.view(xm.LINK_DTYPE), desc, np.zeros(self.image.nbytes, np.uint8))
        assert self.image.numpy().tobytes() == image.tobytes() and self.status.numpy().tobytes() == status.tobytes(), what
        res = self.r2.cpu().numpy().view(RESULT_DTYPE)[:T]
        ref = oracle.rx_chunk(image, desc[:T].astype(oracle.DESC_DTYPE), 0, None)
        assert (ref["verdict"] == 0).all() and res.tobytes() == ref.tobytes(), what
        return res, image, desc


def frames_bytes(res, image, desc, dres_row):
    """The payload bytes of one stream's frames, in sequence order, and the first frame's seq."""
    first, k = int(dres_row["first_seg"]), int(dres_row["n_seg"])
    out, seq0 = b"", int(res["seq"][first]) if k else None
    for j in range(first, first + k):
        assert int(res["seq"][j]) == (seq0 + len(out)) & sm.M32
        at = int(desc["offset"][j]) + int(desc["len"][j]) - int(res["payload_len"][j])
        out += image[at:at + int(res["payload_len"][j])].tobytes()
    return out, seq0


def chain_batch(rng, ns):
    """ns streams with 4 KiB buffers in different states, wide windows."""
    bufs = [sc.buffer(rng, 4096, int(rng.integers(0, 600)), head_off=0) for _ in range(ns)]
    b = sc.lay_out(bufs, rng=rng)
    b.snd["cwnd"], b.snd["peer_wnd"], b.snd["rto"] = 1 << 20, 1 << 20, rng.integers(100, 300, ns)
    b.snd["srtt"], b.snd["rttvar"], b.snd["ssthresh"] = 80, 10, 1 << 20
    return b


def ack_batch(tuples, state, snd, acked, ts_ref, cur_ts):
    """One pure ACK per stream, as the peer would send it for `acked` bytes past
    snd_una: seq = rcv_nxt, a timestamp option above ts_recent, window 60 000;
    built as tests/test_gpu_datagen_chain.py's chain builds its frames.  Returns
    the chunk, its descriptors, the table entries and what the rx, option,
    lookup, group, receive-walk and ACK-walk models give for it."""
    from mtcp_amd._types import TCPOPT_DTYPE
    from tests import ackwalk_model as am
    from tests import flowtab_model as fm
    from tests import rcvwalk_model as wm
    from tests import tcpopt_model as tm
    ns = len(snd)
    frames = []
    for i in range(ns):
        body = bytes([1, 1, 8, 10]) + ((int(state["ts_recent"][i]) + 5) & sm.M32).to_bytes(4, "big") + int(ts_ref).to_bytes(4, "big")
        f = tm.frame_raw(5, 8, 0x10, body, seed=i)
        f[26:34], f[34:38] = tuples[i][:8], tuples[i][8:12]
        f[38:42] = int(state["rcv_nxt"][i]).to_bytes(4, "big")
        f[42:46] = ((int(snd["snd_una"][i]) + int(acked[i])) & sm.M32).to_bytes(4, "big")
        f[48:50] = (60000).to_bytes(2, "big")
        frames.append(f)
    buf, desc = tm.pack_chunk(frames, slot=64)
    tm.fill_checksums(buf, desc)
    desc = desc.astype(oracle.DESC_DTYPE)
    res = oracle.rx_chunk(buf, desc, 0, None)
    assert (res["verdict"] == 0).all()
    opt = np.zeros(ns, TCPOPT_DTYPE)
    for i in range(ns):
        ihl, doff = int(res["ihl_doff"][i]) & 15, int(res["ihl_doff"][i]) >> 4
        first = int(desc["offset"][i]) + 34 + 4 * ihl
        avail = int(desc["offset"][i]) + int(desc["len"][i]) - first
        blk = np.zeros(64, np.uint8)
        take = max(0, min(64, avail))
        blk[:take] = buf[first:first + take]
        opt[i] = tm.expected_record(blk, 4 * doff - 20, int(res["tcp_flags"][i]), avail)
    ent = fm.entries(fm.record_keys(res), np.arange(ns, dtype=np.uint32))
    grp = gm.group(np.arange(ns, dtype=np.uint32), ns - 1)
    place, state_after, seg_stop = wm.walk(res, opt, ns - 1, *grp, state)
    ack, snd_after, ack_stop = am.walk(res, opt, place, ns - 1, *grp, cur_ts, snd)
    assert (ack["verdict"] == am.ACK_NEW).all() and (ack["rmlen"] == acked).all()
    return buf, desc, ent, state_after, snd_after, ack


def test_application_bytes_in_data_frames_out_with_no_host_refresh(gpu):
    """write_send_dev; the peer's ACK frames for half of what went out through
    rx, the option walk, lookup, group, the receive walk and the ACK walk; a
    second write_send_dev that compacts; rto_send_dev: one behind the other on
    one stream, nothing refreshed by the host and nothing waited for in
    between.  Every output byte of every call is the chained models'; the
    frames, parsed again by rx, carry the written bytes in sequence order, and
    the sweep's frames begin at snd_una with the right bytes."""
    rng = np.random.default_rng(12)
    ns = 24
    b = chain_batch(rng, ns)
    held = b.snd["sb_len"].astype(np.int64).copy()
    b.snd["saw_timestamp"] = 1
    b.requests(np.arange(ns), rng.integers(1000, 2000, size=ns), rng=rng)
    tuples = [rng.integers(1, 255, 12, dtype=np.uint8).tobytes() for _ in range(ns)]
    cur1, cur_ack, cur2, cur3 = 5000, 5040, 5050, 9000
    with gpu.Context(0) as cx, gpu.FlowTable(cx, 10) as tab:
        st = torch.cuda.Stream(device=DEV)
        s1 = Send(gpu, b, 21)
        s1.state["saw_timestamp"] = 1
        s1.d_state = to_dev(s1.state)
        # what the first call leaves, by the models: the peer acknowledges half of each stream's bytes in flight
        w1, dg1, pay1 = s1.expect(b.snd, b.dtx, b.payload, s1.tx0, cur1)
        snd1, tx1, dtx1 = dg1[4], dg1[5], dg1[6]
        k = ((snd1["snd_nxt"].astype(np.int64) - snd1["snd_una"]) & sm.M32) // 2
        assert (k > 400).all()
        abuf, adesc, ent, state_a, snd1a, ack_want = ack_batch(tuples, s1.state, snd1, k, cur1, cur_ack)
        assert (snd1a["sb_len"] == snd1["sb_len"] - k).all() and (snd1a["snd_una"] == (snd1["snd_una"] + k) & sm.M32).all()
        d_abuf, d_adesc, d_ent = to_dev(abuf), to_dev(adesc), to_dev(ent)
        d_res, d_opt = torch.zeros(40 * ns, dtype=torch.uint8, device=DEV), torch.zeros(16 * ns, dtype=torch.uint8, device=DEV)
        d_sid, grp = Guarded(4 * ns), (Guarded(4 * ns), Guarded(4 * ns), Guarded(4 * ns + 4), Guarded(4))
        gwork = Guarded(gpu.Context.group_work_bytes(ns, ns - 1))
        rwork = Guarded(gpu.Context.rcvwalk_work_bytes(ns, ns - 1))
        awork = Guarded(gpu.Context.ackwalk_work_bytes(ns, ns - 1))
        place, rstop, ack, astop = Guarded(16 * ns), Guarded(4 * ns), Guarded(16 * ns), Guarded(4 * ns)
        # the second batch: every stream again, enough to pass the chunk's end, so SBPut compacts
        b2 = sc.Batch(b.snd, b.dtx, b.payload, b.chunks)
        b2.requests(np.arange(ns)[::-1].copy(), rng.integers(3200, 3500, size=ns), rng=rng)
        s2 = Send(gpu, b2, 21, snd=s1.c.snd, dtx=s1.c.dtx, payload=s1.c.payload)
        s2.tx, s2.d_state, s2.state = s1.tx, s1.d_state, state_a
        snap = [Guarded(s1.c.snd.nbytes), Guarded(s1.c.dtx.nbytes), Guarded(s1.c.payload.nbytes)]
        sweep = Guarded(16 * ns), Guarded(4 * ns), Guarded(4 * ns + 4), Guarded(4 * ns), Guarded(4), Guarded(16)
        swork = Guarded(gpu.Context.rto_sweep_work_bytes(ns - 1, ns))
        s3 = Send(gpu, b2, 21, snd=s1.c.snd, dtx=s1.c.dtx, payload=s1.c.payload)
        s3.tx, s3.d_state, s3.state = s1.tx, s1.d_state, state_a

        tab.update_dev(None, 0, d_ent, len(ent), stream=st)
        s1.run(cx, cur1, st)
        gt = tuple(x.t for x in grp)
        cx.rx_chunk_dev(d_abuf, d_adesc, ns, 0, d_res, stream=st)
        cx.rx_tcpopt_chunk_dev(d_abuf, d_adesc, ns, 0, d_res, d_opt, stream=st)
        tab.lookup_dev(d_res, ns, d_sid.t, None, stream=st)
        cx.group_dev(d_sid.t, ns, ns - 1, *gt, gwork.t, stream=st)
        cx.rcvwalk_dev(d_res, d_opt, ns, ns - 1, *gt, s1.d_state, place.t, rstop.t, rwork.t, stream=st)
        cx.ackwalk_dev(d_res, d_opt, place.t, ns, ns - 1, *gt, cur_ack, s1.c.snd.t, ack.t, astop.t, awork.t, stream=st)
        with torch.cuda.stream(st):
            for g_, t_ in zip(snap, (s1.c.snd.t, s1.c.dtx.t, s1.c.payload.t)):
                g_.t.copy_(t_)
        s2.run(cx, cur2, st)
        with torch.cuda.stream(st):
            snap2 = [t_.clone() for t_ in (s1.c.snd.t, s1.c.dtx.t, s1.c.payload.t, s1.tx.t)]
        cx.rto_send_dev(ns - 1, s1.c.snd.t, s1.c.dtx.t, cur3, ns, *(x.t for x in sweep), swork.t, s3.idx, s3.d_state,
                        s1.tx.t, s1.c.payload.t, s3.d_links, s3.image.t, 0, 0, rs.SLOT, s3.seg.t, s3.desc.t, s3.seg_cap,
                        s3.dres.t, s3.dtotal.t, s3.status.t, s3.work.t, stream=st)
        cx.rx_chunk_dev(s3.image.t, s3.desc.t, s3.seg_cap, 0, s3.r2, stream=st)
        st.synchronize()

        # 1. the first write and its frames; 2. the records behind the ACK walk
        assert (w1[0]["verdict"] == sm.WRITTEN).all()
        assert ack.numpy().tobytes() == ack_want.tobytes() and s1.d_state.cpu().numpy().tobytes() == state_a.tobytes()
        assert snap[0].numpy().tobytes() == snd1a.tobytes()
        assert snap[1].numpy().tobytes() == dtx1.tobytes() and snap[2].numpy().tobytes() == pay1.tobytes()
        for g_, e in ((s1.c.wres.numpy(SNDWRITE_RES_DTYPE), w1[0]), (s1.seg.numpy(TX_SEG_DTYPE), dg1[0]),
                      (s1.dres.numpy(DATAGEN_RES_DTYPE), dg1[2])):
            assert g_.tobytes() == e.tobytes()
        image1, _ = xm.build_frames(dg1[0], pay1, LINKS.view(xm.LINK_DTYPE), dg1[1], np.zeros(s1.image.nbytes, np.uint8))
        assert s1.image.numpy().tobytes() == image1.tobytes()
        res1 = s1.r2.cpu().numpy().view(RESULT_DTYPE)
        for i in range(ns):
            got, seq0 = frames_bytes(res1, image1, dg1[1], dg1[2][i])
            off = b.chunks[i][0]
            start, ln = b.ranges[i]
            assert got == b.payload[off:off + held[i]].tobytes() + b.src[start:start + ln].tobytes(), i
            assert seq0 == int(b.snd["snd_nxt"][i])
        # 2. + 3. the second write on the acknowledged records: it compacts, and its frames carry only its bytes
        w2, dg2, pay2 = s2.expect(snd1a, dtx1, pay1, tx1, cur2)
        assert (w2[0]["verdict"] == sm.WRITTEN).all() and (w2[0]["flags"] & SNDWRITE_COMPACTED).all()
        snd2, tx2, dtx2 = dg2[4], dg2[5], dg2[6]
        for got, want, name in zip(snap2, (snd2, dtx2, pay2, tx2), ("snd", "dtx", "payload", "tx")):
            assert got.cpu().numpy().tobytes() == want.tobytes(), name
        for g_, e in ((s2.seg.numpy(TX_SEG_DTYPE), dg2[0]), (s2.desc.numpy(DESC_DTYPE), dg2[1]),
                      (s2.dres.numpy(DATAGEN_RES_DTYPE), dg2[2]), (s2.c.wres.numpy(SNDWRITE_RES_DTYPE), w2[0])):
            assert g_.tobytes() == e.tobytes()
        image2, _ = xm.build_frames(dg2[0], pay2, LINKS.view(xm.LINK_DTYPE), dg2[1], np.zeros(s2.image.nbytes, np.uint8))
        assert s2.image.numpy().tobytes() == image2.tobytes()
        res2 = s2.r2.cpu().numpy().view(RESULT_DTYPE)
        for j in range(ns):
            sid = int(b2.wreq["sid"][j])
            got, seq0 = frames_bytes(res2, image2, dg2[1], dg2[2][j])
            start, _ = b2.ranges[j]
            assert got == b2.src[start:start + int(w2[0]["written"][j])].tobytes() and seq0 == int(snd1["snd_nxt"][sid])
        # 4. the sweep: every stream is due, and retransmits one segment from snd_una out of the compacted chunk
        sw, dg3 = rs.send(snd2, dtx2, cur3, ns, s3.state, tx2, len(pay2), s3.seg_cap)
        assert (sw[2]["verdict"] == rs.RETRANSMIT).all() and len(sw[2]) == ns
        assert s1.c.snd.numpy().tobytes() == dg3[4].tobytes() and s1.c.dtx.numpy().tobytes() == dg3[6].tobytes()
        assert s3.seg.numpy(TX_SEG_DTYPE).tobytes() == dg3[0].tobytes()
        image3, _ = xm.build_frames(dg3[0], pay2, LINKS.view(xm.LINK_DTYPE), dg3[1], np.zeros(s3.image.nbytes, np.uint8))
        assert s3.image.numpy().tobytes() == image3.tobytes()
        res3 = s3.r2.cpu().numpy().view(RESULT_DTYPE)
        sent = [bytes(b.payload[b.chunks[i][0]:][:held[i]]) + bytes(b.src[b.ranges[i][0]:][:b.ranges[i][1]]) for i in range(ns)]
        for j in range(ns):
            sid = int(b2.wreq["sid"][j])
            sent[sid] += bytes(b2.src[b2.ranges[j][0]:][:int(w2[0]["written"][j])])
        for j, r in enumerate(sw[2]):
            sid = int(r["sid"])
            got, seq0 = frames_bytes(res3, image3, dg3[1], dg3[2][j])
            assert seq0 == int(snd2["snd_una"][sid]) and len(got) > 0
            assert got == sent[sid][int(k[sid]):][:len(got)], sid
        for g_ in (*snap, *sweep, swork, s1.c.snd, s1.c.dtx, s1.c.payload, s1.tx, s3.image, s3.seg, d_sid, *grp, gwork, rwork,
                   awork, place, rstop, ack, astop):
            assert g_.guard_intact()


def test_write_send_dev_against_the_chained_models(gpu, ctx):
    """One write_send_dev call with every verdict among its requests: every byte
    of both calls' outputs, and the built frames parse as TCP_OK."""
    rng = np.random.default_rng(13)
    b = sc.random_batch(rng, 40, 90, sizes=(256, 1024, 5000), dup=0.2)
    b.snd["cwnd"], b.snd["peer_wnd"], b.snd["rto"] = 1 << 20, rng.choice([0, 500, 1 << 20], len(b.snd)), 200
    s = Send(gpu, b, 22)
    s.run(ctx, 777)
    torch.cuda.synchronize()
    w, dg, payload = s.expect(b.snd, b.dtx, b.payload, s.tx0, 777)
    s.check(w, dg, payload, "write_send")
    assert (w[0]["verdict"] == sm.WRITTEN).sum() > 10 and {dm.SENT, dm.WINDOW, dm.NONE} <= set(dg[2]["status"].tolist())


def test_the_captured_write_send_set_replayed_twice(gpu):
    rng = np.random.default_rng(14)
    ns = 32
    b = chain_batch(rng, ns)
    b.requests(rng.permutation(ns), rng.integers(1, 5000, size=ns), rng=rng)
    with gpu.Context(0) as cx:
        st = torch.cuda.Stream(device=DEV)
        s = Send(gpu, b, 23)
        s.run(cx, 4242, st)                                       # kernels loaded before the capture
        st.synchronize()
        w, dg, payload = s.expect(b.snd, b.dtx, b.payload, s.tx0, 4242)
        s.check(w, dg, payload, "before the capture")
        assert (w[0]["flags"] & SNDWRITE_COMPACTED).any() and not (w[0]["flags"] & SNDWRITE_COMPACTED).all()

        def reset():
            s.c.snd.t.copy_(to_dev(b.snd)), s.c.dtx.t.copy_(to_dev(b.dtx)), s.c.payload.t.copy_(to_dev(b.payload))
            s.tx.t.copy_(to_dev(s.tx0))
            for x in (s.c.wres, s.c.seg_sid, s.c.seg_start, s.c.seg_stop, s.c.nseg, s.c.total, s.seg, s.desc, s.dres,
                      s.dtotal, s.status):
                x.t.fill_(SENT)
            s.c.work.t.fill_(0x3C), s.work.t.fill_(0x3C), s.image.t.zero_(), s.r2.zero_()
            torch.cuda.synchronize()

        reset()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            s.run(cx, 4242, st)
        for k in range(2):
            reset()
            graph.replay()
            torch.cuda.synchronize()
            s.check(w, dg, payload, f"replay {k}")
        del graph


# ---- the host form -----------------------------------------------------------------------------------------
def host_batch(rng, n_streams, n_req):
    """A random batch whose lengths the host form can pack: a len above 2^31 - 1
    alone would pass MTCP_GPU_SNDWRITE_HOST_MAX_BYTES (EINVAL), so such a
    request is refused by a flag bit instead."""
    b = sc.random_batch(rng, n_streams, n_req, dup=0.2)
    big = b.wreq["len"] > 1 << 20
    b.wreq["len"][big], b.wreq["flags"][big] = 7, 1
    return b


class HostCall:
    def __init__(self, b):
        self.b = b
        self.snd, self.dtx, self.payload = to_dev(b.snd), to_dev(b.dtx), to_dev(b.payload)

    def reset(self):
        self.snd.copy_(to_dev(self.b.snd)), self.dtx.copy_(to_dev(self.b.dtx)), self.payload.copy_(to_dev(self.b.payload))

    def call(self, L, h, wreq=None, n=None):
        b = self.b
        wreq = b.wreq if wreq is None else wreq
        n = len(wreq) if n is None else n
        k = max(len(wreq), 1)
        fill = lambda nbytes, dt: np.full(nbytes, SENT, np.uint8).view(dt)
        outs = (fill(16 * k, SNDWRITE_RES_DTYPE), fill(4 * k, np.uint32), fill(4 * k + 4, np.uint32), fill(4 * k, np.uint32),
                fill(4, np.uint32), fill(16, np.uint64))
        src = np.ascontiguousarray(b.src)
        rc_ = L.mtcp_gpu_sndwrite(h, wreq.ctypes.data, n, b.max_id, self.snd.data_ptr(), self.dtx.data_ptr(),
                                  src.ctypes.data, len(src), self.payload.data_ptr(), len(b.payload),
                                  *(o.ctypes.data for o in outs))
        return (rc_,) + outs

    def check(self, got, want):
        assert got[0] == 0
        for g, w in zip(got[1:], want[3:]):
            assert g.tobytes() == w.tobytes()
        torch.cuda.synchronize()
        assert self.snd.cpu().numpy().tobytes() == want[0].tobytes() and self.dtx.cpu().numpy().tobytes() == want[1].tobytes()
        assert self.payload.cpu().numpy().tobytes() == want[2].tobytes()

    def untouched(self):
        b = self.b
        return (self.snd.cpu().numpy().tobytes() == b.snd.tobytes() and self.dtx.cpu().numpy().tobytes() == b.dtx.tobytes()
                and self.payload.cpu().numpy().tobytes() == b.payload.tobytes())


def test_the_host_form_unbounded_bounded_and_behind_a_stalled_gpu(gpu):
    """The stalled-GPU pattern of tests/test_gpu_bounded.py (its helpers, its
    stall and limit values): ETIMEDOUT within the limit, nothing of the
    caller's written right after the call nor after the stall has ended, the
    context answers EIO, a fresh context gives the model's answers."""
    from mtcp_amd._lib import lib
    from tests.test_gpu_bounded import LIMIT_US, SLACK_S, STALL_US, stall_lib, stream_busy, stream_wait
    L, S = lib(), stall_lib()
    rng = np.random.default_rng(15)
    b = host_batch(rng, 40, 150)
    want = b.expect()
    assert (want[3]["verdict"] == sm.WRITTEN).sum() > 10 and (want[3]["verdict"] == sm.DUP).any()
    assert (want[3]["verdict"] == sm.BAD_REQ).any()
    hc = HostCall(b)
    c = gpu.Context(0)
    handle = c.stream
    hc.check(hc.call(L, c._h), want)                        # unbounded: stage sized, kernels loaded
    c.wait_limit = LIMIT_US
    hc.reset()
    hc.check(hc.call(L, c._h), want)                        # bounded, no stall: the bounce buffers sized
    hc.reset()
    assert S.mtcp_gpu_debug_stall(c._h, STALL_US) == 0
    t0 = time.monotonic()
    got = hc.call(L, c._h)
    dt = time.monotonic() - t0
    assert got[0] == ETIMEDOUT, got[0]
    assert dt < LIMIT_US / 1e6 + SLACK_S, dt
    assert stream_busy(handle)
    untouched = lambda: all((o.view(np.uint8) == SENT).all() for o in got[1:])
    assert untouched()
    assert L.mtcp_gpu_sync(c._h) == EIO
    assert hc.call(L, c._h)[0] == EIO
    own = torch.cuda.Stream(device=DEV)
    dc = Call(gpu, b)
    assert L.mtcp_gpu_sndwrite_dev(c._h, dc.wreq.data_ptr(), dc.n, b.max_id, dc.snd.t.data_ptr(), dc.dtx.t.data_ptr(),
                                   dc.src.data_ptr(), len(b.src), dc.payload.t.data_ptr(), len(b.payload),
                                   *(t.data_ptr() for t in dc.outs()), dc.wb, own.cuda_stream) == EIO
    c.close()
    stream_wait(handle)                                     # the stall and what was queued behind it end
    own.synchronize()
    assert untouched()
    assert (dc.wres.all == SENT).all().item() and dc.payload.numpy().tobytes() == b.payload.tobytes()
    with gpu.Context(0) as fresh:
        fresh.wait_limit = 5_000_000
        hc.reset()
        hc.check(hc.call(L, fresh._h), want)
        # the wrapper, an empty batch, and bytes above one stage
        hc.reset()
        outs = fresh.sndwrite(b.wreq, b.max_id, hc.snd, hc.dtx, b.src, hc.payload)
        for g, w in zip(outs, want[3:]):
            assert g.tobytes() == w.tobytes()
        hc.reset()
        empty = hc.call(L, fresh._h, n=0)
        assert empty[0] == 0 and all((o.view(np.uint8) == SENT).all() for o in empty[1:]) and hc.untouched()
        big = b.wreq.copy()
        big["len"] = (32 << 20) // len(big) + 16
        assert hc.call(L, fresh._h, wreq=big)[0] == EINVAL and hc.untouched()


# ---- error returns -------------------------------------------------------------------------------------------
def test_error_returns(gpu):
    """MTCP_GPU_EINVAL for each misuse the header lists, for every pointer of
    the three entry points; a refused call launches nothing and writes nothing."""
    from mtcp_amd._lib import lib
    L = lib()
    rng = np.random.default_rng(16)
    b = host_batch(rng, 20, 40)
    s = Send(gpu, b, 24)
    c = s.c
    align = {"wreq": 16, "snd": 128, "dtx": 16, "src": 16, "payload": 16, "wres": 16, "seg_sid": 4, "seg_start": 4,
             "seg_stop": 4, "nseg": 4, "total": 8, "work": 16}
    tens = {"wreq": c.wreq, "snd": c.snd.t, "dtx": c.dtx.t, "src": c.src, "payload": c.payload.t, "wres": c.wres.t,
            "seg_sid": c.seg_sid.t, "seg_start": c.seg_start.t, "seg_stop": c.seg_stop.t, "nseg": c.nseg.t,
            "total": c.total.t, "work": c.work.t}
    send_tens = {"idx": s.idx, "state": s.d_state, "tx": s.tx.t, "links": s.d_links, "buf": s.image.t, "seg": s.seg.t,
                 "desc": s.desc.t, "dres": s.dres.t, "dtotal": s.dtotal.t, "status": s.status.t, "dwork": s.work.t}
    send_align = {"idx": 4, "state": 64, "tx": 32, "links": 4, "seg": 8, "desc": 8, "dres": 16, "dtotal": 8, "dwork": 16}

    def ptrs(kw):
        p = {k: t.data_ptr() for k, t in {**tens, **send_tens}.items()}
        p.update(kw)
        return p

    def call(h, n=c.n, max_id=b.max_id, src_bytes=len(b.src), payload_bytes=len(b.payload), wb=c.wb, **kw):
        p = ptrs(kw)
        return L.mtcp_gpu_sndwrite_dev(h, p["wreq"], n, max_id, p["snd"], p["dtx"], p["src"], src_bytes, p["payload"],
                                       payload_bytes, p["wres"], p["seg_sid"], p["seg_start"], p["seg_stop"], p["nseg"],
                                       p["total"], p["work"], wb, None)

    def send(h, n=c.n, max_id=b.max_id, src_bytes=len(b.src), wb=c.wb, dwb=s.work.nbytes, seg_cap=s.seg_cap, n_links=3,
             slot=rs.SLOT, **kw):
        p = ptrs(kw)
        return L.mtcp_gpu_write_send_dev(h, p["wreq"], n, max_id, p["snd"], p["dtx"], p["src"], src_bytes, p["payload"],
                                         len(b.payload), p["wres"], p["seg_sid"], p["seg_start"], p["seg_stop"], p["nseg"],
                                         p["total"], p["work"], wb, p["idx"], p["state"], p["tx"], 1, p["links"], n_links,
                                         p["buf"], 0, s.image.nbytes, 0, slot, 0, 0, p["seg"], p["desc"], seg_cap,
                                         p["dres"], p["dtotal"], p["status"], p["dwork"], dwb, None)

    def misaligned(t, a):
        big = torch.zeros(t.numel() + 256, dtype=torch.uint8, device=DEV)
        return big, big.data_ptr() + (-big.data_ptr()) % 128 + a // 2

    with gpu.Context(0) as cx:
        before = c.raw()
        assert call(None) == EINVAL and send(None) == EINVAL
        for name in tens:
            assert call(cx._h, **{name: None}) == EINVAL, name
            assert send(cx._h, **{name: None}) == EINVAL, name
            keep, p = misaligned(tens[name], align[name])
            assert call(cx._h, **{name: p}) == EINVAL, name
            assert send(cx._h, **{name: p}) == EINVAL, name
        for name in send_tens:
            assert send(cx._h, **{name: None}) == EINVAL, name
            if name in send_align:
                keep, p = misaligned(send_tens[name], send_align[name])
                assert send(cx._h, **{name: p}) == EINVAL, name
        assert call(cx._h, wb=c.wb - 16) == EINVAL and send(cx._h, wb=c.wb - 16) == EINVAL
        assert send(cx._h, dwb=s.work.nbytes - 16) == EINVAL and send(cx._h, seg_cap=0) == EINVAL
        assert send(cx._h, n_links=0) == EINVAL and send(cx._h, slot=66) == EINVAL
        assert call(cx._h, src_bytes=len(b.src) - 8) == EINVAL and call(cx._h, payload_bytes=len(b.payload) - 8) == EINVAL
        assert call(cx._h, n=(1 << 26) + 1) == EINVAL and send(cx._h, n=(1 << 24) + 1) == EINVAL
        assert call(cx._h, max_id=gm.MAX_ID + 1) == EINVAL and send(cx._h, max_id=gm.MAX_ID + 1) == EINVAL
        assert call(cx._h, n=0, wb=0, **{k: None for k in tens}) == 0       # n == 0: OK without a launch
        torch.cuda.synchronize()
        for x, y in zip(before, c.raw()):
            assert x.tobytes() == y.tobytes()
        assert (s.seg.numpy() == SENT).all() and (s.dres.numpy() == SENT).all()
        hc = HostCall(b)
        outs = hc.call(L, cx._h, n=0)[1:]
        src = np.ascontiguousarray(b.src)
        host = lambda **kw: L.mtcp_gpu_sndwrite(*[kw.get(k, v) for k, v in (
            ("h", cx._h), ("wreq", b.wreq.ctypes.data), ("n", c.n), ("max_id", b.max_id), ("snd", hc.snd.data_ptr()),
            ("dtx", hc.dtx.data_ptr()), ("src", src.ctypes.data), ("src_bytes", len(src)),
            ("payload", hc.payload.data_ptr()), ("payload_bytes", len(b.payload)), ("wres", outs[0].ctypes.data),
            ("seg_sid", outs[1].ctypes.data), ("seg_start", outs[2].ctypes.data), ("seg_stop", outs[3].ctypes.data),
            ("nseg", outs[4].ctypes.data), ("total", outs[5].ctypes.data))])
        for k in ("h", "wreq", "snd", "dtx", "src", "payload", "wres", "seg_sid", "seg_start", "seg_stop", "nseg", "total"):
            assert host(**{k: None}) == EINVAL, k
        assert host(payload_bytes=len(b.payload) - 1) == EINVAL and host(max_id=gm.MAX_ID + 1) == EINVAL
        assert host(snd=hc.snd.data_ptr() + 64) == EINVAL and host(dtx=hc.dtx.data_ptr() + 8) == EINVAL
        assert all((o.view(np.uint8) == SENT).all() for o in outs) and hc.untouched()
        assert host() == 0
