"""The batched application read on the GPU (include/mtcp_gpu_rcvread.h,
mtcp_amd/csrc/rcvread_kernels.hpp): every byte of d_dst, d_rres, d_state, d_rbuf,
d_tx (byte 19 among them) and d_total of every case is compared with
tests/rcvread_model.py; none is sampled.

Every destination range has 64 B guard bands (tests/rcvread_cases.py), the
outputs have guards behind them, the workspace is exactly sized and holds 0xA5.
Every source alignment x destination alignment x length 1-48; the lengths around
one and two copy units; a 1 MiB run beside 1-byte runs; request counts around
the wave and the plan workgroup (the read has no one-launch form: the workgroup
is the only count at which a path changes); every verdict; duplicates; all
EAGAIN; all PEEK; the reference-written fixture read by read; random bytes in
every record array; d_tx and d_snd NULL; four workspace fills; the chain rx +
lookup + group + walk + copy + read over two batches with no host refresh; a
captured walk + copy + read replayed twice; the host form unbounded, bounded and
behind a stalled GPU; every error return."""
import ctypes
import time

import numpy as np
import pytest

import oracle
from mtcp_amd._types import (ACKGEN_STATE_DTYPE, RCV_BUF_DTYPE, RCV_PLACE_DTYPE, RCV_STATE_DTYPE, RCVREAD_ON_ACKQ,
                             RCVREAD_PEEK, RCVREAD_REQ_DTYPE, RCVREAD_RES_DTYPE)
from tests import flowtab_model as fm
from tests import group_model as gm
from tests import rcvread_cases as rc
from tests import rcvread_model as rm
from tests import tcpopt_model as tm

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EINVAL, EIO, ETIMEDOUT = -22, -5, -110
GUARD = 4096
SENT = 0xA5
UNIT = rm.UNIT
WG = 256                                               # rcvread_kernels.hpp: requests per plan workgroup


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")
    from mtcp_amd import gpu as g
    assert g.Context.rcvread_tile() == UNIT
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
    """The device arrays of one call on a rcvread_cases.Batch, the outputs guarded."""
    OUT = ("state", "rbuf", "tx", "dst", "rres", "total", "work")

    def __init__(self, gpu, b, work_fill=SENT):
        self.b, self.n = b, len(b.req)
        self.req = to_dev(b.req) if self.n else torch.zeros(32, dtype=torch.uint8, device=DEV)
        self.state, self.rbuf = Guarded(b.state.nbytes, b.state), Guarded(b.rbuf.nbytes, b.rbuf)
        self.tx = None if b.tx is None else Guarded(b.tx.nbytes, b.tx)
        self.snd = None if b.snd is None else to_dev(b.snd)
        self.arena, self.dst = to_dev(b.arena), Guarded(len(b.dst), b.dst)
        self.rres, self.total = Guarded(16 * max(self.n, 1)), Guarded(16)
        self.wb = gpu.Context.rcvread_work_bytes(self.n, b.max_id)
        assert self.wb > 0
        self.work = Guarded(self.wb, work_fill)

    def args(self):
        return (self.req, self.n, self.b.max_id, self.state.t, self.rbuf.t, None if self.tx is None else self.tx.t,
                self.snd, self.arena, self.dst.t, self.rres.t, self.total.t, self.work.t)

    def run(self, ctx, stream=None):
        ctx.rcvread_dev(*self.args(), stream=stream)

    def raw(self):
        return (self.state.numpy().copy(), self.rbuf.numpy().copy(), None if self.tx is None else self.tx.numpy().copy(),
                self.dst.numpy().copy(), self.rres.numpy()[:16 * self.n].copy(), self.total.numpy().copy())

    def check(self, want=None, what=""):
        b = self.b
        want = b.expect() if want is None else want
        for name in self.OUT:
            g = getattr(self, name)
            assert g is None or g.guard_intact(), f"{what}: bytes behind {name} were written"
        state, rbuf, tx, dst, rres, total = self.raw()
        w_state, w_rbuf, w_tx, w_dst, w_rres, w_total = want
        got_r, bad = rres.view(RCVREAD_RES_DTYPE), []
        if rres.tobytes() != w_rres.tobytes():
            bad = np.nonzero(got_r != w_rres)[0]
        assert len(bad) == 0, f"{what}: {len(bad)} of {self.n} results differ, first {bad[0]}: {got_r[bad[0]]} want " \
                              f"{w_rres[bad[0]]} for {b.req[bad[0]]}"
        bad = np.nonzero(dst != w_dst)[0]
        assert len(bad) == 0, f"{what}: {len(bad)} destination bytes differ, first at {bad[0]}: {dst[bad[0]]} want " \
                              f"{w_dst[bad[0]]} (ranges at {b.req['dst_off'][:6].tolist()}...)"
        for name, g, w, dt in (("state", state, w_state, RCV_STATE_DTYPE), ("rbuf", rbuf, w_rbuf, RCV_BUF_DTYPE),
                               ("tx", tx, w_tx, ACKGEN_STATE_DTYPE)):
            if w is None:
                continue
            if g.tobytes() != w.tobytes():
                k = np.nonzero(g.view(dt) != w)[0][0]
                raise AssertionError(f"{what}: {name} of stream {k}: {g.view(dt)[k]} want {w[k]}")
        assert total.view(np.uint64).tolist() == w_total.tolist(), f"{what}: totals"
        assert self.arena.cpu().numpy().tobytes() == b.arena.tobytes(), f"{what}: the arena was written"
        if self.snd is not None:
            assert self.snd.cpu().numpy().tobytes() == b.snd.tobytes(), f"{what}: d_snd was written"
        return want


def run(gpu, ctx, b, what="", work_fill=SENT):
    c = Call(gpu, b, work_fill)
    c.run(ctx)
    torch.cuda.synchronize()
    c.check(what=what)
    return c


# ---- alignment and length ---------------------------------------------------------------------------------
def test_every_alignment_and_short_length(gpu, ctx):
    """16 source x 16 destination alignments x lengths 1-48, one stream each;
    len is 0-2 above or below the merged bytes."""
    rng = np.random.default_rng(1)
    sa, da, ln = (a.reshape(-1) for a in np.meshgrid(np.arange(16), np.arange(16), np.arange(1, 49), indexing="ij"))
    n = len(ln)
    heads = rng.integers(0, 8, size=n)
    b = rc.direct(rng, np.full(n, 64), ln, heads, src_align=sa)
    assert ((b.rbuf["data_off"] + b.rbuf["head_offset"]) % 16 == sa).all()
    lens = np.where(rng.integers(3, size=n) == 0, np.maximum(ln - rng.integers(0, 3, size=n), 1), ln + rng.integers(0, 3, size=n))
    b.requests(np.arange(n), lens, dst_align=da)
    assert (b.req["dst_off"] % 16 == da).all()
    c = run(gpu, ctx, b, "alignments")
    rres = c.raw()[4].view(RCVREAD_RES_DTYPE)
    assert (rres["verdict"] == rm.READ).all() and int(c.raw()[5].view(np.uint64)[0]) == n


def test_lengths_around_one_and_two_units(gpu, ctx):
    """copylen at the unit - 1, the unit, the unit + 1 and the same around two
    units, at destination phases 0, 1, 9 and 15 and source phases 0 and 7: the
    request's last unit holds 1 piece, 255, 256 or one byte of a 257th."""
    rng = np.random.default_rng(2)
    cases = [(ln, da, sa) for ln in (UNIT - 17, UNIT - 1, UNIT, UNIT + 1, 2 * UNIT - 16, 2 * UNIT - 1, 2 * UNIT, 2 * UNIT + 1)
             for da in (0, 1, 9, 15) for sa in (0, 7)]
    ln, da, sa = (np.array(x) for x in zip(*cases))
    b = rc.direct(rng, np.full(len(ln), 3 * UNIT), ln, rng.integers(0, 100, size=len(ln)), src_align=sa)
    b.requests(np.arange(len(ln)), np.full(len(ln), 3 * UNIT), dst_align=da)
    run(gpu, ctx, b, "units")
    want_units = [rm.units(int(q["dst_off"]), int(l)) for q, l in zip(b.req, ln)]
    assert {1, 2, 3} <= set(want_units)


def test_one_megabyte_run_beside_one_byte_runs(gpu, ctx):
    rng = np.random.default_rng(3)
    n = 65
    sizes, merged = np.full(n, 64), np.ones(n, dtype=np.int64)
    sizes[32], merged[32] = 1 << 20, (1 << 20) - 5
    b = rc.direct(rng, sizes, merged, np.where(np.arange(n) == 32, 5, rng.integers(0, 60, size=n)))
    b.requests(np.arange(n), np.full(n, 1 << 20), dst_align=rng.integers(16, size=n), room=merged)
    c = run(gpu, ctx, b, "1 MiB")
    assert c.raw()[5].view(np.uint64).tolist() == [n, (1 << 20) - 5 + 64]


@pytest.mark.parametrize("n", [1, 63, 64, 65, WG - 1, WG, WG + 1, 3 * WG + 7])
def test_request_counts_around_the_wave_and_the_workgroup(gpu, ctx, n):
    rng = np.random.default_rng(100 + n)
    b = rc.random_batch(rng, max(n // 2, 1), n, sizes=(64, 256), dup=0.1)
    run(gpu, ctx, b, f"n={n}")


# ---- the verdict chain ---------------------------------------------------------------------------------
def test_every_verdict_and_flag(gpu, ctx):
    rng = np.random.default_rng(4)
    verdicts, flags = set(), set()
    for trial in range(6):
        b = rc.random_batch(rng, 40, 120, dup=0.25)
        want = run(gpu, ctx, b, f"verdicts {trial}").b.expect()
        verdicts |= set(want[4]["verdict"].tolist())
        flags |= set(want[4]["flags"].tolist())
    assert verdicts == set(range(1, 8)) and {1, 2, 4} <= {f & m for f in flags for m in (1, 2, 4)}


def test_bad_requests(gpu, ctx):
    """sid above max_id, each reserved word, an unknown flag, and the range
    test with len and size: refused whatever merged_len is, accepted at the
    exact fit."""
    rng = np.random.default_rng(5)
    b = rc.direct(rng, np.full(12, 256), [0, 100] * 6, np.zeros(12, dtype=np.int64))
    b.requests(np.arange(12), [10, 10, 10, 10, 10, 10, 10, 10, 300, 300, 200, 200])
    b.req["sid"][0] = 12
    b.req["rsvd"][1, 0], b.req["rsvd"][2, 1], b.req["rsvd"][3, 2] = 1, 1 << 31, 7
    b.req["flags"][4], b.req["flags"][5] = 4, 1 << 31
    end = len(b.dst)
    b.req["dst_off"][6], b.req["dst_off"][7] = end - 9, end - 9          # len 10 does not fit, merged 0 or 100
    b.req["dst_off"][8], b.req["dst_off"][9] = end - 255, end - 256      # MIN(300, 256): one short, exact
    b.req["dst_off"][10], b.req["dst_off"][11] = end + 1, (1 << 64) - 100
    want = run(gpu, ctx, b, "bad requests").b.expect()
    assert want[4]["verdict"].tolist() == [rm.BAD_REQ] * 9 + [rm.READ, rm.BAD_REQ, rm.BAD_REQ]


@pytest.mark.parametrize("where", ["0/1", "0/n-1", "three"])
def test_duplicates(gpu, ctx, where):
    rng = np.random.default_rng(6)
    n = 70
    b = rc.direct(rng, np.full(n, 128), rng.integers(1, 128, size=n), np.zeros(n, dtype=np.int64))
    sids = np.arange(n)
    lens = rng.integers(1, 200, size=n)
    if where == "0/1":
        sids[1] = sids[0]
    elif where == "0/n-1":
        sids[n - 1] = sids[0]
    else:
        sids[40], sids[69] = sids[5], sids[5]
    b.requests(sids, lens, dst_align=rng.integers(16, size=n))
    want = run(gpu, ctx, b, where).b.expect()
    dup = np.nonzero(want[4]["verdict"] == rm.DUP)[0].tolist()
    assert dup == {"0/1": [1], "0/n-1": [n - 1], "three": [40, 69]}[where]


def test_all_eagain_and_all_peek(gpu, ctx):
    rng = np.random.default_rng(7)
    n = 100
    b = rc.direct(rng, np.full(n, 128), np.zeros(n, dtype=np.int64), rng.integers(0, 128, size=n))
    b.requests(np.arange(n), rng.integers(0, 200, size=n))
    c = run(gpu, ctx, b, "all EAGAIN")
    assert (c.raw()[4].view(RCVREAD_RES_DTYPE)["verdict"] == rm.EAGAIN).all() and c.raw()[5].view(np.uint64).tolist() == [0, 0]
    assert (c.raw()[3] == 0x5A).all()
    b = rc.direct(rng, np.full(n, 128), rng.integers(1, 100, size=n), rng.integers(0, 28, size=n))
    b.requests(np.arange(n), rng.integers(1, 200, size=n), np.full(n, RCVREAD_PEEK), dst_align=rng.integers(16, size=n))
    c = run(gpu, ctx, b, "all PEEK")
    state, rbuf, tx = c.raw()[:3]
    assert (c.raw()[4].view(RCVREAD_RES_DTYPE)["verdict"] == rm.PEEKED).all()
    assert state.tobytes() == b.state.tobytes() and rbuf.tobytes() == b.rbuf.tobytes() and tx.tobytes() == b.tx.tobytes()


def test_without_tx_and_snd(gpu, ctx):
    rng = np.random.default_rng(8)
    b = rc.random_batch(rng, 30, 60, with_tx=False)
    want = run(gpu, ctx, b, "NULL tx").b.expect()
    assert not (want[4]["flags"] & 2).any() and (want[4]["verdict"] == rm.READ).any()


@pytest.mark.parametrize("garbage", [False, True])
def test_random_bytes_in_every_record_array(gpu, ctx, garbage):
    """With sane dst_off the accepted ranges are apart and every byte is the
    model's; with random dst_off too only the bounds hold: the guards behind
    every array and the bytes outside [0, dst_bytes) stay."""
    rng = np.random.default_rng(9)
    for trial in range(4):
        b = rc.random_records(rng, 64, 300, arena_bytes=1 << 15, dst_bytes=1 << 17)
        if not garbage:
            run(gpu, ctx, b, f"random records {trial}")
            continue
        b.req["dst_off"] = rng.integers(0, (1 << 17) + 64, size=len(b.req))
        c = Call(gpu, b)
        c.run(ctx)
        torch.cuda.synchronize()
        assert all(getattr(c, name) is None or getattr(c, name).guard_intact() for name in Call.OUT)
        want = b.expect()
        assert c.raw()[4].tobytes() == want[4].tobytes()            # the records do not depend on the overlap
        untouched = np.ones(len(b.dst), dtype=bool)
        for q, r in zip(b.req, want[4]):
            untouched[int(q["dst_off"]):int(q["dst_off"]) + int(r["copylen"])] = False
        assert (c.raw()[3][untouched] == 0x5A).all()


def test_four_workspace_fills_give_identical_bytes(gpu, ctx):
    rng = np.random.default_rng(10)
    b = rc.random_batch(rng, 50, 300, dup=0.3)
    outs = [run(gpu, ctx, b, f"fill {fill:#x}", work_fill=fill).raw() for fill in (0x00, 0xFF, SENT, 0x01)]
    for o in outs[1:]:
        for x, y in zip(outs[0], o):
            assert (x is None and y is None) or x.tobytes() == y.tobytes()


# ---- the fixture ------------------------------------------------------------------------------------------
def test_the_fixture_read_by_read(gpu, ctx):
    """Every case of tests/golden/rcvread_cases.bin is a stream; round k holds
    the k-th read or peek of every case as one batch, the puts in between
    replayed by the model on the host.  The GPU's bytes are the model's, and
    the returned length, the bytes and the offsets are the reference's."""
    cases = rm.load_fixture()
    apps = [rm.App(c["size"], c["init_seq"], c["eff_mss"]) for c in cases]
    pos, serial = [0] * len(cases), [0] * len(cases)
    rounds = checked = 0
    while True:
        evs = {}
        for ci, c in enumerate(cases):
            while pos[ci] < len(c["events"]) and c["events"][pos[ci]]["kind"] == "put":
                ev = c["events"][pos[ci]]
                apps[ci].put(ev["seq"], rm.payload_bytes(ci, serial[ci], ev["len"]))
                serial[ci] += 1
                pos[ci] += 1
            if pos[ci] < len(c["events"]) and len(apps[ci].st.frags) <= 4:
                evs[ci] = c["events"][pos[ci]]
                apps[ci].need_wnd_adv = evs[ci]["need_wnd_adv"]
                pos[ci] += 1
        if not evs:
            break
        rng = np.random.default_rng(rounds)
        b = rc.lay_out(apps, rng)
        ids = sorted(evs)
        b.requests(ids, [evs[ci]["len"] for ci in ids],
                   [(RCVREAD_PEEK if evs[ci]["kind"] == "peek" else 0) | (RCVREAD_ON_ACKQ if evs[ci]["on_ackq"] else 0)
                    for ci in ids], dst_align=rng.integers(16, size=len(ids)))
        c = run(gpu, ctx, b, f"fixture round {rounds}")
        state, rbuf, tx, dst, rres, total = c.raw()
        rres, rbuf = rres.view(RCVREAD_RES_DTYPE), rbuf.view(RCV_BUF_DTYPE)
        for k, ci in enumerate(ids):
            ev, at = evs[ci], int(b.req["dst_off"][k])
            assert int(rres["copylen"][k]) == max(ev["ret"], 0), (rounds, ci)
            assert dst[at:at + max(ev["ret"], 0)].tobytes() == ev["bytes"], (rounds, ci)
            assert (int(rbuf["head_offset"][ci]), int(rbuf["tail_offset"][ci]), int(rbuf["last_len"][ci])) == ev["after"][:3]
            # the host's own replay of the read keeps the App in step with the reference
            (rm.PeekForUser if ev["kind"] == "peek" else rm.CopyToUser)(apps[ci], ev["len"])
            assert apps[ci].snapshot() == ev["after"]
            checked += 1
        rounds += 1
    assert checked > 400 and rounds >= 10


# ---- the chain ---------------------------------------------------------------------------------------------
def chain_frames(tuples, seqs, payloads):
    """One frame per (stream, seq, payload): ACK only, no options."""
    frames = []
    for k, (c, seq, body) in enumerate(zip(tuples, seqs, payloads)):
        f = tm.frame_raw(5, 5, 0x10, body, seed=k)
        f[26:34], f[34:38] = c[:8], c[8:12]
        f[38:42] = int(seq).to_bytes(4, "big")
        frames.append(f)
    buf, desc = tm.pack_chunk(frames, slot=64)
    tm.fill_checksums(buf, desc)
    return buf, desc.astype(oracle.DESC_DTYPE)


class Chain:
    """rx + lookup + group + walk + copy + read on one stream for n frames."""

    def __init__(self, gpu, cx, tab, n, max_id, state, rbuf, arena, n_req, dst_bytes):
        self.gpu, self.cx, self.tab, self.n, self.max_id, self.n_req = gpu, cx, tab, n, max_id, n_req
        self.res = torch.zeros(n * 40, dtype=torch.uint8, device=DEV)
        self.sid = Guarded(4 * n)
        self.g = (Guarded(4 * n), Guarded(4 * n), Guarded(4 * n + 4), Guarded(4))
        self.gwork = Guarded(gpu.Context.group_work_bytes(n, max_id))
        self.wwork = Guarded(gpu.Context.rcvwalk_work_bytes(n, max_id))
        self.cwork = Guarded(gpu.Context.rcvcopy_work_bytes(n, max_id))
        self.rwork = Guarded(gpu.Context.rcvread_work_bytes(n_req, max_id))
        self.place, self.stop, self.cstat = Guarded(16 * n), Guarded(4 * n), Guarded(n)
        self.state, self.rbuf, self.arena = Guarded(state.nbytes, state), Guarded(rbuf.nbytes, rbuf), Guarded(len(arena), arena)
        self.dst, self.rres, self.total = Guarded(dst_bytes, 0x5A), Guarded(16 * n_req), Guarded(16)

    def walk_copy_read(self, d_buf, d_desc, d_req, st, with_rx=True):
        cx, g = self.cx, [x.t for x in self.g]
        if with_rx:
            cx.rx_chunk_dev(d_buf, d_desc, self.n, 0, self.res, stream=st)
            self.tab.lookup_dev(self.res, self.n, self.sid.t, None, stream=st)
            cx.group_dev(self.sid.t, self.n, self.max_id, *g, self.gwork.t, stream=st)
        cx.rcvwalk_dev(self.res, None, self.n, self.max_id, *g, self.state.t, self.place.t, self.stop.t, self.wwork.t,
                       stream=st)
        cx.rcvcopy_dev(d_buf, d_desc, 0, self.res, self.place.t, self.n, self.max_id, *g, self.stop.t, self.rbuf.t,
                       self.arena.t, self.cstat.t, self.cwork.t, stream=st)
        cx.rcvread_dev(d_req, self.n_req, self.max_id, self.state.t, self.rbuf.t, None, None, self.arena.t, self.dst.t,
                       self.rres.t, self.total.t, self.rwork.t, stream=st)


def chain_setup(rng, ns, size, per_batch, batches):
    tuples = [rng.integers(1, 255, 12, dtype=np.uint8).tobytes() for _ in range(ns)]
    irs = rng.integers(1 << 32, size=ns, dtype=np.uint64).astype(np.uint32)
    irs[0] = 0xFFFFFF00                               # stream 0 wraps inside the first batch
    state, rbuf = np.zeros(ns, RCV_STATE_DTYPE), np.zeros(ns, RCV_BUF_DTYPE)
    state["rcv_nxt"], state["head_seq"], state["rcv_wnd"], state["size"], state["tcp_state"] = irs, irs, size, size, 4
    offs = 64 + np.arange(ns) * (size + 64)
    rbuf["data_off"], rbuf["size"] = offs, size
    arena = np.full(int(offs[-1]) + size + 64, 0xEE, dtype=np.uint8)
    sent = [bytearray() for _ in range(ns)]
    chunks = []
    for _ in range(batches):
        who, seqs, bodies = [], [], []
        for k in range(per_batch):
            for s in range(ns):
                body = rng.integers(0, 256, int(rng.integers(1, 120)), dtype=np.uint8).tobytes()
                who.append(s), seqs.append((int(irs[s]) + len(sent[s])) & rm.M32), bodies.append(body)
                sent[s] += body
        # one segment in five swaps places with its successor of the same stream: out of order within the batch
        for i in range(0, len(who) - ns, 5):
            j = i + ns
            who[i], who[j], seqs[i], seqs[j], bodies[i], bodies[j] = who[j], who[i], seqs[j], seqs[i], bodies[j], bodies[i]
        chunks.append(chain_frames([tuples[s] for s in who], seqs, bodies))
    return tuples, state, rbuf, arena, sent, chunks


def test_frames_in_application_bytes_out_over_two_batches(gpu):
    """Two batches of frames through rx, lookup, group, walk, copy and read, the
    second behind the first on the stream with no host refresh and no wait in
    between: what the reads return is what the frames carried, in sequence
    order.  The first read takes a part of every stream, the second the rest."""
    rng = np.random.default_rng(11)
    ns, size, per_batch = 24, 2048, 6
    tuples, state, rbuf, arena, sent, chunks = chain_setup(rng, ns, size, per_batch, 2)
    n = ns * per_batch
    room = 2048
    with gpu.Context(0) as cx, gpu.FlowTable(cx, 10) as tab:
        st = torch.cuda.Stream(device=DEV)
        res0 = oracle.rx_chunk(chunks[0][0], chunks[0][1], 0, None)
        assert (res0["verdict"] == 0).all()
        ent = fm.entries(fm.record_keys(res0[:ns]), np.arange(ns, dtype=np.uint32))
        ch = Chain(gpu, cx, tab, n, ns - 1, state, rbuf, arena, ns, 2 * ns * room)
        reqs = []
        for k in range(2):
            rq = np.zeros(ns, RCVREAD_REQ_DTYPE)
            rq["sid"], rq["len"] = np.arange(ns), (rng.integers(1, 6, size=ns) if k == 0 else room)   # a batch brings 6 bytes or more
            rq["dst_off"] = (2 * np.arange(ns) + k) * room + (rng.integers(16, size=ns) if k == 0 else 0)
            reqs.append(rq)
        bufs = [(to_dev(b), to_dev(d)) for b, d in chunks]
        d_reqs = [to_dev(r) for r in reqs]
        outs = [Guarded(16 * ns), Guarded(16 * ns)]
        tab.update_dev(None, 0, to_dev(ent), len(ent), stream=st)
        for k in range(2):
            ch.walk_copy_read(*bufs[k], d_reqs[k], st)
            with torch.cuda.stream(st):
                outs[k].t.copy_(ch.rres.t)              # device to device, on the stream: no wait
        st.synchronize()
        dst = ch.dst.numpy()
        for g_ in (ch.dst, ch.rres, ch.total, ch.rwork, ch.state, ch.rbuf, ch.arena):
            assert g_.guard_intact()
        r0, r1 = (o.numpy(RCVREAD_RES_DTYPE) for o in outs)
        assert (r0["verdict"] == rm.READ).all() and (r1["verdict"] == rm.READ).all()
        for s in range(ns):
            got = b"".join(dst[int(rq["dst_off"][s]):int(rq["dst_off"][s]) + int(r["copylen"][s])].tobytes()
                           for rq, r in zip(reqs, (r0, r1)))
            assert got == bytes(sent[s]), s
            assert int(r0["copylen"][s]) == int(reqs[0]["len"][s]) and r0["flags"][s] & 1
            assert r1["flags"][s] == 4 and int(r1["rcv_wnd"][s]) == size       # emptied: the fragment freed, no MORE
        stt = ch.state.numpy(RCV_STATE_DTYPE)
        assert (stt["merged_len"] == 0).all() and (stt["nfrag"] == 0).all()
        assert (stt["head_seq"] == stt["rcv_nxt"]).all()
        assert stt["head_seq"].tolist() == [(int(state["head_seq"][s]) + len(sent[s])) & rm.M32 for s in range(ns)]


def test_captured_walk_copy_and_read_replayed_twice(gpu):
    rng = np.random.default_rng(12)
    ns, size, per_batch = 16, 1024, 4
    tuples, state, rbuf, arena, sent, chunks = chain_setup(rng, ns, size, per_batch, 1)
    n = ns * per_batch
    with gpu.Context(0) as cx, gpu.FlowTable(cx, 10) as tab:
        st = torch.cuda.Stream(device=DEV)
        res0 = oracle.rx_chunk(chunks[0][0], chunks[0][1], 0, None)
        ent = fm.entries(fm.record_keys(res0[:ns]), np.arange(ns, dtype=np.uint32))
        ch = Chain(gpu, cx, tab, n, ns - 1, state, rbuf, arena, ns, ns * size + 16)     # + 16: the ranges begin at byte 3
        rq = np.zeros(ns, RCVREAD_REQ_DTYPE)
        rq["sid"], rq["len"], rq["dst_off"] = np.arange(ns), size, np.arange(ns) * size + 3
        d_buf, d_desc, d_req = to_dev(chunks[0][0]), to_dev(chunks[0][1]), to_dev(rq)
        tab.update_dev(None, 0, to_dev(ent), len(ent), stream=st)
        ch.walk_copy_read(d_buf, d_desc, d_req, st)                     # kernels loaded, the group arrays written
        st.synchronize()
        first = [x.numpy().copy() for x in (ch.dst, ch.rres, ch.total, ch.state, ch.rbuf)]
        dst = first[0]
        for s in range(ns):
            assert dst[s * size + 3:s * size + 3 + len(sent[s])].tobytes() == bytes(sent[s])
        graph = torch.cuda.CUDAGraph()

        def reset():
            ch.state.t.copy_(to_dev(state)), ch.rbuf.t.copy_(to_dev(rbuf)), ch.arena.t.copy_(to_dev(arena))
            ch.dst.t.fill_(0x5A), ch.rres.t.fill_(SENT), ch.total.t.fill_(SENT), ch.rwork.t.fill_(0)
            torch.cuda.synchronize()

        reset()
        with torch.cuda.graph(graph, stream=st):
            ch.walk_copy_read(d_buf, d_desc, d_req, st, with_rx=False)
        for _ in range(2):
            reset()
            graph.replay()
            torch.cuda.synchronize()
            for x, y in zip(first, (ch.dst, ch.rres, ch.total, ch.state, ch.rbuf)):
                assert x.tobytes() == y.numpy().tobytes()
                assert y.guard_intact()
        del graph


# ---- the host form -----------------------------------------------------------------------------------------
class HostCall:
    def __init__(self, b):
        self.b = b
        self.state, self.rbuf = to_dev(b.state), to_dev(b.rbuf)
        self.tx, self.snd, self.arena = to_dev(b.tx), to_dev(b.snd), to_dev(b.arena)

    def reset(self):
        self.state.copy_(to_dev(self.b.state)), self.rbuf.copy_(to_dev(self.b.rbuf)), self.tx.copy_(to_dev(self.b.tx))

    def call(self, L, h):
        b, n = self.b, len(self.b.req)
        dst = b.dst.copy()
        rres, total = np.full(n, SENT, dtype=np.uint8).repeat(16).view(RCVREAD_RES_DTYPE), np.full(16, SENT, np.uint8).view(np.uint64)
        rc_ = L.mtcp_gpu_rcvread(h, b.req.ctypes.data, n, b.max_id, self.state.data_ptr(), self.rbuf.data_ptr(),
                                 self.tx.data_ptr(), self.snd.data_ptr(), self.arena.data_ptr(), len(b.arena),
                                 dst.ctypes.data, len(dst), rres.ctypes.data, total.ctypes.data)
        return rc_, dst, rres, total

    def check(self, got, want):
        rc_, dst, rres, total = got
        assert rc_ == 0
        assert rres.tobytes() == want[4].tobytes() and (dst == want[3]).all() and total.tolist() == want[5].tolist()
        torch.cuda.synchronize()
        assert self.state.cpu().numpy().tobytes() == want[0].tobytes()
        assert self.rbuf.cpu().numpy().tobytes() == want[1].tobytes()
        assert self.tx.cpu().numpy().tobytes() == want[2].tobytes()


def test_the_host_form_unbounded_bounded_and_behind_a_stalled_gpu(gpu):
    """The stalled-GPU pattern of tests/test_gpu_bounded.py (its helpers, its
    stall and limit values): ETIMEDOUT within the limit, nothing of the
    caller's written right after the call nor after the stall has ended, the
    context answers EIO, a fresh context gives the model's answers."""
    from mtcp_amd._lib import lib
    from tests.test_gpu_bounded import LIMIT_US, SLACK_S, STALL_US, stall_lib, stream_busy, stream_wait
    L, S = lib(), stall_lib()
    rng = np.random.default_rng(13)
    b = rc.random_batch(rng, 40, 150, dup=0.2)
    want = b.expect()
    assert (want[4]["verdict"] == rm.READ).sum() > 10 and (want[4]["verdict"] == rm.DUP).any()
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
    rc_, dst, rres, total = hc.call(L, c._h)
    dt = time.monotonic() - t0
    assert rc_ == ETIMEDOUT, rc_
    assert dt < LIMIT_US / 1e6 + SLACK_S, dt
    assert stream_busy(handle)
    untouched = lambda: (dst == b.dst).all() and (rres.view(np.uint8) == SENT).all() and (total.view(np.uint8) == SENT).all()
    assert untouched()
    assert L.mtcp_gpu_sync(c._h) == EIO
    assert hc.call(L, c._h)[0] == EIO
    own = torch.cuda.Stream(device=DEV)
    dc = Call(gpu, b)
    assert L.mtcp_gpu_rcvread_dev(c._h, dc.req.data_ptr(), dc.n, b.max_id, dc.state.t.data_ptr(), dc.rbuf.t.data_ptr(),
                                  dc.tx.t.data_ptr(), dc.snd.data_ptr(), dc.arena.data_ptr(), len(b.arena),
                                  dc.dst.t.data_ptr(), len(b.dst), dc.rres.t.data_ptr(), dc.total.t.data_ptr(),
                                  dc.work.t.data_ptr(), dc.wb, own.cuda_stream) == EIO
    c.close()
    stream_wait(handle)                                     # the stall and what was queued behind it end
    own.synchronize()
    assert untouched()
    assert (dc.rres.all == SENT).all().item() and dc.dst.numpy().tobytes() == b.dst.tobytes()
    with gpu.Context(0) as fresh:
        fresh.wait_limit = 5_000_000
        hc.reset()
        hc.check(hc.call(L, fresh._h), want)
        # the wrapper, an empty batch, and a gather above one stage
        hc.reset()
        dst = b.dst.copy()
        rres, total = fresh.rcvread(b.req, b.max_id, hc.state, hc.rbuf, hc.tx, hc.snd, hc.arena, dst)
        assert rres.tobytes() == want[4].tobytes() and (dst == want[3]).all()
        assert L.mtcp_gpu_rcvread(fresh._h, b.req.ctypes.data, 0, b.max_id, hc.state.data_ptr(), hc.rbuf.data_ptr(),
                                  None, None, hc.arena.data_ptr(), len(b.arena), dst.ctypes.data, len(dst),
                                  rres.ctypes.data, total.ctypes.data) == 0
        big = b.req.copy()
        big["len"] = (32 << 20) // len(big) + 16
        hc.reset()
        before = hc.state.cpu().numpy().tobytes()
        got = L.mtcp_gpu_rcvread(fresh._h, big.ctypes.data, len(big), b.max_id, hc.state.data_ptr(), hc.rbuf.data_ptr(),
                                 hc.tx.data_ptr(), hc.snd.data_ptr(), hc.arena.data_ptr(), len(b.arena), dst.ctypes.data,
                                 len(dst), rres.ctypes.data, total.ctypes.data)
        assert got == EINVAL and hc.state.cpu().numpy().tobytes() == before


# ---- error returns -------------------------------------------------------------------------------------------
def test_error_returns(gpu):
    from mtcp_amd._lib import lib
    L = lib()
    rng = np.random.default_rng(14)
    b = rc.random_batch(rng, 20, 40)
    c = Call(gpu, b)
    names = ["req", "state", "rbuf", "tx", "snd", "arena", "dst", "rres", "total", "work"]
    align = {"req": 16, "state": 64, "rbuf": 32, "tx": 32, "snd": 128, "arena": 16, "dst": 16, "rres": 16, "total": 8,
             "work": 16}
    tens = {"req": c.req, "state": c.state.t, "rbuf": c.rbuf.t, "tx": c.tx.t, "snd": c.snd, "arena": c.arena,
            "dst": c.dst.t, "rres": c.rres.t, "total": c.total.t, "work": c.work.t}

    def call(h, n=c.n, max_id=b.max_id, arena_bytes=len(b.arena), wb=c.wb, **kw):
        p = {k: t.data_ptr() for k, t in tens.items()}
        p.update(kw)
        return L.mtcp_gpu_rcvread_dev(h, p["req"], n, max_id, p["state"], p["rbuf"], p["tx"], p["snd"], p["arena"],
                                      arena_bytes, p["dst"], len(b.dst), p["rres"], p["total"], p["work"], wb, None)

    with gpu.Context(0) as cx:
        before = c.raw()
        assert call(None) == EINVAL
        for name in names:
            assert call(cx._h, **{name: None}) == EINVAL, name          # tx or snd alone NULL: EINVAL too
            t = tens[name]
            big = torch.zeros(t.numel() + 256, dtype=torch.uint8, device=DEV)
            base = (-big.data_ptr()) % 128
            assert call(cx._h, **{name: big.data_ptr() + base + align[name] // 2}) == EINVAL, name
        assert call(cx._h, wb=c.wb - 16) == EINVAL
        assert call(cx._h, arena_bytes=len(b.arena) - 8) == EINVAL
        assert call(cx._h, n=(1 << 26) + 1) == EINVAL
        assert call(cx._h, max_id=gm.MAX_ID + 1) == EINVAL
        assert call(cx._h, n=0, req=None, state=None, rbuf=None, tx=None, snd=None, arena=None, dst=None, rres=None,
                    total=None, work=None, wb=0) == 0                   # n == 0: OK without a launch
        torch.cuda.synchronize()
        for x, y in zip(before, c.raw()):
            assert (x is None and y is None) or x.tobytes() == y.tobytes()
        hc = HostCall(b)
        dst, rres, total = b.dst.copy(), np.zeros(c.n, RCVREAD_RES_DTYPE), np.zeros(2, np.uint64)
        host = lambda **kw: L.mtcp_gpu_rcvread(*[kw.get(k, v) for k, v in (
            ("h", cx._h), ("req", b.req.ctypes.data), ("n", c.n), ("max_id", b.max_id), ("state", hc.state.data_ptr()),
            ("rbuf", hc.rbuf.data_ptr()), ("tx", hc.tx.data_ptr()), ("snd", hc.snd.data_ptr()),
            ("arena", hc.arena.data_ptr()), ("arena_bytes", len(b.arena)), ("dst", dst.ctypes.data),
            ("dst_bytes", len(dst)), ("rres", rres.ctypes.data), ("total", total.ctypes.data))])
        for k in ("h", "req", "state", "rbuf", "tx", "snd", "arena", "dst", "rres", "total"):
            assert host(**{k: None}) == EINVAL, k
        assert host(arena_bytes=len(b.arena) - 1) == EINVAL and host(max_id=gm.MAX_ID + 1) == EINVAL
        assert host(state=hc.state.data_ptr() + 32) == EINVAL
        assert (dst == b.dst).all() and not rres.view(np.uint8).any()
        assert host(tx=None, snd=None) == 0
