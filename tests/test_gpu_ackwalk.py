"""The per-stream ProcessACK walk on the GPU (include/mtcp_gpu_ackwalk.h,
mtcp_amd/csrc/ackwalk_kernels.hpp): every byte of d_ack, d_snd and
d_ack_stop[:m] of every case is compared with tests/ackwalk_model.py; none is
sampled.

Guard regions sit behind every output, the workspace is exactly sized and
pre-filled with 0xA5, d_ack_stop past m keeps its sentinel, records of streams
absent from the batch keep every byte and every record its bytes 88-127.
Batch sizes around the wave and one workgroup's records, segment lengths around
the wave and the lanes' round length, 64 and 65 segments, 65 536 packets over
4 096 streams, one heavy stream among short ones, batches that are all MISS /
NONE or all deferred, the random family of tests/ackwalk_gen.py, wrapping
streams, send states and placement records of random bytes, no option records,
purity, the chain rx + tcpopt + lookup + group + rcvwalk + ackwalk on one stream
against the oracle's records, the same chain captured and replayed once, the
host calls (unbounded, bounded) and the error returns.  The timeout path is
HostCall's (tests/test_host_call_rules.py covers it on the CPU)."""
import numpy as np
import pytest

import oracle
from mtcp_amd import _types as T
from mtcp_amd._types import ACK_REC_DTYPE, ACK_STATE_DTYPE, RCV_PLACE_DTYPE, RCV_STATE_DTYPE, TCPOPT_DTYPE, TCPOPT_TS_FOUND
from tests import ackwalk_gen as ag
from tests import ackwalk_model as am
from tests import flowtab_model as fm
from tests import group_model as gm
from tests import rcvwalk_model as rm
from tests import tcpopt_model as tm

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EINVAL = -22
GUARD = 4096
SENT = 0xA5
SENT32 = 0xA5A5A5A5
MISS, NONE, MAX_ID = gm.FLOW_MISS, gm.FLOW_NONE, gm.MAX_ID


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")
    from mtcp_amd import gpu as g
    return g


@pytest.fixture(scope="module")
def ctx(gpu):
    with gpu.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def RT(gpu):
    return gpu.Context.ackwalk_short_len()


def to_dev(a: np.ndarray):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)


class Guarded:
    """`nbytes` of device memory filled with `fill` and a guard region of SENT behind it."""

    def __init__(self, nbytes, fill=SENT):
        self.nbytes = nbytes
        self.all = torch.full((nbytes + GUARD,), SENT, dtype=torch.uint8, device=DEV)
        self.t = self.all[:nbytes]
        if isinstance(fill, np.ndarray):
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(fill).view(np.uint8).reshape(-1)).to(DEV))
        elif fill != SENT:
            self.t.fill_(fill)

    def guard_intact(self):
        return bool((self.all[self.nbytes:] == SENT).all().item())

    def numpy(self, dtype=np.uint32):
        return self.t.cpu().numpy().view(dtype)


class Call:
    """The device arrays of one call on batch b (b["group"], b["place"]: the
    models', or the device tensors the launches in front fill), the outputs
    guarded."""

    def __init__(self, gpu, b, work_fill=SENT, group_on_device=None, place_on_device=None):
        self.b, self.n, self.max_id = b, len(b["res"]), b["max_id"]
        n = self.n
        self.res = to_dev(b["res"])
        self.opt = to_dev(b["opt"]) if b["opt"] is not None else None
        self.d_place = to_dev(b["place"]) if place_on_device is None else place_on_device
        if group_on_device is None:
            idx, seg_sid, seg_start = b["group"]
            self.m = len(seg_sid)
            pad = lambda a, k: np.concatenate([a, np.full(k - len(a), SENT32, np.uint32)])
            self.idx, self.seg_sid = to_dev(idx), to_dev(pad(seg_sid, n))
            self.seg_start, self.nseg = to_dev(pad(seg_start, n + 1)), to_dev(np.array([self.m], np.uint32))
        else:
            self.idx, self.seg_sid, self.seg_start, self.nseg = group_on_device
        self.snd = Guarded(128 * (self.max_id + 1), b["snd"])
        self.ack, self.stop = Guarded(16 * n), Guarded(4 * n)
        self.wb = gpu.Context.ackwalk_work_bytes(n, self.max_id)
        assert self.wb > 0
        self.work = Guarded(self.wb, work_fill)

    def run(self, ctx, stream=None):
        ctx.ackwalk_dev(self.res, self.opt, self.d_place, self.n, self.max_id, self.idx, self.seg_sid, self.seg_start,
                        self.nseg, self.b["cur_ts"], self.snd.t, self.ack.t, self.stop.t, self.work.t, stream=stream)

    def reset(self):
        self.snd.t.copy_(to_dev(self.b["snd"]))
        self.ack.t.fill_(SENT)
        self.stop.t.fill_(SENT)

    def raw(self):
        return (self.ack.numpy(ACK_REC_DTYPE).copy(), self.snd.numpy(ACK_STATE_DTYPE).copy(), self.stop.numpy().copy())

    def check(self, want, what=""):
        for name in ("snd", "ack", "stop", "work"):
            assert getattr(self, name).guard_intact(), f"{what}: bytes behind {name} were written"
        ack, snd, stop = self.raw()
        w_ack, w_snd, w_stop = want
        m = len(w_stop)
        for got, exp, name in ((ack, w_ack, "ack"), (snd, w_snd, "snd"), (stop[:m], w_stop, "ack_stop")):
            bad = np.nonzero(got != exp)[0]
            assert len(bad) == 0, f"{what}: {len(bad)} of {len(exp)} {name} records differ, first at {bad[0]}: " \
                                  f"{got[bad[0]]} want {exp[bad[0]]}"
            assert got.tobytes() == exp.tobytes(), f"{what}: {name}"
        assert (stop[m:] == SENT32).all(), f"{what}: ack_stop past m was written"
        assert snd["user"].tobytes() == self.b["snd"]["user"].tobytes(), f"{what}: bytes 88-127 of a record changed"


def run(gpu, ctx, b, what="", work_fill=SENT):
    want = ag.expect(b)
    c = Call(gpu, b, work_fill)
    c.run(ctx)
    torch.cuda.synchronize()
    c.check(want, what)
    absent = np.setdiff1d(np.arange(b["max_id"] + 1), b["sid"][b["sid"] <= b["max_id"]])
    assert c.raw()[1][absent].tobytes() == b["snd"][absent].tobytes(), f"{what}: an absent stream's record changed"
    return c


def lens_for(rng, n, extra):
    """Stream lengths of 1-40 packets that sum to n - extra."""
    lens, left = [], n - extra
    while left > 0:
        k = int(min(left, rng.integers(1, 41)))
        lens.append(k)
        left -= k
    return lens


# ---- shapes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4095, 4096, 4097])
def test_batch_sizes(gpu, ctx, n):
    rng = np.random.default_rng(n)
    if n == 1:
        for extra in (0, 1):
            run(gpu, ctx, ag.batch(rng, lens_for(rng, 1, extra), extra=extra), f"n = 1, extra = {extra}")
        return
    extra = n // 16
    b = ag.batch(rng, lens_for(rng, n, extra), extra=extra, special=ag.family_special, snd_special=ag.family_snd_special)
    assert len(b["res"]) == n
    run(gpu, ctx, b, f"n = {n}")


@pytest.mark.parametrize("nseg", [64, 65])
def test_segment_lengths_around_the_wave_and_the_round(gpu, ctx, RT, nseg):
    """Every length at which the walker takes another path (RT: the packets a
    lane walks per round), in a table of 64 and of 65 segments: a wave's last
    lane has and has not a segment."""
    rng = np.random.default_rng(nseg)
    pool = [RT - 1, RT, RT + 1, 2 * RT + 1, 63, 64, 65, 129, 1, 2]
    lens = [pool[(k * 7 + nseg) % len(pool)] for k in range(nseg)]
    lens[0], lens[-1] = RT + 1, RT                         # a round and one packet first, exactly one round last
    assert set(lens) == set(pool)
    b = ag.batch(rng, lens, fin=0.0)
    assert len(b["group"][1]) == nseg
    run(gpu, ctx, b, f"{nseg} segments")
    b = ag.batch(rng, lens, extra=5)                       # and with the MISS and NONE segments behind them
    run(gpu, ctx, b, f"{nseg} stream segments, MISS and NONE")


def test_65536_packets_over_4096_streams(gpu, ctx):
    rng = np.random.default_rng(40)
    b = ag.batch(rng, [16] * 4096, max_id=5000)
    assert len(b["res"]) == 65536
    c = run(gpu, ctx, b, "65 536 packets")
    counts = np.bincount(c.raw()[0]["verdict"], minlength=16)
    assert all(counts[v] > 0 for v in am.WALKED)


def test_one_heavy_stream_among_1024_short_ones(gpu, ctx):
    rng = np.random.default_rng(41)
    lens = [int(k) for k in rng.integers(1, 9, 1024)]
    lens[500] = 3000
    def long_buffer(r, s, snd):                             # the heavy stream's ACKs find new data to the end
        if s != 500:
            return None
        snd.sb_size, snd.sb_len, snd.snd_wnd = 1 << 26, (1 << 26) - 5000, 5000
        snd.snd_nxt = (snd.sb_head_seq + snd.sb_len) & am.M32
        return snd
    b = ag.batch(rng, lens, fin=0.0, snd_special=long_buffer)
    c = run(gpu, ctx, b, "one stream of 3 000 packets")
    heavy = np.argmax(np.bincount(b["sid"][b["sid"] <= b["max_id"]]))
    v = c.raw()[0]["verdict"][b["sid"] == heavy]
    assert len(v) == 3000 and np.isin(v, am.WALKED).sum() > 500 and (v == am.ACK_NEW).sum() > 200


def test_all_miss_or_none_and_all_deferred(gpu, ctx):
    rng = np.random.default_rng(42)
    b = ag.batch(rng, [], max_id=50, extra=700)
    c = run(gpu, ctx, b, "every packet MISS or NONE")
    assert c.raw()[0].tobytes() == bytes(16 * 700)
    assert c.raw()[1].tobytes() == b["snd"].tobytes()

    def other_state(r, s, snd):
        snd.tcp_state = 3 + (s % 7 > 0) * (1 + s % 7)       # every state but ESTABLISHED
        return snd
    b = ag.batch(rng, lens_for(rng, 900, 0), snd_special=other_state)
    c = run(gpu, ctx, b, "every stream defers at its first packet")
    ack, snd, stop = c.raw()
    assert set(ack["verdict"].tolist()) == {am.DEFER_STATE, am.DEFER_BEHIND}
    assert snd.tobytes() == b["snd"].tobytes()
    assert np.array_equal(stop[:len(b["group"][1])], b["group"][2][:-1])


# ---- content ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def family():
    """The batch tests/test_ackwalk_model.py holds to its statistics."""
    b = ag.family()
    ag.expect(b)
    return b


def test_random_family(gpu, ctx, family):
    c = run(gpu, ctx, family, "the family")
    ack = c.raw()[0]
    counts = np.bincount(ack["verdict"], minlength=16)
    assert all(counts[v] > 0 for v in am.WALKED) and counts[am.DEFER_RCV] > 0
    assert all((ack["flags"] & getattr(T, "ACK_" + f)).any() for f in T.ACK_FLAGS)


def test_wrapping_streams(gpu, ctx):
    rng = np.random.default_rng(43)
    b = ag.batch(rng, [12] * 400, wrap=True)
    c = run(gpu, ctx, b, "wrap")
    snd = c.raw()[1]
    moved = snd["snd_una"] != b["snd"]["snd_una"]
    assert (snd["snd_una"][moved] < b["snd"]["snd_una"][moved]).sum() > 50     # snd_una passed 2^32


def test_states_and_placements_of_random_bytes(gpu, ctx):
    b = ag.garbage_batch(np.random.default_rng(44), 4000, 6)
    c = run(gpu, ctx, b, "random state bytes")
    counts = np.bincount(c.raw()[0]["verdict"], minlength=16)
    assert counts[am.DEFER_BAD_STATE] > 1000 and counts[am.ACK_NEW] > 100 and counts[am.DEFER_ARITH] > 0, counts.tolist()
    assert (c.raw()[0]["verdict"][b["sid"] <= b["max_id"]] != am.NONE).all()    # every record written


def test_without_option_records(gpu, ctx, family):
    b = ag.drop_options(dict(family))
    c = run(gpu, ctx, b, "d_opt NULL")
    v = c.raw()[0]["verdict"]
    assert (v == am.DEFER_RCV).sum() > 50 and (v == am.ACK_NEW).sum() > 500


def test_purity(gpu, ctx, family):
    wb = gpu.Context.ackwalk_work_bytes(len(family["res"]), family["max_id"])
    fills = [SENT, 0, 0xFF, np.random.default_rng(45).integers(0, 256, wb, dtype=np.uint8)]
    seen = [run(gpu, ctx, family, f"workspace fill {i}", f).raw() for i, f in enumerate(fills)]
    for other in seen[1:]:
        for a, b in zip(seen[0], other):
            assert a.tobytes() == b.tobytes()


# ---- behind rx, tcpopt, lookup, group and the receive walk ---------------------------------------------
def make_chain_batch():
    """2 048 frames made from a generated batch, as tests/test_gpu_rcvwalk.py
    makes them, with the batch's ack_seq and window in the TCP header.  The
    expectation is the two models fed with the ORACLE's records of the frames
    and the option model's records."""
    rng = np.random.default_rng(46)
    b = ag.batch(rng, lens_for(rng, 1900, 0), extra=148)
    n = len(b["res"])
    assert n == 2048
    ids = np.unique(b["sid"][b["sid"] <= b["max_id"]])
    tuples = {int(s): rng.integers(1, 255, 12, dtype=np.uint8).tobytes() for s in ids}
    frames = []
    for i in range(n):
        r, o, s = b["res"][i], b["opt"][i], int(b["sid"][i])
        body = b""
        if int(o["flags"]) & TCPOPT_TS_FOUND:
            body = bytes([1, 1, 8, 10]) + int(o["ts_val"]).to_bytes(4, "big") + int(o["ts_ref"]).to_bytes(4, "big")
        body += rng.integers(0, 256, min(int(r["payload_len"]), 300), dtype=np.uint8).tobytes()
        f = tm.frame_raw(5, 8 if int(o["flags"]) & TCPOPT_TS_FOUND else 5, int(r["tcp_flags"]), body, seed=i)
        t = tuples.get(s, rng.integers(1, 255, 12, dtype=np.uint8).tobytes())
        f[26:34] = t[:8]                                    # saddr, daddr
        f[34:38] = t[8:12]                                  # sport, dport
        f[38:42] = int(r["seq"]).to_bytes(4, "big")
        f[42:46] = int(r["ack_seq"]).to_bytes(4, "big")
        f[48:50] = int(r["window"]).to_bytes(2, "big")
        frames.append(f)
    buf, desc = tm.pack_chunk(frames, slot=64)
    tm.fill_checksums(buf, desc)
    for i in np.nonzero(b["sid"] == NONE)[0]:
        buf[int(desc["offset"][i]) + 50] ^= 0x55            # the TCP checksum no longer holds
    desc = desc.astype(oracle.DESC_DTYPE)
    res = oracle.rx_chunk(buf, desc, 0, None)
    ok = res["verdict"] == 0
    assert (~ok).sum() == (b["sid"] == NONE).sum()
    assert np.array_equal(res["ack_seq"][ok], b["res"]["ack_seq"][ok]) and np.array_equal(res["window"][ok], b["res"]["window"][ok])
    opt = np.zeros(n, TCPOPT_DTYPE)
    for i in np.nonzero(ok)[0]:
        ihl, doff = int(res["ihl_doff"][i]) & 15, int(res["ihl_doff"][i]) >> 4
        first = int(desc["offset"][i]) + 34 + 4 * ihl
        avail = int(desc["offset"][i]) + int(desc["len"][i]) - first
        blk = np.zeros(64, np.uint8)
        take = max(0, min(64, avail))
        blk[:take] = buf[first:first + take]
        opt[i] = tm.expected_record(blk, 4 * doff - 20, int(res["tcp_flags"][i]), avail)
    first_of = {s: int(np.nonzero(b["sid"] == s)[0][0]) for s in tuples}
    ent = fm.entries(fm.record_keys(res[[first_of[int(s)] for s in ids]]), ids.astype(np.uint32))
    model = fm.FlowTable()
    model.update(ins=ent)
    sid = model.lookup(res)
    assert np.array_equal(sid, b["sid"])
    chain = {"res": res, "opt": opt, "sid": sid, "state": b["state"], "snd": b["snd"], "max_id": b["max_id"],
             "cur_ts": b["cur_ts"], "group": gm.group(sid, b["max_id"])}
    chain["rcv_want"] = rm.walk(res, opt, chain["max_id"], *chain["group"], chain["state"])
    chain["place"] = chain["rcv_want"][0]
    ack = ag.expect(chain)[0]
    counts = np.bincount(ack["verdict"], minlength=16)
    assert counts[am.ACK_NEW] > 500 and counts[am.ACK_OLD] > 50 and counts[am.NONE] == 148, counts.tolist()
    return buf, desc, ent, chain


@pytest.fixture(scope="module")
def chain_batch():
    return make_chain_batch()


def group_outputs(n):
    return Guarded(4 * n), Guarded(4 * n), Guarded(4 * n + 4), Guarded(4)


class Chain:
    """The device arrays of rx + tcpopt + lookup + group + rcvwalk + ackwalk for chain_batch."""

    def __init__(self, gpu, chain_batch):
        self.buf, self.desc, self.ent, self.chain = chain_batch
        n, max_id = len(self.desc), self.chain["max_id"]
        self.n, self.max_id = n, max_id
        self.d_buf, self.d_desc, self.d_ent = to_dev(self.buf), to_dev(self.desc), to_dev(self.ent)
        self.d_res = torch.zeros(n * 40, dtype=torch.uint8, device=DEV)
        self.d_opt = torch.zeros(n * 16, dtype=torch.uint8, device=DEV)
        self.sid, self.g = Guarded(4 * n), group_outputs(n)
        self.gwork = Guarded(gpu.Context.group_work_bytes(n, max_id))
        self.rwork = Guarded(gpu.Context.rcvwalk_work_bytes(n, max_id))
        self.state = Guarded(64 * (max_id + 1), self.chain["state"])
        self.place, self.rstop = Guarded(16 * n), Guarded(4 * n)
        self.c = Call(gpu, self.chain, group_on_device=tuple(x.t for x in self.g), place_on_device=self.place.t)
        self.c.res, self.c.opt = self.d_res, self.d_opt

    def launch(self, cx, tab, st):
        n, max_id, g = self.n, self.max_id, tuple(x.t for x in self.g)
        cx.rx_chunk_dev(self.d_buf, self.d_desc, n, 0, self.d_res, stream=st)
        cx.rx_tcpopt_chunk_dev(self.d_buf, self.d_desc, n, 0, self.d_res, self.d_opt, stream=st)
        tab.lookup_dev(self.d_res, n, self.sid.t, None, stream=st)
        cx.group_dev(self.sid.t, n, max_id, *g, self.gwork.t, stream=st)
        cx.rcvwalk_dev(self.d_res, self.d_opt, n, max_id, *g, self.state.t, self.place.t, self.rstop.t, self.rwork.t,
                       stream=st)
        self.c.run(cx, stream=st)

    def reset(self):
        self.c.reset()
        self.state.t.copy_(to_dev(self.chain["state"]))
        for x in (self.sid, self.place, self.rstop, *self.g):
            x.t.fill_(SENT)
        self.d_res.zero_()
        self.d_opt.zero_()
        self.c.work.t.fill_(0)

    def check(self, what):
        chain = self.chain
        assert self.d_res.cpu().numpy().tobytes() == chain["res"].tobytes(), what
        assert self.d_opt.cpu().numpy().tobytes() == chain["opt"].tobytes(), what
        assert np.array_equal(self.sid.numpy(), chain["sid"]), what
        assert self.g[3].numpy()[0] == len(chain["group"][1]), what
        assert self.place.numpy(RCV_PLACE_DTYPE).tobytes() == chain["rcv_want"][0].tobytes(), what
        assert self.state.numpy(RCV_STATE_DTYPE).tobytes() == chain["rcv_want"][1].tobytes(), what
        for x in (self.sid, self.place, self.rstop, self.state, self.gwork, self.rwork, *self.g):
            assert x.guard_intact(), what
        self.c.check(chain["want"], what)


def test_chain_on_one_stream(gpu, chain_batch):
    ch = Chain(gpu, chain_batch)
    st = torch.cuda.Stream(device=DEV)
    with gpu.Context(0) as cx, gpu.FlowTable(cx, 12) as tab:
        tab.update_dev(None, 0, ch.d_ent, len(ch.ent), stream=st)
        ch.launch(cx, tab, st)
        st.synchronize()
    ch.check("behind rx, tcpopt, lookup, group and the receive walk")


def test_captured_chain_replayed(gpu, chain_batch):
    """The six launches of the chain captured once (a linear chain on one
    stream) and replayed once from reset state."""
    ch = Chain(gpu, chain_batch)
    st = torch.cuda.Stream(device=DEV)
    with gpu.Context(0) as cx, gpu.FlowTable(cx, 12) as tab:
        tab.update_dev(None, 0, ch.d_ent, len(ch.ent), stream=st)
        ch.launch(cx, tab, st)                              # kernels loaded before the capture
        st.synchronize()
        ch.check("before the capture")
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            ch.launch(cx, tab, st)
        ch.reset()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        ch.check("the replay")
        del graph


# ---- host calls ---------------------------------------------------------------------------------------
def host_call(L, c, b):
    idx, seg_sid, seg_start = b["group"]
    n, m = len(b["res"]), len(seg_sid)
    res, opt, place = np.ascontiguousarray(b["res"]), np.ascontiguousarray(b["opt"]), np.ascontiguousarray(b["place"])
    snd = b["snd"].copy()
    ack = np.full(16 * n, SENT, np.uint8).view(ACK_REC_DTYPE)
    stop = np.full(n, SENT32, np.uint32)
    nseg = np.array([m], np.uint32)
    rc = L.mtcp_gpu_ackwalk(c._h, res.ctypes.data, opt.ctypes.data, place.ctypes.data, n, b["max_id"], idx.ctypes.data,
                            seg_sid.ctypes.data, seg_start.ctypes.data, nseg.ctypes.data, b["cur_ts"], snd.ctypes.data,
                            ack.ctypes.data, stop.ctypes.data)
    return rc, (ack, snd, stop)


def host_check(got, b, what=""):
    ack, snd, stop = got
    w_ack, w_snd, w_stop = b["want"]
    m = len(w_stop)
    assert ack.tobytes() == w_ack.tobytes() and snd.tobytes() == w_snd.tobytes(), what
    assert np.array_equal(stop[:m], w_stop) and (stop[m:] == SENT32).all(), what


@pytest.mark.parametrize("limit", [0, 5_000_000], ids=["unbounded", "bounded"])
def test_host_calls(gpu, family, limit):
    from mtcp_amd._lib import lib
    L = lib()
    rng = np.random.default_rng(47)
    small = ag.batch(rng, [3, 1, 40], extra=2)              # the staging reused by a smaller call
    ag.expect(small)
    with gpu.Context(0) as c:
        if limit:
            c.wait_limit = limit
        for b in (family, small, family):
            rc, got = host_call(L, c, b)
            assert rc == 0
            host_check(got, b)
        snd = family["snd"].copy()                          # the Python view
        ack, stop = c.ackwalk(family["res"], family["opt"], family["place"], family["max_id"], *family["group"],
                              family["cur_ts"], snd)
        assert ack.tobytes() == family["want"][0].tobytes() and snd.tobytes() == family["want"][1].tobytes()
        assert np.array_equal(stop, family["want"][2])
        b = ag.drop_options(dict(family))
        snd = b["snd"].copy()
        want = ag.expect(b)
        ack, stop = c.ackwalk(b["res"], None, b["place"], b["max_id"], *b["group"], b["cur_ts"], snd)
        assert ack.tobytes() == want[0].tobytes() and snd.tobytes() == want[1].tobytes()


# ---- error returns -------------------------------------------------------------------------------------
def test_error_returns(gpu, ctx):
    from mtcp_amd._lib import lib
    L = lib()
    rng = np.random.default_rng(48)
    b = ag.batch(rng, lens_for(rng, 600, 20), extra=20)
    ag.expect(b)
    n, max_id, ts = len(b["res"]), b["max_id"], b["cur_ts"]
    d = Call(gpu, b)
    room = {k: Guarded(v.numel() + 64) for k, v in (("res", d.res), ("opt", d.opt), ("place", d.d_place), ("idx", d.idx),
                                                     ("seg_sid", d.seg_sid), ("seg_start", d.seg_start),
                                                     ("nseg", d.nseg))}
    p = lambda t, off=0: t.data_ptr() + off
    big = (1 << 26) + 1

    def dev(c=ctx._h, r=p(d.res), o=p(d.opt), pc=p(d.d_place), n_=n, mx=max_id, i=p(d.idx), ss=p(d.seg_sid),
            st=p(d.seg_start), ns=p(d.nseg), s=p(d.snd.t), a=p(d.ack.t), sp=p(d.stop.t), w=p(d.work.t), wbytes=d.wb):
        return L.mtcp_gpu_ackwalk_dev(c, r, o, pc, n_, mx, i, ss, st, ns, ts, s, a, sp, w, wbytes, None)

    bad = {
        "ctx NULL": dev(c=None), "res NULL": dev(r=None), "place NULL": dev(pc=None), "idx NULL": dev(i=None),
        "seg_sid NULL": dev(ss=None), "seg_start NULL": dev(st=None), "nseg NULL": dev(ns=None), "snd NULL": dev(s=None),
        "ack NULL": dev(a=None), "ack_stop NULL": dev(sp=None), "work NULL": dev(w=None),
        "res misaligned": dev(r=p(room["res"].t, 4)), "opt misaligned": dev(o=p(room["opt"].t, 8)),
        "place misaligned": dev(pc=p(room["place"].t, 8)),
        "idx misaligned": dev(i=p(room["idx"].t, 2)), "seg_sid misaligned": dev(ss=p(room["seg_sid"].t, 1)),
        "seg_start misaligned": dev(st=p(room["seg_start"].t, 3)), "nseg misaligned": dev(ns=p(room["nseg"].t, 2)),
        "snd misaligned by 64": dev(s=p(d.snd.t, 64)), "snd misaligned by 16": dev(s=p(d.snd.t, 16)),
        "ack misaligned": dev(a=p(d.ack.t, 8)), "ack_stop misaligned": dev(sp=p(d.stop.t, 2)),
        "work misaligned": dev(w=p(d.work.t, 8)), "work too small": dev(wbytes=d.wb - 1), "no work bytes": dev(wbytes=0),
        "n too large": dev(n_=big), "max_id too large": dev(mx=MAX_ID + 1), "max_id is NONE": dev(mx=NONE),
    }
    with gpu.Context(0, compact=True) as cc:
        bad["compact context"] = dev(c=cc._h)
        res, opt, place = np.ascontiguousarray(b["res"]), np.ascontiguousarray(b["opt"]), np.ascontiguousarray(b["place"])
        idx, seg_sid, seg_start = b["group"]
        nseg = np.array([len(seg_sid)], np.uint32)
        h_snd = b["snd"].copy()
        h_ack, h_stop = np.full(16 * n, SENT, np.uint8), np.full(n, SENT32, np.uint32)

        def host(c=ctx._h, r=res.ctypes.data, o=opt.ctypes.data, pc=place.ctypes.data, n_=n, mx=max_id,
                 i=idx.ctypes.data, ss=seg_sid.ctypes.data, st=seg_start.ctypes.data, ns=nseg.ctypes.data,
                 s=h_snd.ctypes.data, a=h_ack.ctypes.data, sp=h_stop.ctypes.data):
            return L.mtcp_gpu_ackwalk(c, r, o, pc, n_, mx, i, ss, st, ns, ts, s, a, sp)

        bad.update({"host: ctx NULL": host(c=None), "host: res NULL": host(r=None), "host: place NULL": host(pc=None),
                    "host: idx NULL": host(i=None), "host: seg_sid NULL": host(ss=None),
                    "host: seg_start NULL": host(st=None), "host: nseg NULL": host(ns=None),
                    "host: snd NULL": host(s=None), "host: ack NULL": host(a=None), "host: ack_stop NULL": host(sp=None),
                    "host: n too large": host(n_=big), "host: max_id too large": host(mx=MAX_ID + 1),
                    "host: compact context": host(c=cc._h)})
    assert {k: v for k, v in bad.items() if v != EINVAL} == {}
    assert dev(n_=0) == 0 and host(n_=0) == 0
    assert dev(n_=0, r=None, o=None, pc=None, i=None, ss=None, st=None, ns=None, s=None, a=None, sp=None, w=None,
               wbytes=0) == 0
    torch.cuda.synchronize()
    for g in (d.ack, d.stop, d.work):                       # none of these wrote anything
        assert (g.all == SENT).all().item()
    assert d.snd.numpy(ACK_STATE_DTYPE).tobytes() == b["snd"].tobytes() and d.snd.guard_intact()
    assert (h_ack == SENT).all() and (h_stop == SENT32).all() and h_snd.tobytes() == b["snd"].tobytes()
    assert dev() == 0 and host() == 0                       # and the same arguments, valid, work
    torch.cuda.synchronize()
    d.check(b["want"], "after the refused calls")
    host_check((h_ack.view(ACK_REC_DTYPE), h_snd, h_stop), b)
    d.reset()
    assert dev(o=None) == 0                                 # d_opt may be NULL
    torch.cuda.synchronize()
