"""The per-stream receive walk on the GPU (include/mtcp_gpu_rcvwalk.h,
mtcp_amd/csrc/rcvwalk_kernels.hpp): every byte of d_place, d_state and
d_seg_stop[:m] of every case is compared with tests/rcvwalk_model.py; none is
sampled.

Guard regions sit behind every output, the workspace is exactly sized and
pre-filled with 0xA5, d_seg_stop past m keeps its sentinel, records of streams
absent from the batch keep every byte.  Batch sizes around the wave and one
workgroup's records, segment lengths around the wave and the lanes'
round length, 64 and 65 segments, 65 536 packets over 4 096 streams, one heavy
stream among short ones, batches that are all MISS / NONE or all deferred, the
random family of tests/rcvwalk_gen.py, wrapping streams and distances of 2^31,
states of random bytes, no option records, purity, the chain rx + tcpopt +
lookup + group + walk on one stream against the oracle's records, a captured
graph replayed, the host calls (unbounded, bounded, behind a stalled GPU) and
the error returns."""
import time

import numpy as np
import pytest

import oracle
from mtcp_amd._types import (RCV_PLACE_DTYPE, RCV_STATE_DTYPE, RESULT_DTYPE, TCPOPT_DTYPE, TCPOPT_TS_FOUND,
                             TCPOPT_TS_UNPINNED)
from tests import flowtab_model as fm
from tests import group_model as gm
from tests import rcvwalk_gen as rg
from tests import rcvwalk_model as rm
from tests import tcpopt_model as tm

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EINVAL, EIO, ETIMEDOUT = -22, -5, -110
GUARD = 4096
SENT = 0xA5
SENT32 = 0xA5A5A5A5
MISS, NONE, MAX_ID = gm.FLOW_MISS, gm.FLOW_NONE, gm.MAX_ID
ACK = 0x10


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
def T(gpu):
    return gpu.Context.rcvwalk_short_len()


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
    """The device arrays of one call on batch b (b["group"]: the model's lists,
    or the device tensors a group launch fills), the outputs guarded."""

    def __init__(self, gpu, b, work_fill=SENT, group_on_device=None):
        self.b, self.n, self.max_id = b, len(b["res"]), b["max_id"]
        n = self.n
        self.res = to_dev(b["res"])
        self.opt = to_dev(b["opt"]) if b["opt"] is not None else None
        if group_on_device is None:
            idx, seg_sid, seg_start = b["group"]
            self.m = len(seg_sid)
            pad = lambda a, k: np.concatenate([a, np.full(k - len(a), SENT32, np.uint32)])
            self.idx, self.seg_sid = to_dev(idx), to_dev(pad(seg_sid, n))
            self.seg_start, self.nseg = to_dev(pad(seg_start, n + 1)), to_dev(np.array([self.m], np.uint32))
        else:
            self.idx, self.seg_sid, self.seg_start, self.nseg = group_on_device
        self.state = Guarded(64 * (self.max_id + 1), b["state"])
        self.place, self.stop = Guarded(16 * n), Guarded(4 * n)
        self.wb = gpu.Context.rcvwalk_work_bytes(n, self.max_id)
        assert self.wb > 0
        self.work = Guarded(self.wb, work_fill)

    def run(self, ctx, stream=None):
        ctx.rcvwalk_dev(self.res, self.opt, self.n, self.max_id, self.idx, self.seg_sid, self.seg_start, self.nseg,
                        self.state.t, self.place.t, self.stop.t, self.work.t, stream=stream)

    def reset(self):
        self.state.t.copy_(to_dev(self.b["state"]))
        self.place.t.fill_(SENT)
        self.stop.t.fill_(SENT)

    def raw(self):
        return (self.place.numpy(RCV_PLACE_DTYPE).copy(), self.state.numpy(RCV_STATE_DTYPE).copy(),
                self.stop.numpy().copy())

    def check(self, want, what=""):
        for name in ("state", "place", "stop", "work"):
            assert getattr(self, name).guard_intact(), f"{what}: bytes behind {name} were written"
        place, state, stop = self.raw()
        w_place, w_state, w_stop = want
        m = len(w_stop)
        for got, exp, name in ((place, w_place, "place"), (state, w_state, "state"), (stop[:m], w_stop, "seg_stop")):
            bad = np.nonzero(got != exp)[0]
            assert len(bad) == 0, f"{what}: {len(bad)} of {len(exp)} {name} records differ, first at {bad[0]}: " \
                                  f"{got[bad[0]]} want {exp[bad[0]]}"
            assert got.tobytes() == exp.tobytes(), f"{what}: {name}"
        assert (stop[m:] == SENT32).all(), f"{what}: seg_stop past m was written"


def expect(b):
    if "group" not in b:
        b["group"] = gm.group(b["sid"], b["max_id"])
    if "want" not in b:
        b["want"] = rm.walk(b["res"], b["opt"], b["max_id"], *b["group"], b["state"])
    return b["want"]


def run(gpu, ctx, b, what="", work_fill=SENT):
    want = expect(b)
    c = Call(gpu, b, work_fill)
    c.run(ctx)
    torch.cuda.synchronize()
    c.check(want, what)
    absent = np.setdiff1d(np.arange(b["max_id"] + 1), b["sid"][b["sid"] <= b["max_id"]])
    assert c.raw()[1][absent].tobytes() == b["state"][absent].tobytes(), f"{what}: an absent stream's record changed"
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
            run(gpu, ctx, rg.batch(rng, lens_for(rng, 1, extra), extra=extra), f"n = 1, extra = {extra}")
        return
    extra = n // 16
    b = rg.batch(rng, lens_for(rng, n, extra), extra=extra, special=rg.family_special)
    assert len(b["res"]) == n
    run(gpu, ctx, b, f"n = {n}")


@pytest.mark.parametrize("nseg", [64, 65])
def test_segment_lengths_around_the_wave_and_the_threshold(gpu, ctx, T, nseg):
    """Every length at which the walker takes another path (T: the packets a
    lane walks per round), in a table of 64 and of 65 segments: a wave's last
    lane has and has not a segment."""
    rng = np.random.default_rng(nseg)
    pool = [1, 2, 63, 64, 65, 127, 128, 129, T - 1, T, T + 1]
    lens = [pool[(k * 7 + nseg) % len(pool)] for k in range(nseg)]
    lens[0], lens[-1] = T + 1, T                           # a round and one packet first, exactly one round last
    assert set(lens) == set(pool)
    b = rg.batch(rng, lens)
    expect(b)
    assert len(b["group"][1]) == nseg
    run(gpu, ctx, b, f"{nseg} segments")
    b = rg.batch(rng, lens, extra=5)                       # and with the MISS and NONE segments behind them
    run(gpu, ctx, b, f"{nseg} stream segments, MISS and NONE")


def test_65536_packets_over_4096_streams(gpu, ctx):
    rng = np.random.default_rng(40)
    b = rg.batch(rng, [16] * 4096, max_id=5000)
    assert len(b["res"]) == 65536
    c = run(gpu, ctx, b, "65 536 packets")
    counts = np.bincount(c.raw()[0]["verdict"], minlength=16)
    assert all(counts[v] > 0 for v in rm.WALKED)


def test_one_heavy_stream_among_1024_short_ones(gpu, ctx):
    rng = np.random.default_rng(41)
    lens = [int(k) for k in rng.integers(1, 9, 1024)]
    lens[500] = 8192
    b = rg.batch(rng, lens, defers=False)                  # no FIN: the heavy stream is walked until reordering
                                                           # leaves it a fifth fragment, thousands of packets in
    c = run(gpu, ctx, b, "one stream of 8 192 packets")
    heavy = np.argmax(np.bincount(b["sid"][b["sid"] <= b["max_id"]]))
    v = c.raw()[0]["verdict"][b["sid"] == heavy]
    assert (v == rm.PUT_STORED).sum() > 2000 and (v == rm.DEFER_BEHIND).sum() > 2000


def test_all_miss_or_none_and_all_deferred(gpu, ctx):
    rng = np.random.default_rng(42)
    b = rg.batch(rng, [], max_id=50, extra=700)
    c = run(gpu, ctx, b, "every packet MISS or NONE")
    assert c.raw()[0].tobytes() == bytes(16 * 700)
    assert c.raw()[1].tobytes() == b["state"].tobytes()

    def other_state(r, s, st):
        st.tcp_state = 3 + (s % 7 > 0) * (1 + s % 7)        # every state but ESTABLISHED
        return st
    b = rg.batch(rng, lens_for(rng, 900, 0), special=other_state)
    c = run(gpu, ctx, b, "every stream defers at its first packet")
    place, state, stop = c.raw()
    assert set(place["verdict"].tolist()) == {rm.DEFER_STATE, rm.DEFER_BEHIND}
    assert state.tobytes() == b["state"].tobytes()
    assert np.array_equal(stop[:len(b["group"][1])], b["group"][2][:-1])


# ---- content ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def family():
    """The batch tests/test_rcvwalk_model.py holds to its statistics."""
    rng = np.random.default_rng(2024)
    b = rg.batch(rng, rg.family_lens(rng, 500), extra=150, special=rg.family_special)
    expect(b)
    return b


def test_random_family(gpu, ctx, family):
    c = run(gpu, ctx, family, "the family")
    counts = np.bincount(c.raw()[0]["verdict"], minlength=16)
    assert all(counts[v] > 0 for v in rm.WALKED) and counts[rm.DEFER_FLAGS] > 0
    assert (family["opt"]["flags"] & TCPOPT_TS_UNPINNED).any() and counts[rm.DEFER_TS] > 0


def test_wrap_and_two_to_the_31(gpu, ctx):
    rng = np.random.default_rng(43)
    b = rg.batch(rng, [12] * 400, wrap=True)
    n = len(b["res"])
    r = rng.random(n)
    b["res"]["seq"] = np.where(r < 0.05, b["res"]["seq"] + np.uint32(0x80000000), b["res"]["seq"])
    b["res"]["seq"] = np.where((r >= 0.05) & (r < 0.08),
                               b["res"]["seq"] + np.uint32(0x80000000) - b["res"]["payload_len"], b["res"]["seq"])
    b["opt"]["ts_val"] = np.where((r >= 0.08) & (r < 0.12), b["opt"]["ts_val"] + np.uint32(0x80000000),
                                  b["opt"]["ts_val"])
    # fragments exactly 2^31 from the head: the two orders disagree inside RBPut too
    far = np.nonzero(b["state"]["nfrag"] >= 2)[0][::3]
    b["state"]["frag"]["seq"][far, 1] = b["state"]["head_seq"][far] + np.uint32(0x80000000)
    c = run(gpu, ctx, b, "wrap and 2^31")
    st = c.raw()[1]
    moved = st["rcv_nxt"] != b["state"]["rcv_nxt"]
    assert (st["rcv_nxt"][moved] < b["state"]["rcv_nxt"][moved]).sum() > 50    # rcv_nxt passed 2^32


def test_states_of_random_bytes(gpu, ctx):
    b = rg.garbage_batch(np.random.default_rng(44), 4000, 6)
    c = run(gpu, ctx, b, "random state bytes")
    counts = np.bincount(c.raw()[0]["verdict"], minlength=16)
    assert counts[rm.DEFER_BAD_STATE] > 1000 and counts[rm.PUT_STORED] > 100, counts.tolist()


def test_without_option_records(gpu, ctx, family):
    b = dict(family, opt=None)
    del b["want"]
    c = run(gpu, ctx, b, "d_opt NULL")
    v = c.raw()[0]["verdict"]
    assert (v == rm.DEFER_TS).sum() > 50 and (v == rm.PUT_STORED).sum() > 1000
    assert not np.isin(v, (rm.PAWS_NO_TS, rm.PAWS_OLD)).any()


def test_purity(gpu, ctx, family):
    wb = gpu.Context.rcvwalk_work_bytes(len(family["res"]), family["max_id"])
    fills = [SENT, 0, 0xFF, np.random.default_rng(45).integers(0, 256, wb, dtype=np.uint8)]
    seen = [run(gpu, ctx, family, f"workspace fill {i}", f).raw() for i, f in enumerate(fills)]
    for other in seen[1:]:
        for a, b in zip(seen[0], other):
            assert a.tobytes() == b.tobytes()


# ---- behind rx, tcpopt, lookup and group ---------------------------------------------------------------
@pytest.fixture(scope="module")
def chain_batch():
    """2 048 frames made from a generated batch: the streams' frames carry
    their own 4-tuple, NOP NOP TS where the packet has a timestamp, a payload
    of at most 300 B; the MISS packets a tuple the table does not hold; the
    NONE packets a broken checksum.  The expectation is the model fed with the
    ORACLE's records of the frames and the option model's records."""
    rng = np.random.default_rng(46)
    lens = lens_for(rng, 1900, 0)
    b = rg.batch(rng, lens, extra=148)
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
        frames.append(f)
    buf, desc = tm.pack_chunk(frames, slot=64)
    tm.fill_checksums(buf, desc)
    for i in np.nonzero(b["sid"] == NONE)[0]:
        buf[int(desc["offset"][i]) + 50] ^= 0x55            # the TCP checksum no longer holds
    desc = desc.astype(oracle.DESC_DTYPE)
    res = oracle.rx_chunk(buf, desc, 0, None)
    ok = res["verdict"] == 0
    assert (~ok).sum() == (b["sid"] == NONE).sum()
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
    chain = {"res": res, "opt": opt, "sid": sid, "state": b["state"], "max_id": b["max_id"]}
    expect(chain)
    counts = np.bincount(chain["want"][0]["verdict"], minlength=16)
    assert counts[rm.PUT_STORED] > 800 and counts[rm.PAWS_OLD] > 5 and counts[rm.NONE] == 148
    return buf, desc, ent, chain


def group_outputs(n):
    return Guarded(4 * n), Guarded(4 * n), Guarded(4 * n + 4), Guarded(4)


def test_chain_on_one_stream(gpu, chain_batch):
    buf, desc, ent, chain = chain_batch
    n, max_id = len(desc), chain["max_id"]
    d_buf, d_desc, d_ent = to_dev(buf), to_dev(desc), to_dev(ent)
    d_res = torch.zeros(n * 40, dtype=torch.uint8, device=DEV)
    d_opt = torch.zeros(n * 16, dtype=torch.uint8, device=DEV)
    sid = Guarded(4 * n)
    g = group_outputs(n)
    gwork = Guarded(gpu.Context.group_work_bytes(n, max_id))
    c = Call(gpu, chain, group_on_device=tuple(x.t for x in g))
    c.res, c.opt = d_res, d_opt
    st = torch.cuda.Stream(device=DEV)
    with gpu.Context(0) as cx, gpu.FlowTable(cx, 12) as tab:
        cx.rx_chunk_dev(d_buf, d_desc, n, 0, d_res, stream=st)
        cx.rx_tcpopt_chunk_dev(d_buf, d_desc, n, 0, d_res, d_opt, stream=st)
        tab.update_dev(None, 0, d_ent, len(ent), stream=st)
        tab.lookup_dev(d_res, n, sid.t, None, stream=st)
        cx.group_dev(sid.t, n, max_id, *(x.t for x in g), gwork.t, stream=st)
        c.run(cx, stream=st)
        st.synchronize()
    assert d_res.cpu().numpy().tobytes() == chain["res"].tobytes()
    assert d_opt.cpu().numpy().tobytes() == chain["opt"].tobytes()
    assert np.array_equal(sid.numpy(), chain["sid"])
    assert g[3].numpy()[0] == len(chain["group"][1])
    c.check(chain["want"], "behind rx, tcpopt, lookup and group")


def test_captured_group_and_walk_replayed(gpu, chain_batch):
    """The group and walk launches captured once (a linear chain) and replayed
    once from reset state."""
    _, _, _, chain = chain_batch
    n, max_id = len(chain["res"]), chain["max_id"]
    d_sid = to_dev(chain["sid"])
    g = group_outputs(n)
    gwork = Guarded(gpu.Context.group_work_bytes(n, max_id))
    c = Call(gpu, chain, group_on_device=tuple(x.t for x in g))
    st = torch.cuda.Stream(device=DEV)
    with gpu.Context(0) as cx:
        def launch():
            cx.group_dev(d_sid, n, max_id, *(x.t for x in g), gwork.t, stream=st)
            c.run(cx, stream=st)

        launch()                                            # kernels loaded before the capture
        st.synchronize()
        c.check(chain["want"], "before the capture")
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            launch()
        c.reset()
        for x in g:
            x.t.fill_(SENT)
        c.work.t.fill_(0)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        c.check(chain["want"], "the replay")
        del graph


# ---- host calls ---------------------------------------------------------------------------------------
def host_call(L, c, b):
    idx, seg_sid, seg_start = b["group"]
    n, m = len(b["res"]), len(seg_sid)
    res, opt = np.ascontiguousarray(b["res"]), np.ascontiguousarray(b["opt"])
    state = b["state"].copy()
    place = np.full(16 * n, SENT, np.uint8).view(RCV_PLACE_DTYPE)
    stop = np.full(n, SENT32, np.uint32)
    nseg = np.array([m], np.uint32)
    rc = L.mtcp_gpu_rcvwalk(c._h, res.ctypes.data, opt.ctypes.data, n, b["max_id"], idx.ctypes.data,
                            seg_sid.ctypes.data, seg_start.ctypes.data, nseg.ctypes.data, state.ctypes.data,
                            place.ctypes.data, stop.ctypes.data)
    return rc, (place, state, stop)


def host_check(got, b, what=""):
    place, state, stop = got
    w_place, w_state, w_stop = b["want"]
    m = len(w_stop)
    assert place.tobytes() == w_place.tobytes() and state.tobytes() == w_state.tobytes(), what
    assert np.array_equal(stop[:m], w_stop) and (stop[m:] == SENT32).all(), what


def untouched(got, b):
    place, state, stop = got
    return (place.view(np.uint8) == SENT).all() and state.tobytes() == b["state"].tobytes() and (stop == SENT32).all()


@pytest.mark.parametrize("limit", [0, 5_000_000], ids=["unbounded", "bounded"])
def test_host_calls(gpu, family, limit):
    from mtcp_amd._lib import lib
    L = lib()
    rng = np.random.default_rng(47)
    small = rg.batch(rng, [3, 1, 40], extra=2)              # the staging reused by a smaller call
    expect(small)
    with gpu.Context(0) as c:
        if limit:
            c.wait_limit = limit
        for b in (family, small, family):
            rc, got = host_call(L, c, b)
            assert rc == 0
            host_check(got, b)
        state = family["state"].copy()                      # the Python view
        place, stop = c.rcvwalk(family["res"], family["opt"], family["max_id"], *family["group"], state)
        assert place.tobytes() == family["want"][0].tobytes() and state.tobytes() == family["want"][1].tobytes()
        assert np.array_equal(stop, family["want"][2])
        state = family["state"].copy()
        want = rm.walk(family["res"], None, family["max_id"], *family["group"], family["state"])
        place, stop = c.rcvwalk(family["res"], None, family["max_id"], *family["group"], state)
        assert place.tobytes() == want[0].tobytes() and state.tobytes() == want[1].tobytes()


def test_host_call_gives_up_at_the_limit(gpu, family):
    """The stalled-GPU pattern of tests/test_gpu_bounded.py (its helpers, its
    stall and limit values), as tests/test_gpu_group.py does it: ETIMEDOUT
    within the limit, nothing of the caller's is written (the state array
    included) right after the call and after the stall has ended, the context
    answers EIO, a fresh context gives the model's answers."""
    from mtcp_amd._lib import lib
    from tests.test_gpu_bounded import LIMIT_US, SLACK_S, STALL_US, stall_lib, stream_busy, stream_wait
    L, S = lib(), stall_lib()
    b = family
    c = gpu.Context(0)
    handle = c.stream
    rc, got = host_call(L, c, b)                            # unbounded: stage sized, kernels loaded
    assert rc == 0
    host_check(got, b)
    c.wait_limit = LIMIT_US
    rc, got = host_call(L, c, b)                            # bounded, no stall: the bounce buffers sized
    assert rc == 0
    host_check(got, b)
    assert S.mtcp_gpu_debug_stall(c._h, STALL_US) == 0
    t0 = time.monotonic()
    rc, got = host_call(L, c, b)
    dt = time.monotonic() - t0
    assert rc == ETIMEDOUT, rc
    assert dt < LIMIT_US / 1e6 + SLACK_S, dt
    assert stream_busy(handle)
    assert untouched(got, b)
    assert L.mtcp_gpu_sync(c._h) == EIO
    rc2, got2 = host_call(L, c, b)
    assert rc2 == EIO and untouched(got2, b)
    own = torch.cuda.Stream(device=DEV)
    d = Call(gpu, b)
    d.place.t.fill_(SENT)
    assert L.mtcp_gpu_rcvwalk_dev(c._h, d.res.data_ptr(), d.opt.data_ptr(), d.n, d.max_id, d.idx.data_ptr(),
                                  d.seg_sid.data_ptr(), d.seg_start.data_ptr(), d.nseg.data_ptr(),
                                  d.state.t.data_ptr(), d.place.t.data_ptr(), d.stop.t.data_ptr(),
                                  d.work.t.data_ptr(), d.wb, own.cuda_stream) == EIO
    c.close()
    stream_wait(handle)                                     # the stall and what was queued behind it end
    own.synchronize()
    assert untouched(got, b) and untouched(got2, b)
    assert (d.place.all == SENT).all().item() and (d.stop.all == SENT).all().item() and (d.work.all == SENT).all().item()
    assert d.state.numpy(RCV_STATE_DTYPE).tobytes() == b["state"].tobytes()
    with gpu.Context(0) as fresh:
        fresh.wait_limit = 5_000_000
        rc, got = host_call(L, fresh, b)
        assert rc == 0
        host_check(got, b)


# ---- error returns -------------------------------------------------------------------------------------
def test_error_returns(gpu, ctx):
    from mtcp_amd._lib import lib
    L = lib()
    rng = np.random.default_rng(48)
    b = rg.batch(rng, lens_for(rng, 600, 20), extra=20)
    expect(b)
    n, max_id = len(b["res"]), b["max_id"]
    d = Call(gpu, b)
    room = {k: Guarded(v.numel() + 64) for k, v in (("res", d.res), ("opt", d.opt), ("idx", d.idx),
                                                     ("seg_sid", d.seg_sid), ("seg_start", d.seg_start),
                                                     ("nseg", d.nseg))}
    p = lambda t, off=0: t.data_ptr() + off
    big = (1 << 26) + 1

    def dev(c=ctx._h, r=p(d.res), o=p(d.opt), n_=n, mx=max_id, i=p(d.idx), ss=p(d.seg_sid), st=p(d.seg_start),
            ns=p(d.nseg), s=p(d.state.t), pl=p(d.place.t), sp=p(d.stop.t), w=p(d.work.t), wbytes=d.wb):
        return L.mtcp_gpu_rcvwalk_dev(c, r, o, n_, mx, i, ss, st, ns, s, pl, sp, w, wbytes, None)

    bad = {
        "ctx NULL": dev(c=None), "res NULL": dev(r=None), "idx NULL": dev(i=None), "seg_sid NULL": dev(ss=None),
        "seg_start NULL": dev(st=None), "nseg NULL": dev(ns=None), "state NULL": dev(s=None),
        "place NULL": dev(pl=None), "seg_stop NULL": dev(sp=None), "work NULL": dev(w=None),
        "res misaligned": dev(r=p(room["res"].t, 4)), "opt misaligned": dev(o=p(room["opt"].t, 8)),
        "idx misaligned": dev(i=p(room["idx"].t, 2)), "seg_sid misaligned": dev(ss=p(room["seg_sid"].t, 1)),
        "seg_start misaligned": dev(st=p(room["seg_start"].t, 3)), "nseg misaligned": dev(ns=p(room["nseg"].t, 2)),
        "state misaligned": dev(s=p(d.state.t, 32)), "state misaligned by 16": dev(s=p(d.state.t, 16)),
        "place misaligned": dev(pl=p(d.place.t, 8)), "seg_stop misaligned": dev(sp=p(d.stop.t, 2)),
        "work misaligned": dev(w=p(d.work.t, 8)), "work too small": dev(wbytes=d.wb - 1), "no work bytes": dev(wbytes=0),
        "n too large": dev(n_=big), "max_id too large": dev(mx=MAX_ID + 1), "max_id is NONE": dev(mx=NONE),
    }
    with gpu.Context(0, compact=True) as cc:
        bad["compact context"] = dev(c=cc._h)
        res, opt = np.ascontiguousarray(b["res"]), np.ascontiguousarray(b["opt"])
        idx, seg_sid, seg_start = b["group"]
        nseg = np.array([len(seg_sid)], np.uint32)
        h_state = b["state"].copy()
        h_place, h_stop = np.full(16 * n, SENT, np.uint8), np.full(n, SENT32, np.uint32)

        def host(c=ctx._h, r=res.ctypes.data, o=opt.ctypes.data, n_=n, mx=max_id, i=idx.ctypes.data,
                 ss=seg_sid.ctypes.data, st=seg_start.ctypes.data, ns=nseg.ctypes.data, s=h_state.ctypes.data,
                 pl=h_place.ctypes.data, sp=h_stop.ctypes.data):
            return L.mtcp_gpu_rcvwalk(c, r, o, n_, mx, i, ss, st, ns, s, pl, sp)

        bad.update({"host: ctx NULL": host(c=None), "host: res NULL": host(r=None), "host: idx NULL": host(i=None),
                    "host: seg_sid NULL": host(ss=None), "host: seg_start NULL": host(st=None),
                    "host: nseg NULL": host(ns=None), "host: state NULL": host(s=None),
                    "host: place NULL": host(pl=None), "host: seg_stop NULL": host(sp=None),
                    "host: n too large": host(n_=big), "host: max_id too large": host(mx=MAX_ID + 1),
                    "host: compact context": host(c=cc._h)})
    assert {k: v for k, v in bad.items() if v != EINVAL} == {}
    assert dev(n_=0) == 0 and host(n_=0) == 0
    assert dev(n_=0, r=None, o=None, i=None, ss=None, st=None, ns=None, s=None, pl=None, sp=None, w=None, wbytes=0) == 0
    torch.cuda.synchronize()
    for g in (d.place, d.stop, d.work):                     # none of these wrote anything
        assert (g.all == SENT).all().item()
    assert d.state.numpy(RCV_STATE_DTYPE).tobytes() == b["state"].tobytes() and d.state.guard_intact()
    assert (h_place == SENT).all() and (h_stop == SENT32).all() and h_state.tobytes() == b["state"].tobytes()
    assert dev() == 0 and host() == 0                       # and the same arguments, valid, work
    torch.cuda.synchronize()
    d.check(b["want"], "after the refused calls")
    host_check((h_place.view(RCV_PLACE_DTYPE), h_state, h_stop), b)
    assert dev(o=None) == 0                                 # d_opt may be NULL
    torch.cuda.synchronize()
