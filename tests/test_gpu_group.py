"""The group step on the GPU (include/mtcp_gpu_group.h, mtcp_amd/csrc/
group_kernels.hpp): every output of every case is compared with
tests/group_model.py; none is sampled.

Guard regions sit behind every output, the workspace is exactly sized and
pre-filled with 0xA5, and the table's entries past m and m + 1 must keep their
sentinel.  Batch sizes around the wave and the tile, the shapes that show a
lost order, every max_id around every power of two (pass counts, digit
widths, the MISS / NONE mapping), purity, the chain rx + update + lookup +
group on one stream against the oracle's records, a captured graph replayed,
one 1 M-record batch, the host calls (unbounded, bounded, behind a stalled GPU)
and the error returns."""
import time

import numpy as np
import pytest

import oracle
from mtcp_amd import pktgen
from tests import flowtab_model as fm
from tests import group_model as gm

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EINVAL, EIO, ETIMEDOUT = -22, -5, -110
GUARD = 4096                       # bytes behind every device output
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
def T(gpu):
    return gpu.Context.group_tile()


def to_dev(a: np.ndarray):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(DEV)


class Guarded:
    """`nbytes` of device memory filled with `fill` and a guard region of SENT behind it."""

    def __init__(self, nbytes, fill=SENT):
        self.nbytes = nbytes
        self.all = torch.full((nbytes + GUARD,), SENT, dtype=torch.uint8, device=DEV)
        self.t = self.all[:nbytes]
        if isinstance(fill, np.ndarray):
            self.t.copy_(torch.from_numpy(fill).to(DEV))
        elif fill != SENT:
            self.t.fill_(fill)

    def guard_intact(self):
        return bool((self.all[self.nbytes:] == SENT).all().item())

    def numpy(self, dtype=np.uint32):
        return self.t.cpu().numpy().view(dtype)


class Outputs:
    """The four outputs and the exactly sized workspace of one call on n records."""

    def __init__(self, gpu, n, max_id, work_fill=SENT):
        self.n = n
        self.idx, self.seg_sid = Guarded(4 * n), Guarded(4 * n)
        self.seg_start, self.nseg = Guarded(4 * n + 4), Guarded(4)
        self.wb = gpu.Context.group_work_bytes(n, max_id)
        assert self.wb > 0
        self.work = Guarded(self.wb, work_fill)

    def call(self, ctx, d_sid, max_id, stream=None):
        ctx.group_dev(d_sid, self.n, max_id, self.idx.t, self.seg_sid.t, self.seg_start.t, self.nseg.t,
                      self.work.t, stream=stream)

    def raw(self):
        """The outputs' bytes as they are (sentinels included)."""
        return tuple(g.numpy().copy() for g in (self.idx, self.seg_sid, self.seg_start, self.nseg))

    def reset(self):
        for g in (self.idx, self.seg_sid, self.seg_start, self.nseg):
            g.t.fill_(SENT)

    def check(self, want, what=""):
        """Guards intact, (idx, seg_sid, seg_start) equal to `want`, nothing written past m and m + 1."""
        for name in ("idx", "seg_sid", "seg_start", "nseg", "work"):
            assert getattr(self, name).guard_intact(), f"{what}: bytes behind {name} were written"
        idx, seg_sid, seg_start, nseg = self.raw()
        w_idx, w_sid, w_start = want
        m = int(nseg[0])
        assert m == len(w_sid), f"{what}: m = {m}, want {len(w_sid)}"
        bad = np.nonzero(idx != w_idx)[0]
        assert len(bad) == 0, f"{what}: {len(bad)} of {self.n} indices differ, first at {bad[0]}: " \
                              f"{idx[bad[0]]} want {w_idx[bad[0]]}"
        assert np.array_equal(seg_sid[:m], w_sid), what
        assert np.array_equal(seg_start[:m + 1], w_start), what
        assert (seg_sid[m:] == SENT32).all() and (seg_start[m + 1:] == SENT32).all(), \
            f"{what}: table entries past m were written"


def run(gpu, ctx, sid, max_id, what="", work_fill=SENT):
    sid = np.ascontiguousarray(sid, dtype=np.uint32)
    out = Outputs(gpu, len(sid), max_id, work_fill)
    out.call(ctx, to_dev(sid), max_id)
    torch.cuda.synchronize()
    out.check(gm.group(sid, max_id), what)
    return out


def mixed(rng, n, max_id):
    """Every class: streams (a few crowded, many sparse), MISS, NONE, values above max_id."""
    sid = rng.integers(0, max_id + 1, n, dtype=np.uint64)
    r = rng.random(n)
    sid = np.where(r < 0.3, rng.integers(0, min(max_id, 7) + 1, n, dtype=np.uint64), sid)
    sid = np.where(r > 0.94, MISS, sid)
    sid = np.where(r > 0.96, NONE, sid)
    sid = np.where(r > 0.98, max_id + 1 + rng.integers(0, 9, n, dtype=np.uint64), sid)
    return sid.astype(np.uint32)


# ---- batch sizes ------------------------------------------------------------------------------
@pytest.mark.parametrize("tiles,plus", [(0, 1), (0, 2), (0, 63), (0, 64), (0, 65), (1, -1), (1, 0), (1, 1), (2, 5),
                                        (17, 5)])
def test_batch_sizes_with_every_class(gpu, ctx, T, tiles, plus):
    n = tiles * T + plus
    max_id = 1000
    rng = np.random.default_rng(n)
    if n <= 2:                                              # too few records for every class at once: each in turn
        pool = [5, MISS, NONE, max_id + 1, max_id, 0]
        for k in range(len(pool)):
            run(gpu, ctx, (pool[k:] + pool[:k])[:n], max_id, f"n = {n}, rotation {k}")
        return
    sid = mixed(rng, n, max_id)
    sid[:4] = [MISS, NONE, max_id + 1, max_id]
    sid[-1] = 0
    run(gpu, ctx, sid, max_id, f"n = {n}")
    for special in (MISS, NONE):
        assert (sid == special).any()
    assert ((sid > max_id) & (sid < MISS)).any() and (sid <= max_id).any()


# ---- stability and shape --------------------------------------------------------------------
@pytest.mark.parametrize("which", ["65", "T", "2T+5"])
def test_stability_and_shape(gpu, ctx, T, which):
    n = {"65": 65, "T": T, "2T+5": 2 * T + 5}[which]
    ar = np.arange(n, dtype=np.uint32)
    out = run(gpu, ctx, np.full(n, 9, np.uint32), 20, "one stream")
    idx, seg_sid, seg_start, nseg = out.raw()
    assert nseg[0] == 1 and np.array_equal(idx, ar) and seg_sid[0] == 9 and seg_start[:2].tolist() == [0, n]
    out = run(gpu, ctx, ar[::-1], n - 1, "n distinct ids, descending")
    idx, seg_sid, seg_start, nseg = out.raw()
    assert nseg[0] == n and np.array_equal(idx, ar[::-1]) and np.array_equal(seg_sid, ar)
    out = run(gpu, ctx, np.where(ar % 2 == 0, 300, 2).astype(np.uint32), 300, "two ids alternating")
    idx = out.raw()[0]
    assert np.array_equal(idx[:n // 2], ar[1::2]) and np.array_equal(idx[n // 2:], ar[0::2])
    sid = np.full(n, 70000, np.uint32)
    sid[-1] = 3
    out = run(gpu, ctx, sid, 70000, "one id holds n - 1 records, another the last")
    assert out.raw()[0][0] == n - 1
    out = run(gpu, ctx, np.full(n, MISS, np.uint32), 5, "only MISS")
    assert out.raw()[1][0] == MISS and out.raw()[3][0] == 1
    out = run(gpu, ctx, np.full(n, NONE, np.uint32), 5, "only NONE")
    assert out.raw()[1][0] == NONE and out.raw()[3][0] == 1
    out = run(gpu, ctx, np.full(n, 6, np.uint32), 5, "only values above max_id")
    assert out.raw()[1][0] == NONE and np.array_equal(out.raw()[0], ar)


# ---- digit edges ------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(1, 33))
def test_digit_edges(gpu, ctx, T, k):
    """max_id around 2^k: a dropped top digit, an off-by-one pass count, a
    MISS / NONE mapping that collides with a real id.  About 300 records per
    case as one workgroup, and the same values again above one tile (the
    launches per pass)."""
    rng = np.random.default_rng(1000 + k)
    for max_id in sorted({min(v, MAX_ID) for v in (2 ** k - 2, 2 ** k - 1, 2 ** k)}):
        pool = [0, 1, 2 ** (k - 1) - 1, 2 ** (k - 1), max_id - 1, max_id, max_id + 1, MISS, NONE]
        pool = np.array([min(max(v, 0), 0xFFFFFFFF) for v in pool], dtype=np.uint32)
        for n in (300, T + 300):
            sid = pool[rng.integers(0, len(pool), n)]
            sid[:len(pool)] = pool[::-1]
            run(gpu, ctx, sid, max_id, f"k = {k}, max_id = {max_id:#x}, n = {n}")


# ---- purity ------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["T", "2T+5"])
def test_purity(gpu, ctx, T, which):
    n = {"T": T, "2T+5": 2 * T + 5}[which]
    rng = np.random.default_rng(21)
    max_id = 1 << 20                                        # 21 key bits: three passes, both index arrays
    sid = mixed(rng, n, max_id)
    wb = gpu.Context.group_work_bytes(n, max_id)
    fills = [SENT, 0, 0xFF, rng.integers(0, 256, wb, dtype=np.uint8)]
    seen = [run(gpu, ctx, sid, max_id, f"workspace fill {i}", f).raw() for i, f in enumerate(fills)]
    for other in seen[1:]:
        for a, b in zip(seen[0], other):
            assert a.tobytes() == b.tobytes()


# ---- behind rx and lookup -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def rx_batch():
    """65 536 generated bimodal frames, the oracle's records of them, the
    entries of the TCP_OK packets at even indices (id = packet index), the
    model's answers with all entries and with those of id < 32 768 only."""
    n, seed = 65536, 31
    desc, nbytes = pktgen.layout(n, "bimodal", 6, seed)
    buf = np.zeros((nbytes + 63) & ~63, np.uint8)
    oracle.pktgen(buf, desc, 6, seed, 0)
    want = oracle.rx_chunk(buf, desc, 6, None)
    pick = np.nonzero((want["verdict"] == 0) & (np.arange(n) % 2 == 0))[0]
    ent = fm.entries(fm.record_keys(want[pick]), pick.astype(np.uint32))
    answers = []
    for part in (ent, ent[ent["id"] < 32768]):
        model = fm.FlowTable()
        model.update(ins=part)
        answers.append(model.lookup(want))
    ok = want["verdict"] == 0
    assert (answers[0][ok] < MISS).sum() >= ok.sum() // 4 and (answers[0][ok] == MISS).sum() >= ok.sum() // 4
    assert (answers[0][~ok] == NONE).all() and not np.array_equal(answers[0], answers[1])
    return buf, desc, want, ent, answers


def check_slices(want, ent, ans, idx, seg_sid, seg_start):
    """Every stream's slice holds exactly its 4-tuple's TCP_OK packets, ascending."""
    keys = fm.record_keys(want)
    ok = want["verdict"] == 0
    by_key = {}
    for i in np.nonzero(ok)[0]:
        by_key.setdefault(keys[i].tobytes(), []).append(int(i))
    key_of_id = {int(e["id"]): fm.entry_key(e) for e in ent}
    streams = 0
    for j, s in enumerate(int(x) for x in seg_sid):
        pk = idx[seg_start[j]:seg_start[j + 1]]
        assert (np.diff(pk.astype(np.int64)) > 0).all(), s
        if s <= 65535:
            assert pk.tolist() == by_key[key_of_id[s]], s
            streams += 1
        elif s == MISS:
            assert ok[pk].all() and (ans[pk] == MISS).all() and len(pk) == (ans == MISS).sum()
        else:
            assert s == NONE and np.array_equal(pk, np.nonzero(~ok)[0])
    assert streams == len(np.unique(ans[ans <= 65535])) > 1000


def test_group_behind_rx_and_lookup_on_one_stream(gpu, rx_batch):
    buf, desc, want, ent, answers = rx_batch
    n, max_id, ans = len(desc), len(desc) - 1, answers[0]
    d_buf, d_desc, d_ent = to_dev(buf), to_dev(desc), to_dev(ent)
    d_res = torch.zeros(n * 40, dtype=torch.uint8, device=DEV)
    sid = Guarded(4 * n)
    out = Outputs(gpu, n, max_id)
    st = torch.cuda.Stream(device=DEV)
    with gpu.Context(0) as c, gpu.FlowTable(c, 17) as tab:
        c.rx_chunk_dev(d_buf, d_desc, n, 6, d_res, stream=st)
        tab.update_dev(None, 0, d_ent, len(ent), stream=st)
        tab.lookup_dev(d_res, n, sid.t, None, stream=st)
        out.call(c, sid.t, max_id, stream=st)
        st.synchronize()
    assert sid.guard_intact()
    assert d_res.cpu().numpy().tobytes() == want.tobytes()
    assert np.array_equal(sid.numpy(), ans)
    out.check(gm.group(ans, max_id), "behind rx and lookup")
    idx, seg_sid, seg_start, nseg = out.raw()
    m = int(nseg[0])
    check_slices(want, ent, ans, idx, seg_sid[:m], seg_start[:m + 1])


def test_captured_chain_replay(gpu, rx_batch):
    """rx, lookup and group captured once (a linear chain) and replayed twice
    on fresh inputs: the table holds all entries at the first replay and half
    of them at the second (the updates run outside the graph)."""
    buf, desc, want, ent, answers = rx_batch
    n, max_id = len(desc), len(desc) - 1
    late = ent[ent["id"] >= 32768]
    d_buf, d_desc, d_ent, d_late = to_dev(buf), to_dev(desc), to_dev(ent), to_dev(late)
    d_res = torch.zeros(n * 40, dtype=torch.uint8, device=DEV)
    sid = Guarded(4 * n)
    out = Outputs(gpu, n, max_id)
    st = torch.cuda.Stream(device=DEV)
    with gpu.Context(0) as c, gpu.FlowTable(c, 17) as tab:
        def launch():
            c.rx_chunk_dev(d_buf, d_desc, n, 6, d_res, stream=st)
            tab.lookup_dev(d_res, n, sid.t, None, stream=st)
            out.call(c, sid.t, max_id, stream=st)

        tab.update_dev(None, 0, d_ent, len(ent), stream=st)
        launch()                                            # kernels loaded before the capture
        st.synchronize()
        out.check(gm.group(answers[0], max_id), "before the capture")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            launch()
        for rep, ans in enumerate(answers):
            if rep == 1:
                tab.update_dev(d_late, len(late), None, 0, stream=st)
                st.synchronize()
            sid.t.fill_(SENT)
            out.reset()
            out.work.t.fill_(rep)
            d_res.zero_()
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert sid.guard_intact() and np.array_equal(sid.numpy(), ans)
            out.check(gm.group(ans, max_id), f"replay {rep}")
        del g


# ---- full size ------------------------------------------------------------------------------
def test_one_million_records_of_65536_streams(gpu, ctx):
    rng = np.random.default_rng(22)
    n, max_id = 1 << 20, 65535
    sid = rng.integers(0, max_id + 1, n, dtype=np.uint64)
    r = rng.random(n)
    sid = np.where(r < 0.05, MISS, np.where(r < 0.15, NONE, sid)).astype(np.uint32)
    sid[12345] = max_id + 1                                 # a caller's garbage
    out = run(gpu, ctx, sid, max_id, "1 M records")
    assert out.raw()[3][0] == max_id + 3                    # every stream, MISS and NONE


# ---- host calls -----------------------------------------------------------------------------
def host_call(L, c, sid, max_id):
    n = len(sid)
    idx, seg_sid = np.full(n, SENT32, np.uint32), np.full(n, SENT32, np.uint32)
    seg_start, nseg = np.full(n + 1, SENT32, np.uint32), np.full(1, SENT32, np.uint32)
    rc = L.mtcp_gpu_group(c._h, sid.ctypes.data, n, max_id, idx.ctypes.data, seg_sid.ctypes.data,
                          seg_start.ctypes.data, nseg.ctypes.data)
    return rc, (idx, seg_sid, seg_start, nseg)


def host_check(got, want, what=""):
    idx, seg_sid, seg_start, nseg = got
    m = int(nseg[0])
    assert m == len(want[1]), what
    assert np.array_equal(idx, want[0]) and np.array_equal(seg_sid[:m], want[1]), what
    assert np.array_equal(seg_start[:m + 1], want[2]), what
    assert (seg_sid[m:] == SENT32).all() and (seg_start[m + 1:] == SENT32).all(), what


@pytest.mark.parametrize("limit", [0, 5_000_000], ids=["unbounded", "bounded"])
def test_host_calls(gpu, T, limit):
    from mtcp_amd._lib import lib
    L = lib()
    rng = np.random.default_rng(23)
    with gpu.Context(0) as c:
        if limit:
            c.wait_limit = limit
        for n, max_id in ((3 * T + 7, 70000), (3000, 1 << 24), (5, 0), (T + 1, 200)):   # the staging reused by smaller calls
            sid = mixed(rng, n, max_id)
            want = gm.group(sid, max_id)
            rc, got = host_call(L, c, sid, max_id)
            assert rc == 0
            host_check(got, want, f"n = {n}")
            idx, seg_sid, seg_start = c.group(sid, max_id)                              # the Python view
            assert np.array_equal(idx, want[0]) and np.array_equal(seg_sid, want[1])
            assert np.array_equal(seg_start, want[2])


def test_host_call_gives_up_at_the_limit(gpu, T):
    """The stalled-GPU pattern of tests/test_gpu_bounded.py (its helpers, its
    stall and limit values), as tests/test_gpu_flowtab.py does it: ETIMEDOUT
    within the limit, the outputs keep their sentinel right after the call and
    after the stall has ended, the context answers EIO, a fresh context gives
    the model's answers."""
    from mtcp_amd._lib import lib
    from tests.test_gpu_bounded import LIMIT_US, SLACK_S, STALL_US, stall_lib, stream_busy, stream_wait
    L, S = lib(), stall_lib()
    rng = np.random.default_rng(24)
    n, max_id = T + 100, 5000
    sid = mixed(rng, n, max_id)
    want = gm.group(sid, max_id)
    untouched = lambda got: all((a == SENT32).all() for a in got)

    c = gpu.Context(0)
    handle = c.stream
    rc, got = host_call(L, c, sid, max_id)                  # unbounded: stage sized, kernels loaded
    assert rc == 0
    host_check(got, want)
    c.wait_limit = LIMIT_US
    rc, got = host_call(L, c, sid, max_id)                  # bounded, no stall: the bounce buffers sized
    assert rc == 0
    host_check(got, want)
    assert S.mtcp_gpu_debug_stall(c._h, STALL_US) == 0
    t0 = time.monotonic()
    rc, got = host_call(L, c, sid, max_id)
    dt = time.monotonic() - t0
    assert rc == ETIMEDOUT, rc
    assert dt < LIMIT_US / 1e6 + SLACK_S, dt
    assert stream_busy(handle)
    assert untouched(got)
    assert L.mtcp_gpu_sync(c._h) == EIO
    rc2, got2 = host_call(L, c, sid, max_id)
    assert rc2 == EIO and untouched(got2)
    own = torch.cuda.Stream(device=DEV)
    dout = Outputs(gpu, n, max_id)
    assert L.mtcp_gpu_group_dev(c._h, to_dev(sid).data_ptr(), n, max_id, dout.idx.t.data_ptr(),
                                dout.seg_sid.t.data_ptr(), dout.seg_start.t.data_ptr(), dout.nseg.t.data_ptr(),
                                dout.work.t.data_ptr(), dout.wb, own.cuda_stream) == EIO
    c.close()
    stream_wait(handle)                                     # the stall and what was queued behind it end
    own.synchronize()
    assert untouched(got) and untouched(got2)
    assert all((g.all == SENT).all().item() for g in (dout.idx, dout.seg_sid, dout.seg_start, dout.nseg, dout.work))
    with gpu.Context(0) as fresh:
        fresh.wait_limit = 5_000_000
        rc, got = host_call(L, fresh, sid, max_id)
        assert rc == 0
        host_check(got, want)


# ---- error returns ---------------------------------------------------------------------------
def test_error_returns(gpu, ctx, T):
    from mtcp_amd._lib import lib
    L = lib()
    rng = np.random.default_rng(25)
    n, max_id = T + 64, 500
    sid = mixed(rng, n, max_id)
    d_sid = Guarded(4 * n + 8)
    d_sid.t[:4 * n] = to_dev(sid)
    out = Outputs(gpu, n + 2, max_id)                       # room for the misaligned variants
    wb = gpu.Context.group_work_bytes(n, max_id)
    p = lambda g, off=0: g.t.data_ptr() + off
    big = (1 << 26) + 1

    def dev(c=ctx._h, s=p(d_sid), n_=n, mx=max_id, i=p(out.idx), ss=p(out.seg_sid), st=p(out.seg_start),
            ns=p(out.nseg), w=p(out.work), wbytes=wb):
        return L.mtcp_gpu_group_dev(c, s, n_, mx, i, ss, st, ns, w, wbytes, None)

    bad = {
        "ctx NULL": dev(c=None), "sid NULL": dev(s=None), "idx NULL": dev(i=None), "seg_sid NULL": dev(ss=None),
        "seg_start NULL": dev(st=None), "nseg NULL": dev(ns=None), "work NULL": dev(w=None),
        "sid misaligned": dev(s=p(d_sid, 2)), "idx misaligned": dev(i=p(out.idx, 1)),
        "seg_sid misaligned": dev(ss=p(out.seg_sid, 2)), "seg_start misaligned": dev(st=p(out.seg_start, 3)),
        "nseg misaligned": dev(ns=p(out.nseg, 2)), "work misaligned": dev(w=p(out.work, 8)),
        "work too small": dev(wbytes=wb - 1), "no work bytes": dev(wbytes=0),
        "n too large": dev(n_=big), "max_id too large": dev(mx=MAX_ID + 1), "max_id is NONE": dev(mx=NONE),
        "one tile, work NULL": dev(n_=64, w=None), "one tile, work misaligned": dev(n_=64, w=p(out.work, 4)),
    }
    assert {k: v for k, v in bad.items() if v != EINVAL} == {}
    assert dev(n_=0) == 0 and dev(n_=0, s=None, i=None, ss=None, st=None, ns=None, w=None, wbytes=0) == 0
    # the host call
    h = [np.full(n + 1, SENT32, np.uint32) for _ in range(4)]

    def host(c=ctx._h, s=sid.ctypes.data, n_=n, mx=max_id, i=h[0].ctypes.data, ss=h[1].ctypes.data,
             st=h[2].ctypes.data, ns=h[3].ctypes.data):
        return L.mtcp_gpu_group(c, s, n_, mx, i, ss, st, ns)

    bad = {"ctx NULL": host(c=None), "sid NULL": host(s=None), "idx NULL": host(i=None),
           "seg_sid NULL": host(ss=None), "seg_start NULL": host(st=None), "nseg NULL": host(ns=None),
           "n too large": host(n_=big), "max_id too large": host(mx=MAX_ID + 1)}
    assert {k: v for k, v in bad.items() if v != EINVAL} == {}
    assert host(n_=0) == 0 and host(n_=0, s=None, i=None, ss=None, st=None, ns=None) == 0
    torch.cuda.synchronize()
    for g in (out.idx, out.seg_sid, out.seg_start, out.nseg, out.work):     # none of these wrote anything
        assert (g.all == SENT).all().item()
    assert all((a == SENT32).all() for a in h)
    assert dev() == 0 and host() == 0                       # and the same arguments, valid, work
    torch.cuda.synchronize()
    want = gm.group(sid, max_id)
    m = len(want[1])
    assert out.nseg.numpy()[0] == m == h[3][0]
    assert np.array_equal(out.idx.numpy()[:n], want[0]) and np.array_equal(h[0][:n], want[0])
    assert np.array_equal(out.seg_sid.numpy()[:m], want[1]) and np.array_equal(h[1][:m], want[1])
    assert np.array_equal(out.seg_start.numpy()[:m + 1], want[2]) and np.array_equal(h[2][:m + 1], want[2])
