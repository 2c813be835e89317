"""The steer step on the GPU (include/mtcp_gpu_steer.h, mtcp_amd/csrc/
steer_kernels.hpp): every idx, start and gathered descriptor is compared
exactly against tests/steer_model.py.

Hand-made records over a Q x n grid (both record sizes, both flag values),
skewed destinations, guard regions behind every output and the workspace,
the descriptor gather, steering behind the rx launch on one stream against
the oracle's records, a captured graph replayed, determinism, the host call
(bounded and behind a stalled GPU) and the error returns."""
import time

import numpy as np
import pytest

import oracle
from mtcp_amd import DESC_DTYPE, RESULT16_DTYPE, RESULT_DTYPE, STEER_DROP_BAD, compact_of, pktgen
from tests import steer_model as sm

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EINVAL, EIO, ETIMEDOUT = -22, -5, -110
GUARD = 4096                       # bytes behind every device array
SENT = 0xA5
V_TCP_OK = 0
QS = (1, 2, 3, 7, 16, 17, 64, 128)


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")
    from mtcp_amd import gpu as g
    return g


@pytest.fixture(scope="module")
def T(gpu):
    t = gpu.Context.steer_tile()
    assert t >= 256 and t % 64 == 0
    return t


@pytest.fixture(scope="module")
def ctxs(gpu):
    """One context per (Q, compact), opened on first use, closed at the end."""
    made = {}

    def get(Q, compact=False):
        if (Q, compact) not in made:
            made[(Q, compact)] = gpu.Context(0, rss=True, rss_queues=Q, compact=compact)
        return made[(Q, compact)]

    yield get
    for c in made.values():
        c.close()


def sizes(T):
    return (1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 5, 257 * T + 5)


_records = {}


def random_records(dtype, n, seed=0):
    """Every byte random (rss_queue covers 0..255); seven records of eight
    get their verdict folded into 0..15, the eighth keeps a value up to 255.
    Cached: the large batches are generated once and never changed."""
    key = (dtype.itemsize, n, seed)
    if key not in _records:
        rng = np.random.default_rng(1000 * seed + n % 9973 + dtype.itemsize)
        r = rng.integers(0, 256, n * dtype.itemsize, dtype=np.uint8).view(dtype)
        fold = np.arange(n) % 8 != 7
        r["verdict"][fold] &= 15
        r.flags.writeable = False
        _records[key] = r
    return _records[key]


def to_dev(a: np.ndarray):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(DEV)


class Guarded:
    """`nbytes` of device memory filled with SENT and a guard region behind it."""

    def __init__(self, nbytes):
        self.nbytes = nbytes
        self.all = torch.full((nbytes + GUARD,), SENT, dtype=torch.uint8, device=DEV)
        self.t = self.all[:nbytes]

    def guard_intact(self):
        return bool((self.all[self.nbytes:] == SENT).all().item())

    def numpy(self, dtype):
        return self.t.cpu().numpy().view(dtype)


def run_steer(ctx, res: np.ndarray, flags=0, desc: np.ndarray | None = None, stream=None):
    """steer_dev over `res` with guarded outputs and a workspace of exactly
    steer_work_bytes(n); returns (idx, start, desc_out or None) after checking
    every guard."""
    n, Q = len(res), ctx.num_queues
    wb = ctx.steer_work_bytes(n)
    assert wb > 0
    idx, start, work = Guarded(4 * n), Guarded(4 * (Q + 2)), Guarded(wb)
    d_res = to_dev(res)
    d_desc = dout = None
    if desc is not None:
        d_desc, dout = to_dev(desc), Guarded(8 * n)
    ctx.steer_dev(d_res, n, idx.t, start.t, work.t, flags=flags, desc=d_desc,
                  desc_out=None if dout is None else dout.t, stream=stream)
    torch.cuda.synchronize()
    for name, g in (("idx", idx), ("start", start), ("work", work), ("desc_out", dout)):
        assert g is None or g.guard_intact(), f"{name}: bytes behind the array were written"
    return idx.numpy(np.uint32), start.numpy(np.uint32), None if dout is None else dout.numpy(DESC_DTYPE)


def assert_model(res, Q, flags, idx, start, what=""):
    want_idx, want_start = sm.steer(res, Q, flags)
    assert np.array_equal(start, want_start), f"{what}: start {start} want {want_start}"
    bad = np.nonzero(idx != want_idx)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} idx differ, first at {bad[0]}: {idx[bad[0]]} want {want_idx[bad[0]]}"


def check(ctx, res, flags, what=""):
    idx, start, _ = run_steer(ctx, res, flags)
    assert_model(res, ctx.num_queues, flags, idx, start, what)
    return idx, start


# ---- hand-made records ----------------------------------------------------------
@pytest.mark.parametrize("ni", range(13))
@pytest.mark.parametrize("Q", QS)
def test_random_records_full_grid(ctxs, T, Q, ni):
    n = sizes(T)[ni]
    check(ctxs(Q), random_records(RESULT_DTYPE, n), 0, f"Q={Q} n={n}")


@pytest.mark.parametrize("k", range(13))
@pytest.mark.parametrize("compact,flags", [(False, STEER_DROP_BAD), (True, 0), (True, STEER_DROP_BAD)])
def test_random_records_diagonal(ctxs, T, compact, flags, k):
    n, Q = sizes(T)[k], QS[(k + 3 * int(compact) + flags) % len(QS)]
    dtype = RESULT16_DTYPE if compact else RESULT_DTYPE
    res = random_records(dtype, n, seed=1)
    check(ctxs(Q, compact), res, flags, f"compact={compact} flags={flags} Q={Q} n={n}")
    # random queue bytes are mostly >= Q: the same records with their queues folded into 0 .. Q + 1
    even = res.copy()
    even["rss_queue"] %= Q + 2
    check(ctxs(Q, compact), even, flags, f"folded queues, compact={compact} flags={flags} Q={Q} n={n}")
    if flags and n >= 255:                      # the flag matters for these records
        assert not np.array_equal(sm.dest(even, Q, 0), sm.dest(even, Q, flags))


def test_context_without_rss_has_one_queue(gpu, T):
    with gpu.Context(0) as ctx:
        assert ctx.num_queues == 1
        res = random_records(RESULT_DTYPE, T + 1, seed=2)
        _, start = check(ctx, res, STEER_DROP_BAD, "no RSS")
        assert len(start) == 3


# ---- skew -----------------------------------------------------------------------
def made(n, queue, verdict=0, dtype=RESULT_DTYPE):
    r = np.zeros(n, dtype)
    r["rss_queue"], r["verdict"] = queue, verdict
    return r


def test_skewed_destinations(ctxs, T):
    n = 3 * T + 5
    i = np.arange(n)
    c16, c128 = ctxs(16), ctxs(128)
    idx, start = check(c16, made(n, 3), 0, "one queue")
    assert np.array_equal(idx, i) and start[3] == 0 and start[4] == n
    idx, start = check(c16, made(n, 200), 0, "all rest")
    assert np.array_equal(idx, i) and start[16] == 0
    idx, start = check(c16, made(n, 2, verdict=9), STEER_DROP_BAD, "all dropped")
    assert np.array_equal(idx, i) and start[16] == 0
    check(c128, made(n, 128 - (i * 129) // n), 0, "descending")           # 128 (rest) down to 0
    check(c16, made(n, np.where(i % 2 == 0, 5, 16)), 0, "alternating queue / rest")
    check(c128, made(n, np.where(i % 2 == 0, 127, 0)), 0, "alternating 127 / 0")
    # one packet per list exactly at wave and tile boundaries, the others in queue 0
    q = np.zeros(T + 1, np.int64)
    q[[63, 64, T - 1, T]] = [1, 2, 3, 16]
    idx, start = check(c16, made(T + 1, q), 0, "boundaries")
    assert idx[start[1]] == 63 and idx[start[2]] == 64 and idx[start[3]] == T - 1 and idx[start[16]] == T
    # every wave meets all 128 queues (and the rest list) in its rounds
    check(c128, made(n, (i * 37) % 129), 0, "all destinations per wave")
    check(c128, made(n, i % 128), 0, "i mod 128")
    check(c128, made(T, (i[:T] * 37) % 129), STEER_DROP_BAD, "all destinations, one tile")


# ---- bounds -----------------------------------------------------------------------
@pytest.mark.parametrize("Q,nk", [(1, 8), (7, 9), (128, 10), (17, 11), (128, 12), (64, 4)])
def test_every_store_is_in_bounds_and_every_position_written(ctxs, T, Q, nk):
    """run_steer's guards (idx, start, desc_out, a workspace of exactly
    steer_work_bytes(n)) are intact, no position of idx keeps its sentinel,
    and idx is a permutation."""
    n = sizes(T)[nk]
    res = random_records(RESULT_DTYPE, n, seed=1)
    desc = np.zeros(n, DESC_DTYPE)
    desc["offset"], desc["len"] = np.arange(n), np.arange(n) % 1500
    idx, start, dout = run_steer(ctxs(Q), res, STEER_DROP_BAD, desc=desc)
    assert not (idx == 0xA5A5A5A5).any()
    assert np.array_equal(np.sort(idx), np.arange(n, dtype=np.uint32))
    assert start[0] == 0 and start[-1] == n and (np.diff(start.astype(np.int64)) >= 0).all()
    assert_model(res, Q, STEER_DROP_BAD, idx, start)
    assert dout.tobytes() == desc[idx].tobytes()


# ---- descriptors ------------------------------------------------------------------
@pytest.mark.parametrize("compact", [False, True])
def test_descriptor_gather(gpu, ctxs, T, compact):
    ctx = ctxs(5, compact)
    dtype = RESULT16_DTYPE if compact else RESULT_DTYPE
    for n in (65, T, 3 * T + 5):
        res = random_records(dtype, n, seed=4)
        rng = np.random.default_rng(n)
        desc = rng.integers(0, 256, 8 * n, dtype=np.uint8).view(DESC_DTYPE)
        idx, start, dout = run_steer(ctx, res, 0, desc=desc)
        assert_model(res, 5, 0, idx, start, f"gather n={n}")
        assert dout.tobytes() == desc[idx].tobytes()
        idx2, start2, none = run_steer(ctx, res, 0)             # both NULL: the same lists
        assert none is None and idx2.tobytes() == idx.tobytes() and start2.tobytes() == start.tobytes()
    # exactly one NULL
    from mtcp_amd._lib import MtcpGpuError
    n = 100
    d_res, d_desc = to_dev(random_records(dtype, n, seed=4)), to_dev(np.zeros(n, DESC_DTYPE))
    idx, start, work, dout = Guarded(4 * n), Guarded(28), Guarded(ctx.steer_work_bytes(n)), Guarded(8 * n)
    for kw in (dict(desc=d_desc), dict(desc_out=dout.t)):
        with pytest.raises(MtcpGpuError) as e:
            ctx.steer_dev(d_res, n, idx.t, start.t, work.t, **kw)
        assert e.value.code == EINVAL
    torch.cuda.synchronize()
    assert (idx.all == SENT).all().item() and (dout.all == SENT).all().item()


# ---- behind rx, end to end ------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed_batch(golden):
    """A generated bimodal batch of 5 000 frames followed by the golden rx
    frames, byte offsets (off_shift 0)."""
    n, seed = 5000, 23
    desc, nbytes = pktgen.layout(n, "bimodal", 0, seed)
    buf = np.zeros(nbytes, np.uint8)
    oracle.pktgen(buf, desc, 0, seed, 0)
    gd = golden.desc.copy()
    gd["offset"] += nbytes
    allbuf = np.concatenate([buf, golden.buf])
    pad = (-allbuf.nbytes) % 64
    if pad:
        allbuf = np.concatenate([allbuf, np.zeros(pad, np.uint8)])
    alldesc = np.concatenate([desc, gd])
    return allbuf, alldesc, to_dev(allbuf), to_dev(alldesc)


_oracle_records = {}


def oracle_records(mixed_batch, key, Q, endian):
    k = (key, Q, endian)
    if k not in _oracle_records:
        buf, desc = mixed_batch[0], mixed_batch[1]
        _oracle_records[k] = oracle.rx_chunk(buf, desc, 0, oracle.rss_cfg(key, Q, endian))
    return _oracle_records[k]


def rx_then_steer(ctx, mixed_batch, flags, stream):
    """rx_chunk_dev and steer_dev on `stream` with no sync between; returns a
    function that reads (idx, start, desc_out) back."""
    _, desc, d_buf, d_desc = mixed_batch
    n, Q = len(desc), ctx.num_queues
    d_res = torch.zeros(n * ctx.record_size, dtype=torch.uint8, device=DEV)
    idx, start, work, dout = Guarded(4 * n), Guarded(4 * (Q + 2)), Guarded(ctx.steer_work_bytes(n)), Guarded(8 * n)

    def launch():
        ctx.rx_chunk_dev(d_buf, d_desc, n, 0, d_res, stream=stream)
        ctx.steer_dev(d_res, n, idx.t, start.t, work.t, flags=flags, desc=d_desc, desc_out=dout.t, stream=stream)

    def read():
        stream.synchronize()
        assert idx.guard_intact() and start.guard_intact() and work.guard_intact() and dout.guard_intact()
        return idx.numpy(np.uint32), start.numpy(np.uint32), dout.numpy(DESC_DTYPE)

    return launch, read, (idx, start, dout)


def assert_flows_whole(want, idx, start):
    """Every TCP_OK 4-tuple: all its packets in one list, in ascending index."""
    n = len(want)
    list_of = np.zeros(n, np.int64)
    pos_of = np.zeros(n, np.int64)
    for l in range(len(start) - 1):
        list_of[idx[start[l]:start[l + 1]]] = l
    pos_of[idx] = np.arange(n)
    ok = np.nonzero(want["verdict"] == V_TCP_OK)[0]
    flows = {}
    for i in ok:
        flows.setdefault((int(want["saddr"][i]), int(want["daddr"][i]), int(want["sport"][i]),
                          int(want["dport"][i])), []).append(i)
    assert len(flows) > 100
    for members in flows.values():
        assert len({list_of[i] for i in members}) == 1
        p = pos_of[members]
        assert (np.diff(p) > 0).all()


@pytest.mark.parametrize("compact", [False, True], ids=["40B", "16B"])
@pytest.mark.parametrize("endian", [0, 1])
@pytest.mark.parametrize("Q", [1, 2, 5, 16])
def test_steer_behind_rx_equals_the_model_over_the_oracles_records(gpu, mixed_batch, Q, endian, compact):
    want = oracle_records(mixed_batch, oracle.KEY_MICROSOFT, Q, endian)
    desc = mixed_batch[1]
    st = torch.cuda.Stream(device=DEV)
    with gpu.Context(0, rss=True, rss_key=oracle.KEY_MICROSOFT, rss_queues=Q, rss_endian=bool(endian),
                     compact=compact) as ctx:
        for flags in (0, STEER_DROP_BAD):
            launch, read, _ = rx_then_steer(ctx, mixed_batch, flags, st)
            launch()
            idx, start, dout = read()
            model_in = compact_of(want) if compact else want
            assert_model(model_in, Q, flags, idx, start, f"Q={Q} endian={endian} flags={flags}")
            assert dout.tobytes() == desc[idx].tobytes()
            assert_flows_whole(want, idx, start)
    if Q == 16:
        assert (np.diff(start.astype(np.int64))[:16] > 0).all()      # every queue gets packets


@pytest.mark.parametrize("Q", [1, 8])
def test_degenerate_key(gpu, mixed_batch, Q):
    """The shipped 0x05 key (util/rss.c:84-90): its hash is byte-replicated and
    the same in both directions of a flow, yet it still spreads flows over the
    queues, so it runs with the default queue count and as the single-queue
    case; both directions of a flow land in one list."""
    want = oracle_records(mixed_batch, oracle.KEY_0X05, Q, 1)
    st = torch.cuda.Stream(device=DEV)
    with gpu.Context(0, rss=True, rss_queues=Q) as ctx:
        launch, read, _ = rx_then_steer(ctx, mixed_batch, 0, st)
        launch()
        idx, start, _ = read()
    assert_model(want, Q, 0, idx, start, "0x05 key")
    ok = want["verdict"] == V_TCP_OK
    h = want["rss_hash"][ok]
    assert ((h & 0xFF) * 0x01010101 == h).all()              # byte-replicated
    if Q == 1:
        assert start[1] == len(want) and np.array_equal(idx, np.arange(len(want)))
    assert_flows_whole(want, idx, start)


# ---- replay -------------------------------------------------------------------------
@pytest.mark.parametrize("compact", [False, True], ids=["40B", "16B"])
def test_captured_rx_and_steer_replay(gpu, mixed_batch, compact):
    Q = 16
    want = oracle_records(mixed_batch, oracle.KEY_MICROSOFT, Q, 0)
    st = torch.cuda.Stream(device=DEV)
    with gpu.Context(0, rss=True, rss_key=oracle.KEY_MICROSOFT, rss_queues=Q, rss_endian=False,
                     compact=compact) as ctx:
        launch, read, (idx_g, start_g, dout_g) = rx_then_steer(ctx, mixed_batch, STEER_DROP_BAD, st)
        launch()                                           # kernels loaded before the capture
        read()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            launch()
        seen = []
        for _ in range(2):
            for t in (idx_g, start_g, dout_g):
                t.t.fill_(SENT)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            idx, start, dout = read()
            assert_model(want, Q, STEER_DROP_BAD, idx, start, "replay")
            assert dout.tobytes() == mixed_batch[1][idx].tobytes()
            seen.append((idx.tobytes(), start.tobytes(), dout.tobytes()))
        assert seen[0] == seen[1]
        del g


# ---- determinism ------------------------------------------------------------------------
def test_two_runs_give_identical_bytes(ctxs, T):
    res = random_records(RESULT_DTYPE, 257 * T + 5)
    a = run_steer(ctxs(128), res, STEER_DROP_BAD)
    b = run_steer(ctxs(128), res, STEER_DROP_BAD)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ---- host call ------------------------------------------------------------------------
@pytest.mark.parametrize("compact,limit,nk", [(False, 0, 9), (False, 5_000_000, 10), (True, 0, 10),
                                              (True, 5_000_000, 5), (False, 0, 12), (False, 5_000_000, 12)])
def test_host_call(gpu, T, compact, limit, nk):
    n, Q = sizes(T)[nk], 7
    dtype = RESULT16_DTYPE if compact else RESULT_DTYPE
    res = random_records(dtype, n, seed=1)
    with gpu.Context(0, rss=True, rss_queues=Q, compact=compact) as ctx:
        if limit:
            ctx.wait_limit = limit
        for flags in (0, STEER_DROP_BAD):
            idx, start = ctx.steer(res, flags)
            assert_model(res, Q, flags, idx, start, f"host n={n} limit={limit}")
        idx, start = ctx.steer(res[:3], 0)                  # the staging reused by a smaller call
        assert_model(res[:3], Q, 0, idx, start)


def test_host_call_gives_up_at_the_limit(gpu, golden):
    """The stalled-GPU pattern of tests/test_gpu_bounded.py (its helpers, its
    stall and limit values): ETIMEDOUT within the limit, idx and start keep
    their sentinel right after the call and after the stall has ended, the
    context answers EIO, a fresh context gives the model's lists."""
    from mtcp_amd._lib import lib
    from tests.test_gpu_bounded import LIMIT_US, SLACK_S, STALL_US, stall_lib, stream_busy, stream_wait
    L, S = lib(), stall_lib()
    Q = golden.rss_num_queues
    res = np.ascontiguousarray(golden.expect)
    n = len(res)

    def call(ctx):
        idx = np.full(n, 0xA5A5A5A5, np.uint32)
        start = np.full(Q + 2, 0xA5A5A5A5, np.uint32)
        rc = L.mtcp_gpu_steer(ctx._h, res.ctypes.data, n, STEER_DROP_BAD, idx.ctypes.data, start.ctypes.data)
        return rc, idx, start

    ctx = gpu.Context(0, rss=True, rss_queues=Q)
    handle = ctx.stream
    rc, idx, start = call(ctx)                              # unbounded: stage sized, kernels loaded
    assert rc == 0
    assert_model(res, Q, STEER_DROP_BAD, idx, start, "before the stall")
    ctx.wait_limit = LIMIT_US
    assert S.mtcp_gpu_debug_stall(ctx._h, STALL_US) == 0
    t0 = time.monotonic()
    rc, idx, start = call(ctx)
    dt = time.monotonic() - t0
    assert rc == ETIMEDOUT, rc
    assert dt < LIMIT_US / 1e6 + SLACK_S, dt
    assert stream_busy(handle)
    assert (idx == 0xA5A5A5A5).all() and (start == 0xA5A5A5A5).all()
    assert L.mtcp_gpu_sync(ctx._h) == EIO
    rc2, idx2, start2 = call(ctx)
    assert rc2 == EIO and (idx2 == 0xA5A5A5A5).all() and (start2 == 0xA5A5A5A5).all()
    ctx.close()
    stream_wait(handle)                                     # the stall and what was queued behind it end
    assert (idx == 0xA5A5A5A5).all() and (start == 0xA5A5A5A5).all()
    with gpu.Context(0, rss=True, rss_queues=Q) as fresh:
        fresh.wait_limit = 5_000_000
        rc, idx, start = call(fresh)
        assert rc == 0
        assert_model(res, Q, STEER_DROP_BAD, idx, start, "fresh context")


# ---- error returns ------------------------------------------------------------------
def test_error_returns(gpu, T):
    from mtcp_amd._lib import lib
    L = lib()
    n = 3 * T + 5
    res = random_records(RESULT_DTYPE, n, seed=6)
    d_res = to_dev(res)
    d_desc = to_dev(np.zeros(n, DESC_DTYPE))
    with gpu.Context(0, rss=True, rss_queues=16) as ctx:
        Q = 16
        wb = ctx.steer_work_bytes(n)
        assert wb >= n and ctx.steer_work_bytes(sm.STEER_MAX_PKTS + 1) == 0
        assert L.mtcp_gpu_steer_work_bytes(None, n) == 0
        assert ctx.steer_work_bytes(sm.STEER_MAX_PKTS) > sm.STEER_MAX_PKTS
        idx, start, work, dout = Guarded(4 * n + 8), Guarded(4 * (Q + 2) + 8), Guarded(wb + 16), Guarded(8 * n + 8)
        h = ctx._h
        p = lambda t, off=0: t.data_ptr() + off

        def dev(ctx_h=h, res_p=p(d_res), n_=n, flags=0, idx_p=p(idx.t), start_p=p(start.t), desc_p=None,
                dout_p=None, work_p=p(work.t), wbytes=wb):
            return L.mtcp_gpu_steer_dev(ctx_h, res_p, n_, flags, idx_p, start_p, desc_p, dout_p, work_p, wbytes,
                                        None)

        bad = {
            "ctx NULL": dev(ctx_h=None), "res NULL": dev(res_p=None), "idx NULL": dev(idx_p=None),
            "start NULL": dev(start_p=None), "work NULL": dev(work_p=None),
            "res misaligned": dev(res_p=p(d_res, 4)), "idx misaligned": dev(idx_p=p(idx.t, 2)),
            "start misaligned": dev(start_p=p(start.t, 1)), "work misaligned": dev(work_p=p(work.t, 8)),
            "desc misaligned": dev(desc_p=p(d_desc, 4), dout_p=p(dout.t)),
            "desc_out misaligned": dev(desc_p=p(d_desc), dout_p=p(dout.t, 4)),
            "desc only": dev(desc_p=p(d_desc)), "desc_out only": dev(dout_p=p(dout.t)),
            "unknown flag": dev(flags=2), "unknown flags": dev(flags=0x80000001),
            "n too large": dev(n_=sm.STEER_MAX_PKTS + 1), "workspace too small": dev(wbytes=wb - 1),
        }
        assert {k: v for k, v in bad.items() if v != EINVAL} == {}
        assert dev(n_=0) == 0 and dev(n_=0, res_p=None, idx_p=None, start_p=None, work_p=None) == 0
        hidx, hstart = np.full(n, 0xA5A5A5A5, np.uint32), np.full(Q + 2, 0xA5A5A5A5, np.uint32)
        host = lambda **kw: L.mtcp_gpu_steer(kw.get("c", h), kw.get("r", res.ctypes.data), kw.get("n", n),
                                             kw.get("f", 0), kw.get("i", hidx.ctypes.data),
                                             kw.get("s", hstart.ctypes.data))
        assert host(c=None) == EINVAL and host(r=None) == EINVAL and host(i=None) == EINVAL
        assert host(s=None) == EINVAL and host(f=4) == EINVAL and host(n=sm.STEER_MAX_PKTS + 1) == EINVAL
        assert host(n=0) == 0
        torch.cuda.synchronize()
        for g in (idx, start, work, dout):
            assert (g.all == SENT).all().item()              # none of these calls wrote anything
        assert (hidx == 0xA5A5A5A5).all() and (hstart == 0xA5A5A5A5).all()
        assert dev() == 0                                    # and the same arguments, valid, work
        torch.cuda.synchronize()
        assert_model(res, Q, 0, idx.numpy(np.uint32)[:n], start.numpy(np.uint32)[:Q + 2])
    # Q above MTCP_GPU_STEER_MAX_QUEUES
    with gpu.Context(0, rss=True, rss_queues=129) as big:
        assert big.steer_work_bytes(n) == 0
        wk = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
        st = torch.zeros(4 * 131, dtype=torch.uint8, device=DEV)
        assert L.mtcp_gpu_steer_dev(big._h, p(d_res), n, 0, p(idx.t), p(st), None, None, p(wk), 1 << 20,
                                    None) == EINVAL
        assert L.mtcp_gpu_steer(big._h, res.ctypes.data, n, 0, hidx.ctypes.data, hstart.ctypes.data) == EINVAL


def test_abandoned_context_answers_eio_and_writes_nothing(gpu, golden):
    """A context abandoned by a bounded call (the stall pattern of
    tests/test_gpu_bounded.py): steer_dev and steer answer EIO, nothing is
    written."""
    from mtcp_amd._lib import lib
    from tests.test_gpu_bounded import LIMIT_US, STALL_US, stall_lib, stream_wait
    L, S = lib(), stall_lib()
    Q, n = 4, 1000
    res = random_records(RESULT_DTYPE, n, seed=7)
    ctx = gpu.Context(0, rss=True, rss_queues=Q)
    handle = ctx.stream
    ctx.steer(res)                                          # stage sized, kernels loaded
    ctx.wait_limit = LIMIT_US
    assert S.mtcp_gpu_debug_stall(ctx._h, STALL_US) == 0
    hidx, hstart = np.full(n, 0xA5A5A5A5, np.uint32), np.full(Q + 2, 0xA5A5A5A5, np.uint32)
    assert L.mtcp_gpu_steer(ctx._h, res.ctypes.data, n, 0, hidx.ctypes.data, hstart.ctypes.data) == ETIMEDOUT
    d_res = to_dev(res)
    idx, start, work = Guarded(4 * n), Guarded(4 * (Q + 2)), Guarded(16)
    own = torch.cuda.Stream(device=DEV)
    assert L.mtcp_gpu_steer_dev(ctx._h, d_res.data_ptr(), n, 0, idx.t.data_ptr(), start.t.data_ptr(), None, None,
                                work.t.data_ptr(), 16, own.cuda_stream) == EIO
    assert L.mtcp_gpu_steer(ctx._h, res.ctypes.data, n, 0, hidx.ctypes.data, hstart.ctypes.data) == EIO
    ctx.close()
    stream_wait(handle)
    own.synchronize()
    assert (idx.all == SENT).all().item() and (start.all == SENT).all().item()
    assert (hidx == 0xA5A5A5A5).all() and (hstart == 0xA5A5A5A5).all()
