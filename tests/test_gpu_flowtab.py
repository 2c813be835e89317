"""The device flow table on the GPU (include/mtcp_gpu_flowtab.h, mtcp_amd/csrc/
flowtab_kernels.hpp): every answer of every case is compared with
tests/flowtab_model.py, the restatement of mtcp/src/fhash.c; none is sampled.

Small tables (chains, wrap-around, a full table), 40 keys sharing one home
slot, batch sizes around the wave and workgroup with every verdict mixed in
and guard regions behind the outputs, the update's edge cases, 200 rounds of
churn and a rehash, the lookup behind the rx launch against the oracle's
records, a captured graph replayed, one full-size batch, the host calls
(unbounded, bounded, behind a stalled GPU) and the error returns."""
import ctypes
import time

import numpy as np
import pytest

import oracle
from mtcp_amd import RESULT_DTYPE, pktgen
from tests import flowtab_model as fm

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EINVAL, EIO, ETIMEDOUT = -22, -5, -110
GUARD = 4096                       # bytes behind every device output
SENT = 0xA5
SENT32 = 0xA5A5A5A5
MISS, NONE, MAX_ID = fm.FLOW_MISS, fm.FLOW_NONE, fm.MAX_ID


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


def random_keys(rng, n):
    """n distinct 12-byte keys."""
    k = np.unique(rng.integers(0, 256, (n + n // 8 + 8, 12), dtype=np.uint8), axis=0)
    assert len(k) >= n
    return k[rng.permutation(len(k))[:n]].copy()


def records_of(keys: np.ndarray, verdict=0) -> np.ndarray:
    """40 B rx records whose stream key is keys[i] (the packet carries it the
    other way round, tcp_in.c:1180-1186)."""
    e = fm.entries(keys, 0)
    r = np.zeros(len(keys), dtype=RESULT_DTYPE)
    r["daddr"], r["saddr"], r["dport"], r["sport"] = e["saddr"], e["daddr"], e["sport"], e["dport"]
    r["verdict"] = verdict
    return r


def keys_with_home(rng, cap_log2, home, count):
    """`count` distinct random keys whose home slot (mtcp_gpu_flowtab_home) is `home`."""
    from mtcp_amd import gpu as g
    out = set()
    while len(out) < count:
        for k in rng.integers(0, 256, (4096, 12), dtype=np.uint8):
            if g.FlowTable.home(bytes(k), cap_log2) == home:
                out.add(bytes(k))
    return np.frombuffer(b"".join(sorted(out)[:count]), dtype=np.uint8).reshape(count, 12).copy()


def dev_lookup(tab, res: np.ndarray, with_bins=True, stream=None):
    """lookup_dev with guarded outputs; returns (sid, bins or None)."""
    n = len(res)
    d_res = to_dev(res)
    sid, bins = Guarded(4 * n), Guarded(4 * n) if with_bins else None
    tab.lookup_dev(d_res, n, sid.t, None if bins is None else bins.t, stream=stream)
    torch.cuda.synchronize()
    assert sid.guard_intact(), "bytes behind d_sid were written"
    assert bins is None or bins.guard_intact(), "bytes behind d_bins were written"
    return sid.numpy(np.uint32), None if bins is None else bins.numpy(np.uint32)


def dev_update(tab, dele=None, ins=None, stream=None):
    d = None if dele is None or len(dele) == 0 else to_dev(dele)
    i = None if ins is None or len(ins) == 0 else to_dev(ins)
    tab.update_dev(d, 0 if d is None else len(dele), i, 0 if i is None else len(ins), stream=stream)
    torch.cuda.synchronize()


class Pair:
    """A device table and the model, kept in step."""

    def __init__(self, gpu, ctx, cap_log2):
        self.tab = gpu.FlowTable(ctx, cap_log2)
        self.model = fm.FlowTable()
        assert self.tab.capacity == 1 << cap_log2

    def update(self, dele=None, ins=None, host=False):
        if host:
            self.tab.update(dele, ins)
        else:
            dev_update(self.tab, dele, ins)
        self.model.update(() if dele is None else dele, () if ins is None else ins)

    def check(self, keys, what="", with_bins=True):
        """Every key of `keys` looked up as a TCP_OK record: the model's answer."""
        res = records_of(keys)
        sid, bins = dev_lookup(self.tab, res, with_bins)
        want = self.model.lookup(res)
        bad = np.nonzero(sid != want)[0]
        assert len(bad) == 0, f"{what}: {len(bad)} of {len(keys)} answers differ, first at {bad[0]}: " \
                              f"{sid[bad[0]]:#x} want {want[bad[0]]:#x}"
        if with_bins:
            assert np.array_equal(bins, oracle.flow_bins(res))
        return sid

    def check_stats(self, **want):
        st = self.tab.stats()
        assert st["live"] == self.model.count, st
        for k, v in want.items():
            assert st[k] == v, (k, st)
        return st

    def close(self):
        self.tab.close()


# ---- small tables -------------------------------------------------------------------------
@pytest.mark.parametrize("held", [1, 8, 15, 16])
def test_cap16(gpu, ctx, held):
    rng = np.random.default_rng(100 + held)
    keys = random_keys(rng, 16 + 16)
    mine, absent = keys[:held], keys[16:]
    p = Pair(gpu, ctx, 4)
    try:
        ids = rng.integers(0, MAX_ID + 1, held, dtype=np.uint64).astype(np.uint32)
        ids[0] = MAX_ID                                     # the largest id a slot may hold
        if held > 1:
            ids[1] = 0
        p.update(ins=fm.entries(mine, ids))
        p.check_stats(tombs=0, insert_failed=0, remove_missed=0)
        sid = p.check(keys, f"cap 16, {held} held")        # every held key, 16 absent ones (and unheld ones)
        assert (sid[:held] == ids).all() and (sid[16:] == MISS).all()
        if held == 16:
            # the table is full: a further insert is counted and changes no lookup,
            # and a miss ends after cap probes (the lookups of `absent` above did)
            dev_update(p.tab, ins=fm.entries(absent[:3], [1, 2, 3]))
            p.check_stats(tombs=0, insert_failed=3)
            assert np.array_equal(p.check(keys, "after the failed inserts"), sid)
    finally:
        p.close()


def test_cap16_chain_wraps_past_the_last_slot(gpu, ctx):
    rng = np.random.default_rng(7)
    keys = keys_with_home(rng, 4, 14, 10)                   # slots 14, 15, 0, 1, 2
    p = Pair(gpu, ctx, 4)
    try:
        p.update(ins=fm.entries(keys[:5], [50, 40, 30, 20, 10]))
        sid = p.check(keys, "wrapped chain")
        assert sid[:5].tolist() == [50, 40, 30, 20, 10] and (sid[5:] == MISS).all()
        p.update(dele=fm.entries(keys[1:2], [40]))          # a TOMB inside the chain: it still reaches its end
        sid = p.check(keys, "wrapped chain with a TOMB")
        assert sid[:5].tolist() == [50, MISS, 30, 20, 10]
        p.check_stats(tombs=1)
    finally:
        p.close()


# ---- collisions ---------------------------------------------------------------------------
def test_forty_keys_share_one_home_near_the_end(gpu, ctx):
    rng = np.random.default_rng(8)
    home = 1024 - 9
    keys = keys_with_home(rng, 10, home, 80)
    mine, absent = keys[:40], keys[40:]
    ids = rng.permutation(40).astype(np.uint32) + 1000
    p = Pair(gpu, ctx, 10)
    try:
        p.update(ins=fm.entries(mine, ids))
        assert np.array_equal(p.check(keys, "40 colliding keys")[:40], ids)
        third = np.arange(0, 40, 3)
        p.update(dele=fm.entries(mine[third], ids[third]))
        st = p.check_stats(tombs=len(third), insert_failed=0, remove_missed=0)
        sid = p.check(keys, "every third removed")
        assert (sid[third] == MISS).all() and (sid[40:] == MISS).all()
        p.update(ins=fm.entries(mine[third], ids[third]))   # the TOMB slots are taken again
        st2 = p.check_stats(insert_failed=0, remove_missed=0)
        assert st2["tombs"] == 0 < st["tombs"]
        assert np.array_equal(p.check(keys, "reinserted")[:40], ids)
    finally:
        p.close()


# ---- batch sizes ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table_4k(gpu, ctx):
    """cap 8 192 holding 3 000 of 6 000 keys."""
    rng = np.random.default_rng(9)
    keys = random_keys(rng, 6000)
    p = Pair(gpu, ctx, 13)
    p.update(ins=fm.entries(keys[:3000], np.arange(3000, dtype=np.uint32) * 7 + 1), host=True)
    yield p, keys
    p.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, 4097])
def test_batch_sizes_with_every_verdict(ctx, table_4k, n):
    p, keys = table_4k
    rng = np.random.default_rng(n)
    res = records_of(keys[rng.integers(0, len(keys), n)], verdict=rng.integers(0, 12, n).astype(np.uint8))
    res["verdict"][:: 3] = 0                                # a third TCP_OK at least
    want = p.model.lookup(res)
    sid, bins = dev_lookup(p.tab, res)
    assert np.array_equal(sid, want)
    assert ((sid == NONE) == (res["verdict"] != 0)).all()
    d_bins = torch.zeros(n, dtype=torch.int32, device=DEV)
    ctx.flow_hash_dev(to_dev(res), n, d_bins)
    torch.cuda.synchronize()
    assert np.array_equal(bins, d_bins.cpu().numpy().view(np.uint32))     # as mtcp_gpu_flow_hash_dev
    assert np.array_equal(bins, oracle.flow_bins(res))
    sid2, none = dev_lookup(p.tab, res, with_bins=False)   # d_bins == NULL
    assert none is None and np.array_equal(sid2, want)
    if n > 100:
        ok = res["verdict"] == 0
        assert (sid[ok] == MISS).sum() > n // 20 and (sid[ok] < MISS).sum() > n // 20


# ---- update edge cases ----------------------------------------------------------------------
def test_update_edge_cases(gpu, ctx):
    rng = np.random.default_rng(10)
    keys = random_keys(rng, 12)
    p = Pair(gpu, ctx, 6)
    try:
        p.update()                                          # n_del = n_ins = 0
        p.check_stats(tombs=0, insert_failed=0, remove_missed=0)
        p.update(ins=fm.entries(keys[:4], [10, 11, 12, 13]))            # n_del = 0
        p.update(dele=fm.entries(keys[:1], [10]))                       # n_ins = 0
        p.check_stats(tombs=1, remove_missed=0)
        assert p.check(keys, "after single-sided updates")[:4].tolist() == [MISS, 11, 12, 13]
        # an absent pair; the right key with the wrong id
        p.update(dele=fm.entries(keys[5:6], [1]))
        p.check_stats(remove_missed=1)
        p.update(dele=fm.entries(keys[1:2], [99]))
        p.check_stats(remove_missed=2)
        assert p.model.remove_missed == 2
        assert p.check(keys, "after missed removes")[:4].tolist() == [MISS, 11, 12, 13]
        # the same pair held twice, removed twice in one call
        twice = fm.entries(keys[[6, 6]], [77, 77])
        p.update(ins=twice)
        assert p.check(keys, "pair held twice")[6] == 77 and p.model.count == 5
        p.update(dele=twice)
        assert p.check(keys, "pair removed twice")[6] == MISS
        p.check_stats(remove_missed=2)
        # removes run before inserts within one call
        p.update(dele=fm.entries(keys[2:3], [12]), ins=fm.entries(keys[2:3], [5]))
        assert p.check(keys, "remove and insert of one key in one call")[2] == 5
        # duplicate keys, ids descending: the lowest id (the reference: the first inserted, 30)
        p.update(ins=fm.entries(keys[[8, 8, 8]], [30, 20, 25]))
        assert p.check(keys, "duplicate keys")[8] == 20 and p.model.search(bytes(keys[8])) == 30
        p.update(dele=fm.entries(keys[8:9], [20]))
        assert p.check(keys, "lowest duplicate removed")[8] == 25
        # an id above MAX_ID on the device path is counted, not held
        dev_update(p.tab, ins=fm.entries(keys[9:11], [MAX_ID + 1, MISS]))
        p.check_stats(insert_failed=2)
        dev_update(p.tab, dele=fm.entries(keys[:1], [MISS]))             # never matches the TOMB of keys[0]
        p.check_stats(insert_failed=2, remove_missed=3)
        p.check(keys, "after refused ids")
    finally:
        p.close()


# ---- churn and rehash ----------------------------------------------------------------------
def test_churn_then_rehash(gpu, ctx):
    rng = np.random.default_rng(11)
    keys = random_keys(rng, 96)
    held = {}                                               # key index -> id
    p = Pair(gpu, ctx, 6)
    try:
        first = rng.permutation(96)[:32]
        for k in first:
            held[int(k)] = int(rng.integers(0, MAX_ID + 1))
        p.update(ins=fm.entries(keys[first], [held[int(k)] for k in first]))
        next_id = 0
        for rnd in range(200):
            out = rng.permutation(sorted(held))[:8]
            free = rng.permutation([k for k in range(96) if k not in held])[:8]
            dele = fm.entries(keys[out], [held.pop(int(k)) for k in out])
            for k in free:
                held[int(k)] = next_id = next_id + 1
            p.update(dele=dele, ins=fm.entries(keys[free], [held[int(k)] for k in free]))
            sid = p.check(keys, f"round {rnd}", with_bins=False)
            assert (sid < MISS).sum() == 32
        st = p.check_stats(insert_failed=0, remove_missed=0)
        assert st["live"] == 32 and st["tombs"] > 0
        p.tab.rehash()
        st2 = p.check_stats(tombs=0, insert_failed=0, remove_missed=0)
        assert st2["live"] == 32
        assert np.array_equal(p.check(keys, "after rehash"), sid)
        p.update(dele=fm.entries(keys[[sorted(held)[0]]], [held[sorted(held)[0]]]))   # and it still updates
        p.check(keys, "update after rehash")
        p.check_stats(tombs=1)
    finally:
        p.close()


# ---- behind rx -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rx_batch():
    """65 536 generated bimodal frames, the oracle's records of them, the
    entries of the TCP_OK packets at even indices (id = packet index) and the
    model's answers."""
    n, seed = 65536, 31
    desc, nbytes = pktgen.layout(n, "bimodal", 6, seed)
    buf = np.zeros((nbytes + 63) & ~63, np.uint8)
    oracle.pktgen(buf, desc, 6, seed, 0)
    want = oracle.rx_chunk(buf, desc, 6, None)
    pick = np.nonzero((want["verdict"] == 0) & (np.arange(n) % 2 == 0))[0]
    ent = fm.entries(fm.record_keys(want[pick]), pick.astype(np.uint32))
    model = fm.FlowTable()
    model.update(ins=ent)
    ans = model.lookup(want)
    ok = want["verdict"] == 0
    # the condition on the even-index rule, from the oracle's records alone
    assert (ans[ok] < MISS).sum() >= ok.sum() // 4 and (ans[ok] == MISS).sum() >= ok.sum() // 4
    assert (ans[~ok] == NONE).all()
    return buf, desc, want, ent, ans


def test_lookup_behind_rx_on_one_stream(gpu, rx_batch):
    buf, desc, want, ent, ans = rx_batch
    n = len(desc)
    d_buf, d_desc, d_ent = to_dev(buf), to_dev(desc), to_dev(ent)
    d_res = torch.zeros(n * 40, dtype=torch.uint8, device=DEV)
    sid, bins = Guarded(4 * n), Guarded(4 * n)
    st = torch.cuda.Stream(device=DEV)
    with gpu.Context(0) as c, gpu.FlowTable(c, 17) as tab:
        c.rx_chunk_dev(d_buf, d_desc, n, 6, d_res, stream=st)
        tab.update_dev(None, 0, d_ent, len(ent), stream=st)
        tab.lookup_dev(d_res, n, sid.t, bins.t, stream=st)
        st.synchronize()
        assert tab.stats() == {"live": len(ent), "tombs": 0, "insert_failed": 0, "remove_missed": 0}
    assert sid.guard_intact() and bins.guard_intact()
    assert d_res.cpu().numpy().tobytes() == want.tobytes()
    got = sid.numpy(np.uint32)
    bad = np.nonzero(got != ans)[0]
    assert len(bad) == 0, (len(bad), bad[:5], got[bad[:5]], ans[bad[:5]])
    assert np.array_equal(bins.numpy(np.uint32), oracle.flow_bins(want))


def test_captured_rx_and_lookup_replay(gpu, rx_batch):
    """The update runs before the capture (replaying it would insert the same
    pairs again); rx and lookup are captured and replayed twice."""
    buf, desc, want, ent, ans = rx_batch
    n = len(desc)
    d_buf, d_desc, d_ent = to_dev(buf), to_dev(desc), to_dev(ent)
    d_res = torch.zeros(n * 40, dtype=torch.uint8, device=DEV)
    sid = Guarded(4 * n)
    st = torch.cuda.Stream(device=DEV)
    with gpu.Context(0) as c, gpu.FlowTable(c, 17) as tab:
        def launch():
            c.rx_chunk_dev(d_buf, d_desc, n, 6, d_res, stream=st)
            tab.lookup_dev(d_res, n, sid.t, None, stream=st)

        tab.update_dev(None, 0, d_ent, len(ent), stream=st)
        launch()                                            # kernels loaded before the capture
        st.synchronize()
        assert np.array_equal(sid.numpy(np.uint32), ans)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            launch()
        seen = []
        for _ in range(2):
            sid.t.fill_(SENT)
            d_res.zero_()
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert sid.guard_intact()
            seen.append(sid.numpy(np.uint32).copy())
            assert np.array_equal(seen[-1], ans)
        assert seen[0].tobytes() == seen[1].tobytes()
        del g


# ---- full size ------------------------------------------------------------------------------
def test_one_million_records_against_65536_flows(gpu, ctx):
    rng = np.random.default_rng(12)
    n, flows = 1 << 20, 65536
    keys = random_keys(rng, 2 * flows)
    ids = rng.permutation(flows).astype(np.uint32)
    p = Pair(gpu, ctx, 17)
    try:
        p.update(ins=fm.entries(keys[:flows], ids), host=True)
        p.check_stats(tombs=0, insert_failed=0, remove_missed=0)
        verdict = np.where(rng.random(n) < 0.9, 0, rng.integers(1, 12, n)).astype(np.uint8)
        which = rng.integers(0, 2 * flows, n)
        res = records_of(keys[which], verdict)
        want = np.where(which < flows, ids[np.minimum(which, flows - 1)], MISS).astype(np.uint32)
        want[verdict != 0] = NONE
        # the expected answers by construction equal the model's on every distinct key
        assert np.array_equal(p.model.lookup(records_of(keys)), np.concatenate([ids, np.full(flows, MISS, np.uint32)]))
        sid, bins = dev_lookup(p.tab, res)
        bad = np.nonzero(sid != want)[0]
        assert len(bad) == 0, (len(bad), bad[:5])
        assert np.array_equal(bins, oracle.flow_bins(res))
    finally:
        p.close()


# ---- host calls -----------------------------------------------------------------------------
@pytest.mark.parametrize("limit", [0, 5_000_000], ids=["unbounded", "bounded"])
def test_host_calls(gpu, limit):
    rng = np.random.default_rng(13)
    keys = random_keys(rng, 3000)
    with gpu.Context(0) as c:
        if limit:
            c.wait_limit = limit
        p = Pair(gpu, c, 12)
        try:
            p.update(ins=fm.entries(keys[:1500], np.arange(1500, dtype=np.uint32)), host=True)
            p.update(dele=fm.entries(keys[:500], np.arange(500, dtype=np.uint32)),
                     ins=fm.entries(keys[2000:2200], np.arange(200, dtype=np.uint32) + 5000), host=True)
            res = records_of(keys, verdict=(np.arange(3000) % 5 == 4).astype(np.uint8) * 9)
            want = p.model.lookup(res)
            sid, bins = p.tab.lookup(res, bins=True)
            assert np.array_equal(sid, want) and np.array_equal(bins, oracle.flow_bins(res))
            assert np.array_equal(p.tab.lookup(res), want)                # bins == NULL
            assert np.array_equal(p.tab.lookup(res[:3]), want[:3])        # the staging reused by a smaller call
            st = p.check_stats(insert_failed=0, remove_missed=0)
            assert 300 <= st["tombs"] <= 500                              # 500 removed; each of the 200 inserts may reuse one
            p.tab.rehash()
            p.check_stats(tombs=0)
            assert np.array_equal(p.tab.lookup(res), want)
        finally:
            p.close()


def test_host_calls_give_up_at_the_limit(gpu):
    """The stalled-GPU pattern of tests/test_gpu_bounded.py (its helpers, its
    stall and limit values): ETIMEDOUT within the limit, sid and bins keep
    their sentinel right after the call and after the stall has ended, the
    context answers EIO to every table call, a fresh context and table give
    the model's answers."""
    from mtcp_amd._lib import lib
    from tests.test_gpu_bounded import LIMIT_US, SLACK_S, STALL_US, stall_lib, stream_busy, stream_wait
    L, S = lib(), stall_lib()
    rng = np.random.default_rng(14)
    keys = random_keys(rng, 1000)
    ent = fm.entries(keys[:500], np.arange(500, dtype=np.uint32) + 3)
    res = records_of(keys)
    n = len(res)
    model = fm.FlowTable()
    model.update(ins=ent)
    want = model.lookup(res)

    def call(tab):
        sid, bins = np.full(n, SENT32, np.uint32), np.full(n, SENT32, np.uint32)
        rc = L.mtcp_gpu_flowtab_lookup(tab._h, res.ctypes.data, n, sid.ctypes.data, bins.ctypes.data)
        return rc, sid, bins

    c = gpu.Context(0)
    handle = c.stream
    tab = gpu.FlowTable(c, 11)
    tab.update(ins=ent)
    rc, sid, bins = call(tab)                               # unbounded: stage sized, kernels loaded
    assert rc == 0 and np.array_equal(sid, want)
    c.wait_limit = LIMIT_US
    rc, sid, bins = call(tab)                               # bounded, no stall: the bounce buffers sized
    assert rc == 0 and np.array_equal(sid, want)
    assert S.mtcp_gpu_debug_stall(c._h, STALL_US) == 0
    t0 = time.monotonic()
    rc, sid, bins = call(tab)
    dt = time.monotonic() - t0
    assert rc == ETIMEDOUT, rc
    assert dt < LIMIT_US / 1e6 + SLACK_S, dt
    assert stream_busy(handle)
    assert (sid == SENT32).all() and (bins == SENT32).all()
    assert L.mtcp_gpu_sync(c._h) == EIO
    rc2, sid2, bins2 = call(tab)
    assert rc2 == EIO and (sid2 == SENT32).all() and (bins2 == SENT32).all()
    st = np.full(4, SENT32, np.uint32)
    assert L.mtcp_gpu_flowtab_stats(tab._h, st.ctypes.data) == EIO and (st == SENT32).all()
    assert L.mtcp_gpu_flowtab_update(tab._h, None, 0, ent.ctypes.data, 1) == EIO
    assert L.mtcp_gpu_flowtab_rehash(tab._h) == EIO
    d = to_dev(ent)
    own = torch.cuda.Stream(device=DEV)
    assert L.mtcp_gpu_flowtab_update_dev(tab._h, None, 0, d.data_ptr(), 1, own.cuda_stream) == EIO
    dsid = Guarded(4 * n)
    assert L.mtcp_gpu_flowtab_lookup_dev(tab._h, to_dev(res).data_ptr(), n, dsid.t.data_ptr(), None,
                                         own.cuda_stream) == EIO
    other = ctypes.c_void_p()
    assert L.mtcp_gpu_flowtab_create(c._h, 10, ctypes.byref(other)) == EIO and not other
    tab.close()
    c.close()
    stream_wait(handle)                                     # the stall and what was queued behind it end
    own.synchronize()
    assert (sid == SENT32).all() and (bins == SENT32).all()
    assert (dsid.all == SENT).all().item()
    with gpu.Context(0) as fresh, gpu.FlowTable(fresh, 11) as tab2:
        fresh.wait_limit = 5_000_000
        tab2.update(ins=ent)
        rc, sid, bins = call(tab2)
        assert rc == 0 and np.array_equal(sid, want) and np.array_equal(bins, oracle.flow_bins(res))


# ---- error returns ---------------------------------------------------------------------------
def test_error_returns(gpu, ctx):
    from mtcp_amd._lib import lib
    L = lib()
    rng = np.random.default_rng(15)
    keys = random_keys(rng, 64)
    ent = fm.entries(keys, np.arange(64, dtype=np.uint32))
    res = records_of(keys)
    n = len(res)
    h = ctypes.c_void_p()
    for bad_log2 in (0, 3, 27, 64):
        assert L.mtcp_gpu_flowtab_create(ctx._h, bad_log2, ctypes.byref(h)) == EINVAL and not h
    assert L.mtcp_gpu_flowtab_create(None, 10, ctypes.byref(h)) == EINVAL
    assert L.mtcp_gpu_flowtab_create(ctx._h, 10, None) == EINVAL
    assert L.mtcp_gpu_flowtab_capacity(None) == 0
    L.mtcp_gpu_flowtab_destroy(None)
    with gpu.FlowTable(ctx, 8) as tab:
        t = tab._h
        d_ent, d_res = Guarded(16 * n + 16), to_dev(res)
        d_ent.t[:16 * n] = to_dev(ent)
        sid, bins = Guarded(4 * n + 8), Guarded(4 * n + 8)
        p = lambda x, off=0: x.data_ptr() + off
        big = (1 << 26) + 1

        def upd(tab_h=t, d=None, nd=0, i=p(d_ent.t), ni=n):
            return L.mtcp_gpu_flowtab_update_dev(tab_h, d, nd, i, ni, None)

        def look(tab_h=t, r=p(d_res), n_=n, s=p(sid.t), b=p(bins.t)):
            return L.mtcp_gpu_flowtab_lookup_dev(tab_h, r, n_, s, b, None)

        bad = {
            "update tab NULL": upd(tab_h=None), "ins NULL": upd(i=None), "del NULL": upd(d=None, nd=1),
            "ins misaligned": upd(i=p(d_ent.t, 8)), "del misaligned": upd(d=p(d_ent.t, 4), nd=1),
            "n_ins too large": upd(ni=big), "n_del too large": upd(d=p(d_ent.t), nd=big),
            "lookup tab NULL": look(tab_h=None), "res NULL": look(r=None), "sid NULL": look(s=None),
            "res misaligned": look(r=p(d_res, 4)), "sid misaligned": look(s=p(sid.t, 2)),
            "bins misaligned": look(b=p(bins.t, 1)), "n too large": look(n_=big),
        }
        assert {k: v for k, v in bad.items() if v != EINVAL} == {}
        assert upd(ni=0) == 0 and upd(i=None, ni=0) == 0 and look(n_=0) == 0
        assert look(n_=0, r=None, s=None, b=None) == 0
        # host calls
        hsid, hbins = np.full(n, SENT32, np.uint32), np.full(n, SENT32, np.uint32)
        over = ent.copy()
        over["id"][5] = MAX_ID + 1
        hu = lambda **kw: L.mtcp_gpu_flowtab_update(kw.get("t", t), kw.get("d", None), kw.get("nd", 0),
                                                    kw.get("i", ent.ctypes.data), kw.get("ni", n))
        hl = lambda **kw: L.mtcp_gpu_flowtab_lookup(kw.get("t", t), kw.get("r", res.ctypes.data), kw.get("n", n),
                                                    kw.get("s", hsid.ctypes.data), kw.get("b", hbins.ctypes.data))
        assert hu(t=None) == EINVAL and hu(i=None) == EINVAL and hu(d=None, nd=1) == EINVAL
        assert hu(ni=big) == EINVAL and hu(d=ent.ctypes.data, nd=big) == EINVAL
        assert hu(i=over.ctypes.data) == EINVAL                    # an id above MAX_ID, as an insert
        assert hu(d=over.ctypes.data, nd=n, ni=0) == EINVAL        # and as a remove
        assert hl(t=None) == EINVAL and hl(r=None) == EINVAL and hl(s=None) == EINVAL and hl(n=big) == EINVAL
        assert hu(ni=0) == 0 and hl(n=0) == 0
        assert L.mtcp_gpu_flowtab_stats(None, hsid.ctypes.data) == EINVAL
        assert L.mtcp_gpu_flowtab_stats(t, None) == EINVAL
        assert L.mtcp_gpu_flowtab_rehash(None) == EINVAL
        torch.cuda.synchronize()
        assert (sid.all == SENT).all().item() and (bins.all == SENT).all().item()    # none of these wrote anything
        assert (hsid == SENT32).all() and (hbins == SENT32).all()
        assert tab.stats() == {"live": 0, "tombs": 0, "insert_failed": 0, "remove_missed": 0}
        assert upd() == 0 and look() == 0                          # and the same arguments, valid, work
        torch.cuda.synchronize()
        assert np.array_equal(sid.numpy(np.uint32)[:n], np.arange(n, dtype=np.uint32))
        assert tab.stats()["live"] == n
    # 16 B records carry no addresses
    with gpu.Context(0, compact=True) as cc, gpu.FlowTable(cc, 8) as tab:
        tab.update(ins=ent)                                        # the table itself works
        assert tab.stats()["live"] == n
        sid = Guarded(4 * n)
        assert L.mtcp_gpu_flowtab_lookup_dev(tab._h, to_dev(res).data_ptr(), n, sid.t.data_ptr(), None, None) == EINVAL
        hsid = np.full(n, SENT32, np.uint32)
        assert L.mtcp_gpu_flowtab_lookup(tab._h, res.ctypes.data, n, hsid.ctypes.data, None) == EINVAL
        torch.cuda.synchronize()
        assert (sid.all == SENT).all().item() and (hsid == SENT32).all()
