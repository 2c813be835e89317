"""Cutting send bursts into tx segments on the GPU (include/mtcp_gpu_txseg.h,
mtcp_amd/csrc/txseg_kernels.hpp): segment records, descriptors, results and
totals byte for byte against tests/txseg_model.py (FlushTCPSendingBuffer's
loop restated literally), the frames behind them against tests/txbuild_model.py,
never against the kernels' own output.  Every output has a guard region behind
it and the workspace is sized exactly."""
import time

import numpy as np
import pytest

from mtcp_amd import DESC_DTYPE, RESULT_DTYPE
from tests import txbuild_model as bm, txseg_model as m

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EINVAL, EIO, ETIMEDOUT = -22, -5, -110
GUARD = 4096
SENT = 0xA5
ONE, MANY = "txseg_one_kernel", "txseg_emit_kernel"
ONE_SEGS = 4096                       # txseg_kernels.hpp kTxsegOneSegs
EMIT_TILE = 1024                      # kTxsegEmitTile
EDGE = m.edge_lists()


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
def tile(gpu):
    return gpu.Context.tx_segment_tile()


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)


class Guarded:
    """nbytes of device memory between two guards of 0xA5."""

    def __init__(self, nbytes):
        self.nbytes = nbytes
        self.whole = torch.full((GUARD + nbytes + GUARD,), SENT, dtype=torch.uint8, device=DEV)
        self.t = self.whole[GUARD:GUARD + nbytes]

    def read(self, what):
        w = self.whole.cpu().numpy()
        assert (w[:GUARD] == SENT).all() and (w[GUARD + self.nbytes:] == SENT).all(), f"{what}: guard written"
        return w[GUARD:GUARD + self.nbytes]


class Run:
    """One device run of mtcp_gpu_tx_segment_dev (or, with payload and links,
    of mtcp_gpu_tx_send_dev)."""

    def __init__(self, ctx, gpu, bursts, kw, payload=None, links=None, flags=0, stream=None):
        self.ctx, self.kw, self.n, self.cap = ctx, kw, len(bursts), kw["seg_cap"]
        self.stream, self.flags = stream, flags
        self.d_burst = up(bursts) if len(bursts) else torch.zeros(64, dtype=torch.uint8, device=DEV)
        self.seg, self.desc = Guarded(48 * self.cap), Guarded(8 * self.cap)
        self.res, self.total = Guarded(16 * self.n), Guarded(16)
        self.work = Guarded(gpu.Context.tx_segment_work_bytes(self.n))
        self.send = payload is not None
        if self.send:
            self.d_payload, self.d_links = up(payload), up(links)
            self.buf, self.status = Guarded(kw["buf_len"]), Guarded(self.cap)
        torch.cuda.synchronize()             # the fills above are done before a launch on another stream

    def launch(self):
        kw = self.kw
        if self.send:
            self.ctx.tx_send_dev(self.d_burst, self.n, self.d_payload, self.d_links, self.buf.t, kw["buf_off"],
                                 kw["off_shift"], kw["slot_bytes"], self.seg.t, self.desc.t, self.cap, self.res.t,
                                 self.total.t, self.status.t, self.work.t, max_mss=kw.get("max_mss", 0),
                                 flags=self.flags, stream=self.stream)
        else:
            self.ctx.tx_segment_dev(self.d_burst, self.n, kw["payload_bytes"], kw["n_links"], kw["buf_off"],
                                    kw["buf_len"], kw["off_shift"], kw["slot_bytes"], self.seg.t, self.desc.t,
                                    self.cap, self.res.t, self.total.t, self.work.t, max_mss=kw.get("max_mss", 0),
                                    stream=self.stream)

    def read(self):
        torch.cuda.synchronize()
        self.work.read("workspace")
        out = (self.seg.read("records").view(bm.SEG_DTYPE), self.desc.read("descriptors").view(DESC_DTYPE),
               self.res.read("results").view(m.RESULT_DTYPE), self.total.read("totals").view(np.uint64))
        if self.send:
            out += (self.buf.read("frames"), self.status.read("status"))
        return out


def assert_records(got, want, what):
    for name, g, w in zip(("records", "descriptors", "results", "totals"), got, want):
        if g.tobytes() == w.tobytes():
            continue
        size = g.dtype.itemsize
        a, b = g.view(np.uint8).reshape(-1, size), w.view(np.uint8).reshape(-1, size)
        i = int(np.flatnonzero((a != b).any(axis=1))[0])
        raise AssertionError(f"{what}: {name} differ first at {i}: got {g[i]}, model {w[i]}")


def segment(ctx, gpu, bursts, kw, kernel=None, what=""):
    want = m.expand(bursts, **kw)
    r = Run(ctx, gpu, bursts, kw)
    r.launch()
    got = r.read()
    if kernel:
        assert ctx.last_kernel == kernel
    assert_records(got, want, what)
    return want


def fanout_bursts(n, seed, lo=0, hi=46):
    """n bursts of lo..hi segments at mss 1460, every eighth stopped by its
    window somewhere; payload offsets anywhere in 1 MiB."""
    rng = np.random.default_rng(seed)
    b = m.random_bursts(n, seed, 1 << 20, mss_choices=(1460,), p_stop=0, p_empty=0)
    fan = rng.integers(lo, hi + 1, n)
    fan[np.arange(n) % 16 == 7], fan[np.arange(n) % 16 == 3] = lo, hi
    ln = np.where(fan == 0, 0, (fan - 1) * 1448 + rng.integers(1, 1449, n))
    b["len"], b["payload_off"] = ln, rng.integers(0, (1 << 20) - 46 * 1448, n)
    window = b["in_flight"].astype(np.int64) + ln
    stopped = np.arange(n) % 8 == 5
    window[stopped] -= (ln[stopped] * rng.random(int(stopped.sum()))).astype(np.int64)
    b["window"] = b["peer_wnd"] = window
    return b


ROOMY = dict(payload_bytes=1 << 20, n_links=3, buf_off=0, buf_len=1 << 40, off_shift=6, slot_bytes=0, max_mss=0)


# ---- 1. sizes --------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["one", "many"])
@pytest.mark.parametrize("n_of", ["1", "2", "63", "64", "65", "T-1", "T", "T+1", "3*T+5"])
def test_sizes(ctx, gpu, tile, n_of, form):
    n = int(eval(n_of, {"T": tile}))
    bursts = fanout_bursts(n, seed=n)
    planned = int(m.expand(bursts, **dict(ROOMY, seg_cap=1 << 20))[3][0])
    if form == "one":
        # above one plan tile there is no one-workgroup form: the batch is cut by a small seg_cap instead
        kw = dict(ROOMY, seg_cap=min(planned + 37, ONE_SEGS))
        kernel = ONE if n <= tile else MANY
    else:
        kw = dict(ROOMY, seg_cap=max(planned + 37, ONE_SEGS + 1))
        kernel = MANY
    _, _, res, total = segment(ctx, gpu, bursts, kw, kernel, f"n {n} {form}")
    assert int(total[0]) == min(planned, kw["seg_cap"])
    if n >= 63:
        assert res["n_seg"].max() >= 40 and (res["n_seg"] == 0).any() and (res["stop"] & 1).any()


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("slot_bytes", [0, 1536])
def test_one_long_burst_among_single_segment_ones(ctx, gpu, where, slot_bytes):
    """2 001 records of one burst cross two emit tiles' borders."""
    singles = fanout_bursts(3000, seed=77, lo=1, hi=1)
    big = m._burst(len=2001 * 524, mss=536, payload_off=5, ip_id=0xFF00, seq=0xFFF00000)
    at = {"first": 0, "middle": 1500, "last": 3000}[where]
    bursts = np.concatenate([singles[:at], big, singles[at:]])
    kw = dict(ROOMY, payload_bytes=1 << 21, slot_bytes=slot_bytes, seg_cap=5001 + 100)
    _, _, res, total = segment(ctx, gpu, bursts, kw, MANY, f"long burst {where}")
    assert int(total[0]) > 4500 and int(res["n_seg"][at]) == 2001
    assert int(res["first_seg"][at]) // EMIT_TILE != (int(res["first_seg"][at]) + 2000) // EMIT_TILE


def test_runs_of_empty_bursts_inside_one_tile(ctx, gpu):
    """More bursts meet one emit tile than it stages: thousands without a
    segment (empty, refused, stopped at once) between those with one."""
    some = fanout_bursts(40, seed=5, lo=1, hi=3)
    none = np.concatenate([m._burst(len=0), m._burst(len=100, rsvd0=1), m._burst(len=100, window=50, peer_wnd=10)])
    bursts = np.concatenate([some[:10], np.tile(none, 1500), some[10:20], np.tile(none, 900), some[20:],
                             np.tile(none, 300)])
    kw = dict(ROOMY, seg_cap=300)
    _, _, res, total = segment(ctx, gpu, bursts, kw, MANY, "empty runs")
    assert 40 <= int(total[0]) <= 120 and (res["status"] == 1).sum() == 2700


# ---- 2. the edge lists -----------------------------------------------------------------
def edge_params():
    out = []
    for name, b, kw in EDGE:
        out.append((name, b, kw))
        if kw["slot_bytes"] == 0 and not name.startswith("room"):
            out.append((name + "_fixed_64k", b, dict(kw, off_shift=6, slot_bytes=65536)))
    return out


@pytest.mark.parametrize("form", ["one", "many"])
@pytest.mark.parametrize("name,bursts,kw", edge_params(), ids=[e[0] for e in edge_params()])
def test_edge_lists(ctx, gpu, tile, name, bursts, kw, form):
    if form == "many":      # empty bursts in front: more than one plan tile, the same segments
        bursts = np.concatenate([np.tile(m._burst(len=0), tile + 1), bursts])
    segment(ctx, gpu, bursts, kw, ONE if form == "one" else MANY, f"{name} {form}")


def test_no_bursts(ctx, gpu):
    for cap, kernel in ((7, ONE), (ONE_SEGS + 3, MANY)):
        _, _, _, total = segment(ctx, gpu, np.zeros(0, m.BURST_DTYPE), dict(ROOMY, seg_cap=cap), kernel, "no bursts")
        assert total.tolist() == [0, 0]


# ---- 3. segment + build ------------------------------------------------------------------
def send_case(n, seed, off_shift, slot_bytes, buf_off):
    nbytes = 1 << 19
    rng = np.random.default_rng(seed)
    bursts = m.random_bursts(n, seed, nbytes, mss_choices=(536, 1460, 1460, 1460), max_len=12000)
    bursts["rsvd1"][::41] = 9
    payload = rng.integers(0, 256, nbytes, dtype=np.uint8)
    links = np.zeros(3, dtype=bm.LINK_DTYPE)
    links["dst"], links["src"] = rng.integers(0, 256, (3, 6)), rng.integers(0, 256, (3, 6))
    kw = dict(payload_bytes=nbytes, n_links=3, buf_off=buf_off, buf_len=1 << 40, off_shift=off_shift,
              slot_bytes=slot_bytes, seg_cap=1 << 16, max_mss=0)
    total = m.expand(bursts, **kw)[3]
    kw["buf_len"] = (buf_off + int(total[1]) + 64 + 15) // 16 * 16     # what the rx call behind it asks of buf_len
    kw["seg_cap"] = int(total[0]) + 300                     # oversized: the tail is void
    return bursts, payload, links, kw


@pytest.mark.parametrize("flags", [0, bm.NO_CSUM], ids=["csum", "no_csum"])
@pytest.mark.parametrize("off_shift,slot_bytes,buf_off", [(6, 0, 128), (0, 1536, 2), (1, 0, 0)])
def test_send_dev_end_to_end(gpu, off_shift, slot_bytes, buf_off, flags):
    bursts, payload, links, kw = send_case(300, 31 + off_shift, off_shift, slot_bytes, buf_off)
    seg, desc, res, total = want = m.expand(bursts, **kw)
    k, cap = int(total[0]), kw["seg_cap"]
    assert k >= 400 and cap == k + 300 and {0, 1} <= set(res["status"].tolist()) and (res["stop"] & 1).any()
    want_img, want_status = bm.build_frames(seg, payload, links, desc, np.full(kw["buf_len"], SENT, np.uint8),
                                            off_shift=off_shift, flags=flags)
    assert not want_status[:k].any() and (want_status[k:] == bm.BAD_SEG).all()
    st = torch.cuda.Stream(device=DEV)
    with gpu.Context(0) as c:
        r = Run(c, gpu, bursts, kw, payload, links, flags=flags, stream=st)
        d_rx = torch.zeros(k * 40, dtype=torch.uint8, device=DEV)
        r.launch()
        c.rx_chunk_dev(r.buf.t, r.desc.t, k, off_shift, d_rx, stream=st)
        *got, image, status = r.read()
    assert_records(got, want, "send_dev")
    # the void records are BAD_SEG to the builder, exactly those, and no byte outside the built frames is written
    assert np.array_equal(status, want_status)
    assert np.array_equal(image, want_img), f"first byte {np.flatnonzero(image != want_img)[:1]}"
    offs = desc["offset"][:k].astype(np.int64) << off_shift
    assert (image[:buf_off] == SENT).all()
    if flags & bm.NO_CSUM:
        for f in (24, 25, 50, 51):
            assert not image[offs + f].any()
        return
    rx = d_rx.cpu().numpy().view(RESULT_DTYPE)
    assert (rx["verdict"] == 0).all() and np.array_equal(rx["payload_len"], seg["payload_len"][:k])
    assert np.array_equal(rx["seq"], seg["seq"][:k])
    for b, x in zip(bursts, res):                           # per burst: its bytes, in order, and consecutive IP ids
        f0, cnt = int(x["first_seg"]), int(x["n_seg"])
        frames = [image[offs[j]:offs[j] + int(desc["len"][j])] for j in range(f0, f0 + cnt)]
        order = np.argsort([(int(rx["seq"][j]) - int(b["seq"])) & 0xFFFFFFFF for j in range(f0, f0 + cnt)])
        sent = np.concatenate([frames[j][66:] for j in order]) if cnt else np.zeros(0, np.uint8)
        at = int(b["payload_off"])
        assert np.array_equal(sent, payload[at:at + int(x["bytes"])])
        ids = [(int(f[18]) << 8) | int(f[19]) for f in frames]
        assert ids == [(int(b["ip_id"]) + j) & 0xFFFF for j in range(cnt)]


# ---- 4. a captured graph -----------------------------------------------------------------
def test_captured_segment_and_build_replay(gpu):
    bursts, payload, links, kw = send_case(300, 57, 6, 0, 64)
    want = m.expand(bursts, **kw)
    want_img, want_status = bm.build_frames(want[0], payload, links, want[1],
                                            np.full(kw["buf_len"], SENT, np.uint8), off_shift=6)
    st = torch.cuda.Stream(device=DEV)
    with gpu.Context(0) as c:
        r = Run(c, gpu, bursts, kw, payload, links, stream=st)
        r.launch()                                         # kernels loaded before the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            r.launch()
        seen = []
        for _ in range(2):
            for x in (r.seg, r.desc, r.res, r.total, r.buf, r.status, r.work):
                x.whole.fill_(SENT)
            torch.cuda.synchronize()
            g.replay()
            *got, image, status = r.read()
            assert_records(got, want, "replay")
            assert np.array_equal(image, want_img) and np.array_equal(status, want_status)
            seen.append(b"".join(x.tobytes() for x in got) + image.tobytes() + status.tobytes())
        assert seen[0] == seen[1]
        del g


# ---- 5. the host call -----------------------------------------------------------------
def host_call(L, c, bursts, payload, links, kw, flags=0):
    cap = kw["seg_cap"]
    buf = np.full(kw["buf_len"], SENT, np.uint8)
    desc = np.full(cap * 8, SENT, np.uint8)
    res = np.full(len(bursts) * 16, SENT, np.uint8)
    status = np.full(cap, SENT, np.uint8)
    total = np.full(16, SENT, np.uint8)
    rc = L.mtcp_gpu_tx_send(c._h, bursts.ctypes.data, len(bursts), payload.ctypes.data, payload.nbytes,
                            links.ctypes.data, len(links), buf.ctypes.data, kw["buf_off"], kw["buf_len"],
                            kw["off_shift"], kw["slot_bytes"], kw.get("max_mss", 0), flags, desc.ctypes.data, cap,
                            res.ctypes.data, total.ctypes.data, status.ctypes.data)
    return rc, buf, desc, res, total, status


def assert_host(out, want, want_img, want_status, what):
    rc, buf, desc, res, total, status = out
    assert rc == 0, rc
    assert_records((want[0], desc.view(DESC_DTYPE), res.view(m.RESULT_DTYPE), total.view(np.uint64)), want, what)
    assert np.array_equal(status, want_status) and np.array_equal(buf, want_img), what


@pytest.mark.parametrize("limit", [0, 5_000_000], ids=["unbounded", "bounded"])
def test_host_call(gpu, limit):
    """A small batch at the staging's first size, a larger one (the staging
    grows), the small one again; equal to the model, as the device path is."""
    from mtcp_amd._lib import lib
    cases = {}
    for what, n, shift, slot in (("small", 20, 0, 0), ("large", 400, 6, 1536)):
        bursts, payload, links, kw = send_case(n, 90 + n, shift, slot, 64)
        want = m.expand(bursts, **kw)
        img, status = bm.build_frames(want[0], payload, links, want[1], np.full(kw["buf_len"], SENT, np.uint8),
                                      off_shift=shift)
        cases[what] = (bursts, payload, links, kw, want, img, status)
    with gpu.Context(0) as c:
        c.wait_limit = limit
        for what in ("small", "large", "small"):
            bursts, payload, links, kw, want, img, status = cases[what]
            assert_host(host_call(lib(), c, bursts, payload, links, kw), want, img, status, f"{what} limit {limit}")
        bursts, payload, links, kw, want, img, status = cases["small"]
        desc, res, total, st = c.tx_send(bursts, payload, links, buf := np.full(kw["buf_len"], SENT, np.uint8),
                                         kw["seg_cap"], buf_off=kw["buf_off"])
        assert_records((want[0], desc, res.view(m.RESULT_DTYPE), total), want, "Context.tx_send")
        assert np.array_equal(buf, img) and np.array_equal(st, status)


def test_host_call_gives_up_at_the_limit(gpu):
    """The stalled-GPU pattern of tests/test_gpu_bounded.py (its helpers, its
    stall and limit values): ETIMEDOUT within the limit; buf, desc, res, total
    and status keep their sentinel right after the call and after the stall
    has ended; the context answers EIO; a fresh context gives the model's bytes."""
    from mtcp_amd._lib import lib
    from tests.test_gpu_bounded import LIMIT_US, SLACK_S, STALL_US, stall_lib, stream_busy, stream_wait
    L, S = lib(), stall_lib()
    bursts, payload, links, kw = send_case(20, 110, 0, 0, 64)
    want = m.expand(bursts, **kw)
    img, wstatus = bm.build_frames(want[0], payload, links, want[1], np.full(kw["buf_len"], SENT, np.uint8))
    untouched = lambda out: all((a == SENT).all() for a in out[1:])

    c = gpu.Context(0)
    handle = c.stream
    assert_host(host_call(L, c, bursts, payload, links, kw), want, img, wstatus, "before the stall")
    r = Run(c, gpu, bursts, kw, payload, links)             # device buffers for the calls refused below
    c.wait_limit = LIMIT_US
    assert S.mtcp_gpu_debug_stall(c._h, STALL_US) == 0
    t0 = time.monotonic()
    out = host_call(L, c, bursts, payload, links, kw)
    dt = time.monotonic() - t0
    assert out[0] == ETIMEDOUT, out[0]
    assert dt < LIMIT_US / 1e6 + SLACK_S, dt
    assert stream_busy(handle)
    assert untouched(out)
    assert L.mtcp_gpu_sync(c._h) == EIO
    out2 = host_call(L, c, bursts, payload, links, kw)
    assert out2[0] == EIO and untouched(out2)
    # the device calls on the abandoned context: EIO, nothing launched
    a = (r.d_burst.data_ptr(), r.n)
    geom = (kw["buf_off"], kw["buf_len"], kw["off_shift"], kw["slot_bytes"], 0)
    outs = (r.seg.t.data_ptr(), r.desc.t.data_ptr(), r.cap, r.res.t.data_ptr(), r.total.t.data_ptr())
    assert L.mtcp_gpu_tx_segment_dev(c._h, *a, len(payload), 3, *geom, *outs, r.work.t.data_ptr(), r.work.nbytes,
                                     None) == EIO
    assert L.mtcp_gpu_tx_send_dev(c._h, *a, r.d_payload.data_ptr(), len(payload), r.d_links.data_ptr(), 3,
                                  r.buf.t.data_ptr(), *geom, 0, *outs, r.status.t.data_ptr(),
                                  r.work.t.data_ptr(), r.work.nbytes, None) == EIO
    c.close()
    stream_wait(handle)                                     # the stall and what was queued behind it end
    assert untouched(out)
    for x in (r.seg, r.desc, r.res, r.total, r.buf, r.status, r.work):
        assert (x.read("abandoned context") == SENT).all()
    with gpu.Context(0) as fresh:
        fresh.wait_limit = 5_000_000
        assert_host(host_call(L, fresh, bursts, payload, links, kw), want, img, wstatus, "fresh context")


# ---- 6. error returns -----------------------------------------------------------------
def test_error_returns(ctx, gpu):
    from mtcp_amd._lib import lib
    L = lib()
    bursts, payload, links, kw = send_case(20, 130, 6, 0, 64)
    want = m.expand(bursts, **kw)
    r = Run(ctx, gpu, bursts, kw, payload, links)
    pad = torch.zeros(64, dtype=torch.uint8, device=DEV)
    good = dict(burst=r.d_burst.data_ptr(), n_burst=r.n, payload=r.d_payload.data_ptr(), payload_bytes=len(payload),
                links=r.d_links.data_ptr(), n_links=3, buf=r.buf.t.data_ptr(), buf_off=64, buf_len=kw["buf_len"],
                off_shift=6, slot_bytes=0, max_mss=0, flags=0, seg=r.seg.t.data_ptr(), desc=r.desc.t.data_ptr(),
                seg_cap=r.cap, res=r.res.t.data_ptr(), total=r.total.t.data_ptr(), status=r.status.t.data_ptr(),
                work=r.work.t.data_ptr(), work_bytes=r.work.nbytes)

    def seg_dev(h=ctx._h, **kw2):
        a = dict(good, **kw2)
        return L.mtcp_gpu_tx_segment_dev(h, a["burst"], a["n_burst"], a["payload_bytes"], a["n_links"],
                                         a["buf_off"], a["buf_len"], a["off_shift"], a["slot_bytes"], a["max_mss"],
                                         a["seg"], a["desc"], a["seg_cap"], a["res"], a["total"], a["work"],
                                         a["work_bytes"], None)

    def send_dev(h=ctx._h, **kw2):
        a = dict(good, **kw2)
        return L.mtcp_gpu_tx_send_dev(h, a["burst"], a["n_burst"], a["payload"], a["payload_bytes"],
                                      a["links"], a["n_links"], a["buf"], a["buf_off"], a["buf_len"], a["off_shift"],
                                      a["slot_bytes"], a["max_mss"], a["flags"], a["seg"], a["desc"], a["seg_cap"],
                                      a["res"], a["total"], a["status"], a["work"], a["work_bytes"], None)

    shared = [dict(burst=None), dict(seg=None), dict(desc=None), dict(res=None), dict(total=None), dict(work=None),
              dict(burst=pad.data_ptr() + 4), dict(seg=pad.data_ptr() + 4), dict(desc=pad.data_ptr() + 4),
              dict(res=pad.data_ptr() + 4), dict(total=pad.data_ptr() + 4), dict(work=pad.data_ptr() + 8),
              dict(off_shift=17), dict(n_links=0), dict(n_links=257), dict(seg_cap=0), dict(seg_cap=(1 << 26) + 1),
              dict(n_burst=(1 << 24) + 1), dict(work_bytes=good["work_bytes"] - 1), dict(slot_bytes=1000),
              dict(buf_off=32)]
    for f in (seg_dev, send_dev):
        assert f(h=None) == EINVAL
        for bad in shared:
            assert f(**bad) == EINVAL, (f.__name__, bad)
    for bad in (dict(payload=None), dict(links=None), dict(buf=None), dict(status=None), dict(flags=2),
                dict(links=pad.data_ptr() + 2), dict(payload=r.buf.t.data_ptr() + 16, payload_bytes=64)):
        assert send_dev(**bad) == EINVAL, bad
    torch.cuda.synchronize()
    for x in (r.seg, r.desc, r.res, r.total, r.buf, r.status, r.work):
        assert (x.read("after refused calls") == SENT).all()        # nothing launched, nothing written

    # the host call: the same checks on host pointers
    hb = host_buffers(bursts, kw)

    def host(**kw2):
        a = dict(dict(burst=bursts.ctypes.data, n_burst=len(bursts), payload=payload.ctypes.data,
                      payload_bytes=payload.nbytes, links=links.ctypes.data, n_links=3, buf=hb["buf"].ctypes.data,
                      buf_off=64, buf_len=kw["buf_len"], off_shift=6, slot_bytes=0, max_mss=0, flags=0,
                      desc=hb["desc"].ctypes.data, seg_cap=kw["seg_cap"], res=hb["res"].ctypes.data,
                      total=hb["total"].ctypes.data, status=hb["status"].ctypes.data), **kw2)
        return L.mtcp_gpu_tx_send(ctx._h, *a.values())

    for bad in (dict(burst=None), dict(payload=None), dict(links=None), dict(buf=None), dict(desc=None),
                dict(res=None), dict(total=None), dict(status=None), dict(off_shift=17), dict(n_links=0),
                dict(n_links=257), dict(seg_cap=0), dict(seg_cap=(1 << 26) + 1), dict(n_burst=(1 << 24) + 1),
                dict(slot_bytes=1000), dict(buf_off=32), dict(flags=2),
                dict(payload=hb["buf"].ctypes.data + 8, payload_bytes=8)):
        assert host(**bad) == EINVAL, bad
    assert all((a == SENT).all() for a in hb.values())
    # the host plan and the workspace size
    assert L.mtcp_gpu_tx_segment_plan(None, 1, 0, 1, 0, 0, 0, 0, 1, 0, None, None) == EINVAL
    assert L.mtcp_gpu_tx_segment_work_bytes((1 << 24) + 1) == 0
    # the calls above left the context usable
    assert send_dev() == 0
    *got, image, status = r.read()
    assert_records(got, want, "after the refused calls")
    assert not status[:int(want[3][0])].any()


def host_buffers(bursts, kw):
    return dict(buf=np.full(kw["buf_len"], SENT, np.uint8), desc=np.full(kw["seg_cap"] * 8, SENT, np.uint8),
                res=np.full(len(bursts) * 16, SENT, np.uint8), total=np.full(16, SENT, np.uint8),
                status=np.full(kw["seg_cap"], SENT, np.uint8))
