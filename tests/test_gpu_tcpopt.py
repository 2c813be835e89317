"""SURVEY §8 f5 on the GPU, through the C ABI (include/mtcp_gpu_tcpopt.h): the
per-packet option records of ParseTCPTimestamp (mtcp/src/tcp_util.c:61-92) and
ParseTCPOptions (tcp_util.c:14-59).  Expected values come from the golden
fixture the reference wrote (tests/golden/tcpopt_cases.bin) or from the
restatement pinned on it (tests/tcpopt_model.py), never from the kernel."""
import numpy as np
import pytest

import oracle
from mtcp_amd import DESC_DTYPE, RESULT_DTYPE, compact_of, pktgen
from tests import tcpopt_model as m

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL, EIO, ETIMEDOUT = -22, -5, -110
SENTINEL = 0xA5
OPT = m.TCPOPT_DTYPE
FLAG_CYCLE = (0x10, 0x02, 0x12, 0x18, 0x06, 0x04, 0x11)     # ACK, SYN, SYN|ACK, PSH|ACK, SYN|RST, RST, FIN|ACK


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")
    from mtcp_amd import gpu as g
    return g


def to_dev(a: np.ndarray):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(DEV)


def as_desc(desc) -> np.ndarray:
    return np.ascontiguousarray(desc).view(DESC_DTYPE) if desc.dtype != DESC_DTYPE else desc


def run_dev(gpu, ctx, buf: np.ndarray, desc: np.ndarray, mode: str = "chunk", res=None, d_buf=None,
            buf_len=None):
    """rx (unless `res`, forged records, is given) and the option launch over
    the frames, chunk or pointer mode.  Returns (records, option records) and
    checks that the option launch left the rx records and the bytes behind
    d_opt[n] alone."""
    n = len(desc)
    rec = ctx.record_size
    b = to_dev(buf) if d_buf is None else d_buf
    bv = b if buf_len is None else b[:buf_len]
    d_res = torch.zeros(n * rec, dtype=torch.uint8, device=DEV) if res is None else to_dev(res)
    d_opt = torch.full(((n + 4) * 16,), SENTINEL, dtype=torch.uint8, device=DEV)
    if mode == "chunk":
        d = to_dev(as_desc(desc))
        if res is None:
            ctx.rx_chunk_dev(bv, d, n, 0, d_res)
    else:
        assert buf_len is None
        ptrs = torch.from_numpy(desc["offset"].astype(np.int64) + b.data_ptr()).to(DEV)
        lens = torch.from_numpy(desc["len"].astype(np.int16)).to(DEV)
        if res is None:
            ctx.rx_ptrs_dev(ptrs, lens, n, d_res)
    torch.cuda.synchronize()
    before = d_res.cpu().numpy().copy()
    if mode == "chunk":
        ctx.rx_tcpopt_chunk_dev(bv, d, n, 0, d_res, d_opt)
    else:
        ctx.rx_tcpopt_ptrs_dev(ptrs, lens, n, d_res, d_opt)
    torch.cuda.synchronize()
    assert np.array_equal(d_res.cpu().numpy(), before), "the option launch changed the rx records"
    raw = d_opt.cpu().numpy()
    assert (raw[n * 16:] == SENTINEL).all(), "bytes behind d_opt[n] were written"
    return before.view(ctx.result_dtype), raw[:n * 16].view(OPT)


def assert_records(got, want, what):
    bad = np.nonzero(got.view(np.uint8).reshape(-1, 16) != want.view(np.uint8).reshape(-1, 16))[0]
    assert len(bad) == 0, (what, len(np.unique(bad)), int(bad[0]), got[bad[0]], want[bad[0]])


# ---- the fixture as frames -----------------------------------------------------
class FixtureFrames:
    """The fixture's cases as frames with ihl 5: the case's block as the
    options, the rest of its 56 bytes behind them, so that every byte a walk
    reads is the byte the reference read.  tcp_flags cycle through
    FLAG_CYCLE; every third frame's tot_len ends with the options (what
    follows lies past 14 + ip_len but inside the frame)."""

    def __init__(self):
        self.cases = m.load_fixture()
        frames, self.flags = [], []
        for k, c in enumerate(self.cases):
            length, fl = int(c["len"]), FLAG_CYCLE[k % len(FLAG_CYCLE)]
            ip_len = 40 + length if k % 3 == 0 else None
            frames.append(m.frame_bytes(c["bytes"], length, bytes(c["bytes"][length:]), 5, fl, ip_len, seed=k))
            self.flags.append(fl)
        self.buf, self.desc = m.pack_chunk(frames)
        assert m.fill_checksums(self.buf, self.desc) == len(frames)
        self.want = np.zeros(len(frames), dtype=OPT)
        for k, c in enumerate(self.cases):
            self.want[k] = m.record_of_case(c, self.flags[k], m.BLOCK)
        self.res = oracle.rx_chunk(self.buf, self.desc.astype(oracle.DESC_DTYPE), 0)
        assert (self.res["verdict"] == 0).all()


@pytest.fixture(scope="module")
def fx():
    return FixtureFrames()


def test_fixture_frames_cover_both_walks(fx):
    f = fx.want["flags"]
    for bit in (m.TS_FOUND, m.MSS, m.WSCALE, m.SACK_PERMIT, m.SAW_TS, m.TS_UNPINNED, m.SYN_UNPINNED):
        assert ((f & bit) != 0).sum() >= 30, hex(bit)
    assert (f & 0x10 == 0).all()


@pytest.mark.parametrize("mode", ["chunk", "ptrs"])
@pytest.mark.parametrize("compact", [False, True])
def test_fixture_parity(gpu, fx, mode, compact):
    with gpu.Context(0, compact=compact) as ctx:
        res, got = run_dev(gpu, ctx, fx.buf, fx.desc, mode)
    want_res = compact_of(fx.res) if compact else fx.res
    assert res.tobytes() == want_res.view(ctx.result_dtype).tobytes()      # rx itself: the oracle's records
    assert_records(got, fx.want, f"fixture {mode} compact={compact}")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4097])
def test_batch_edges(gpu, fx, n):
    with gpu.Context(0) as ctx:
        _, got = run_dev(gpu, ctx, fx.buf, fx.desc[:n], "chunk" if n % 2 else "ptrs")
    assert_records(got, fx.want[:n], f"n={n}")


def generated_expectation(host: np.ndarray, desc: np.ndarray, res: np.ndarray) -> np.ndarray:
    """Option records of a pktgen batch, from its two shapes (pktgen.hip
    gen_headers after tcp_out.c:185-192): doff 8 with NOP NOP TS(10) at frame
    bytes 54..65, or doff 5; flags ACK [| PSH]: the timestamp walk only."""
    want = np.zeros(len(desc), dtype=OPT)
    ok = res["verdict"] == 0
    assert set(np.unique(res["ihl_doff"][ok])) <= {0x55, 0x85}
    assert (res["tcp_flags"][ok] & 0x06 == 0).all()
    ts = np.nonzero(ok & (res["ihl_doff"] == 0x85))[0]
    pos = (desc["offset"][ts].astype(np.int64) << 6)[:, None] + np.arange(54, 66)
    b = host[pos].astype(np.uint32)
    assert (b[:, 0:4] == (1, 1, 8, 10)).all()
    want["ts_val"][ts] = (b[:, 4] << 24) | (b[:, 5] << 16) | (b[:, 6] << 8) | b[:, 7]
    want["ts_ref"][ts] = (b[:, 8] << 24) | (b[:, 9] << 16) | (b[:, 10] << 8) | b[:, 11]
    want["flags"][ts] = m.TS_FOUND
    return want


@pytest.mark.parametrize("compact", [False, True])
def test_generated_bimodal_batch(gpu, compact):
    n, seed = 65536 + 17, 7
    desc, nbytes = pktgen.layout(n, "bimodal", 6, seed)
    b = torch.zeros((nbytes + 15) & ~15, dtype=torch.uint8, device=DEV)
    d = to_dev(desc)
    gpu.pktgen_dev(b, d, n, 6, seed)
    with gpu.Context(0, compact=compact) as ctx:
        d_res = torch.zeros(n * ctx.record_size, dtype=torch.uint8, device=DEV)
        d_opt = torch.full(((n + 4) * 16,), SENTINEL, dtype=torch.uint8, device=DEV)
        ctx.rx_chunk_dev(b, d, n, 6, d_res)
        ctx.rx_tcpopt_chunk_dev(b, d, n, 6, d_res, d_opt)
        torch.cuda.synchronize()
        res = d_res.cpu().numpy().view(ctx.result_dtype)
    raw = d_opt.cpu().numpy()
    assert (raw[n * 16:] == SENTINEL).all()
    host = b.cpu().numpy()
    ores = oracle.rx_chunk(host, desc, 6)
    assert res.tobytes() == (compact_of(ores) if compact else ores).tobytes()
    want = generated_expectation(host, desc, ores)
    assert (want["flags"] == m.TS_FOUND).sum() > n // 5 and (ores["verdict"] != 0).sum() > 0
    assert_records(raw[:n * 16].view(OPT), want, "bimodal")


# ---- the frame's end -------------------------------------------------------------
EDGE_BLOCKS = [
    # (block, first trailing bytes): reads that run behind the option area
    ((1, 1, 1, 8), (0,)),                      # TS kind at len - 1, its length byte 0 at len: ts to len + 8
    ((1, 1, 8, 2), ()),                        # ts at len .. len + 7
    ((1, 1, 1, 2), (0,)),                      # MSS: length byte at len, its two bytes to len + 2
    ((1, 1, 1, 3), (1,)),                      # WSCALE: its byte at len + 1
    ((1, 1, 1, 30), ()),                       # a skipped kind: only its length byte at len
    ((1, 1, 8, 10, 1, 2, 3, 4, 5, 6, 7, 8), ()),   # the natural shape: nothing read behind
]


def frame_end_batch():
    rng = np.random.default_rng(3)
    frames, meta = [], []
    for block, lead in EDGE_BLOCKS:
        for k in range(11):
            for fl in (0x10, 0x02):
                trail = (bytes(lead) + rng.integers(0, 256, 16, dtype=np.uint8).tobytes())[:k]
                length = len(block)
                frames.append(m.frame_bytes(block, length, trail, 5, fl, seed=len(frames)))
                b = np.zeros(m.BLOCK + 16, np.uint8)
                b[:length + k] = np.frombuffer(bytes(block) + trail, np.uint8)
                meta.append((b, length, fl, length + k))
    # the frames stand back to back at even offsets: the bytes behind a frame
    # are its neighbour's headers, and the last frame ends the buffer's data
    starts, pos = [], 0
    for f in frames:
        starts.append(pos)
        pos += (len(f) + 1) & ~1
    buf, desc = m.pack_chunk(frames, starts, tail=16)
    assert m.fill_checksums(buf, desc) == len(frames)
    want = np.zeros(len(frames), dtype=OPT)
    for i, (b, length, fl, avail) in enumerate(meta):
        want[i] = m.expected_record(b, length, fl, avail)
    # the first block's timestamp walk: unpinned for k <= 8, found for k = 9, 10
    first = want["flags"][0:22:2]
    assert (first[:9] == m.TS_UNPINNED).all() and (first[9:] == m.TS_FOUND).all()
    assert ((want["flags"] & m.SYN_UNPINNED) != 0).sum() >= 5 and ((want["flags"] & m.MSS) != 0).sum() >= 5
    return buf, desc, want


@pytest.mark.parametrize("mode", ["chunk", "ptrs"])
def test_frame_end_edge(gpu, mode):
    """Frames that end exactly k bytes behind the option area, k = 0..10: a
    walk is unpinned exactly where the restatement reads at or past the end."""
    buf, desc, want = frame_end_batch()
    with gpu.Context(0) as ctx:
        res, got = run_dev(gpu, ctx, buf, desc, mode)
    assert (res["verdict"] == 0).all()
    assert_records(got, want, f"frame end {mode}")


# ---- placement -------------------------------------------------------------------
def placement_batch():
    """Every even start offset mod 128, ihl 5..15, doff 0..15, RST / SYN /
    neither, bodies that look like options whatever doff says; plus frames rx
    does not pass (bad checksum, ARP, truncated) filled the same way."""
    rng = np.random.default_rng(11)
    cases = m.load_fixture()
    frames, starts, pos = [], [], 0
    k = 0
    for rep in range(6):
        for s in range(0, 128, 2):
            ihl, doff, fl = 5 + k % 11, (k // 3) % 16, (0x10, 0x02, 0x04, 0x12)[k % 4]
            c = cases[(37 * k) % len(cases)]
            body = bytes(c["bytes"]) + bytes([1, 1, 8, 10]) + rng.integers(0, 256, 8, dtype=np.uint8).tobytes()
            f = m.frame_raw(ihl, doff, fl, body, seed=1000 + k)
            pos = ((pos + 127) & ~127) + s
            starts.append(pos)
            frames.append(f)
            pos += len(f)
            k += 1
    buf, desc = m.pack_chunk(frames, starts)
    m.fill_checksums(buf, desc)
    kinds = np.zeros(len(frames), np.uint8)
    for i in range(0, len(frames), 5):               # neighbours rx does not pass
        o, kind = int(desc["offset"][i]), 1 + (i // 5) % 3
        kinds[i] = kind
        if kind == 1:
            buf[o + 60] ^= 0x10                      # TCP (or IP options) checksum breaks
        elif kind == 2:
            buf[o + 12:o + 14] = (0x08, 0x06)        # ARP
        else:
            desc["len"][i] -= 2 * (1 + i % 9)        # the frame ends before 14 + ip_len
    return buf, desc, kinds


def expected_from_oracle(buf, desc, res):
    """Option records from the ORACLE's rx records (verdict, ihl, doff, flags)
    and the restatement over the frame bytes."""
    want = np.zeros(len(desc), dtype=OPT)
    for i, (d, r) in enumerate(zip(desc, res)):
        if r["verdict"] != 0:
            continue
        ihl, doff = int(r["ihl_doff"]) & 15, int(r["ihl_doff"]) >> 4
        first = int(d["offset"]) + 34 + 4 * ihl
        avail = int(d["offset"]) + int(d["len"]) - first
        b = np.zeros(64, np.uint8)
        take = max(0, min(64, avail))
        b[:take] = buf[first:first + take]
        want[i] = m.expected_record(b, 4 * doff - 20, int(r["tcp_flags"]), avail)
    return want


@pytest.mark.parametrize("mode", ["chunk", "ptrs"])
@pytest.mark.parametrize("compact", [False, True])
def test_placement(gpu, mode, compact):
    buf, desc, kinds = placement_batch()
    ores = oracle.rx_chunk(buf, desc.astype(oracle.DESC_DTYPE), 0)
    assert (ores["verdict"][kinds == 0] == 0).all()
    assert set(ores["verdict"][kinds == 1]) <= {4, 9}        # byte 60: IP options (ihl >= 12) or TCP
    assert (ores["verdict"][kinds == 2] == 2).all() and (ores["verdict"][kinds == 3] == 10).all()
    want = expected_from_oracle(buf, desc, ores)
    assert (want[kinds != 0].view(np.uint8) == 0).all()
    doff = ores["ihl_doff"] >> 4
    assert (want[doff <= 5].view(np.uint8) == 0).all() and set(np.unique(doff)) == set(range(16))
    assert set(np.unique(ores["ihl_doff"][kinds == 0] & 15)) == set(range(5, 16))
    assert (want["flags"] != 0).sum() > 60
    with gpu.Context(0, compact=compact) as ctx:
        res, got = run_dev(gpu, ctx, buf, desc, mode)
    wres = compact_of(ores) if compact else ores
    assert res.tobytes() == wres.view(ctx.result_dtype).tobytes()
    assert_records(got, want, f"placement {mode} compact={compact}")


def test_bad_descriptor_is_not_read(gpu, fx):
    """Descriptors that rx answers with BAD_DESC (past buf_len, odd) are not
    touched even when the record handed in says TCP_OK: valid frames with
    options stand behind buf_len, inside the allocation."""
    n, keep = 512, 256
    desc = fx.desc[:n].copy()
    valid_len = int(desc["offset"][keep])                 # a multiple of 128
    b = to_dev(fx.buf)
    want = fx.want[:n].copy()
    want[keep:] = np.zeros((), OPT)
    desc["offset"][5] += 1                                # an odd start
    want[5] = np.zeros((), OPT)
    with gpu.Context(0) as ctx:
        res, _ = run_dev(gpu, ctx, fx.buf, desc, "chunk", d_buf=b, buf_len=valid_len)
        assert (res["verdict"][keep:] == 11).all() and res["verdict"][5] == 11
        forged = fx.res[:n].copy()                        # every record says TCP_OK
        _, got = run_dev(gpu, ctx, fx.buf, desc, "chunk", res=forged, d_buf=b, buf_len=valid_len)
    assert (want[:keep]["flags"] != 0).sum() > 100
    assert_records(got, want, "bad descriptors")


# ---- the host call ---------------------------------------------------------------
def device_pair(gpu, ctx, host: np.ndarray, desc: np.ndarray, off_shift: int):
    n = len(desc)
    b, d = to_dev(host), to_dev(desc)
    d_res = torch.zeros(n * ctx.record_size, dtype=torch.uint8, device=DEV)
    d_opt = torch.zeros(n * 16, dtype=torch.uint8, device=DEV)
    ctx.rx_chunk_dev(b, d, n, off_shift, d_res)
    ctx.rx_tcpopt_chunk_dev(b, d, n, off_shift, d_res, d_opt)
    torch.cuda.synchronize()
    return d_res.cpu().numpy().view(ctx.result_dtype), d_opt.cpu().numpy().view(OPT)


@pytest.fixture(scope="module")
def big_batch(gpu):
    """Just over one 64 MiB stage: 1500 B frames in 1536 B slots."""
    n, seed = (64 << 20) // 1536 + 700, 19
    desc, nbytes = pktgen.layout(n, 1500, 6, seed)
    assert (64 << 20) < nbytes < (66 << 20)
    b = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    gpu.pktgen_dev(b, to_dev(desc), n, 6, seed)
    torch.cuda.synchronize()
    return b.cpu().numpy(), desc


@pytest.mark.parametrize("limit_us", [0, 10_000_000])
@pytest.mark.parametrize("case", ["sorted", "unsorted", "two_stages"])
def test_host_call(gpu, fx, big_batch, case, limit_us):
    if case == "two_stages":
        host, desc, shift = big_batch[0], big_batch[1], 6
    else:
        host, desc, shift = fx.buf, as_desc(fx.desc), 0
        if case == "unsorted":
            desc = np.ascontiguousarray(desc[np.random.default_rng(5).permutation(len(desc))])
    with gpu.Context(0, rss=True, rss_queues=4) as ctx:
        dres, dopt = device_pair(gpu, ctx, host, desc, shift)
        ctx.wait_limit = limit_us
        plain = ctx.rx_chunk(host, desc, shift)
        out, opts = ctx.rx_chunk_opts(host, desc, shift)
    assert out.tobytes() == plain.tobytes() == dres.tobytes()
    if case == "two_stages":
        want = generated_expectation(host, desc, oracle.rx_chunk(host, desc, 6))
    elif case == "unsorted":
        want = fx.want[np.random.default_rng(5).permutation(len(desc))]
    else:
        want = fx.want
    assert_records(dopt, want, f"{case}: device call")
    assert_records(opts, want, f"{case}: host call")


def test_host_call_compact(gpu, fx):
    with gpu.Context(0, compact=True) as ctx:
        out, opts = ctx.rx_chunk_opts(fx.buf, as_desc(fx.desc), 0)
    assert out.tobytes() == compact_of(fx.res).tobytes()
    assert_records(opts, fx.want, "host call, compact")


# ---- error returns -----------------------------------------------------------------
def test_error_returns(gpu, fx):
    from mtcp_amd._lib import lib
    L = lib()
    n = 64
    desc = as_desc(fx.desc[:n])
    b, d = to_dev(fx.buf), to_dev(desc)
    nbytes = b.numel()
    res = to_dev(fx.res[:n])
    opt = torch.full(((n + 1) * 16,), SENTINEL, dtype=torch.uint8, device=DEV)
    ptrs = torch.from_numpy(desc["offset"].astype(np.int64) + b.data_ptr()).to(DEV)
    lens = torch.from_numpy(desc["len"].astype(np.int16)).to(DEV)
    with gpu.Context(0) as ctx, gpu.Context(0, compact=True) as cctx:
        h, pb, pd, pr, po = ctx._h, b.data_ptr(), d.data_ptr(), res.data_ptr(), opt.data_ptr()
        pp, pl = ptrs.data_ptr(), lens.data_ptr()
        chunk, byptr = L.mtcp_gpu_rx_tcpopt_chunk_dev, L.mtcp_gpu_rx_tcpopt_ptrs_dev
        assert chunk(None, pb, nbytes, pd, n, 0, pr, po, None) == EINVAL
        assert chunk(h, None, nbytes, pd, n, 0, pr, po, None) == EINVAL
        assert chunk(h, pb, nbytes, None, n, 0, pr, po, None) == EINVAL
        assert chunk(h, pb, nbytes, pd, n, 0, None, po, None) == EINVAL
        assert chunk(h, pb, nbytes, pd, n, 0, pr, None, None) == EINVAL
        assert chunk(h, pb + 2, nbytes, pd, n, 0, pr, po, None) == EINVAL      # 16 B base
        assert chunk(h, pb, nbytes + 8, pd, n, 0, pr, po, None) == EINVAL      # length % 16
        assert chunk(h, pb, nbytes, pd, n, 17, pr, po, None) == EINVAL         # off_shift
        assert chunk(h, pb, nbytes, pd + 4, n, 0, pr, po, None) == EINVAL      # desc align
        assert chunk(h, pb, nbytes, pd, n, 0, pr + 4, po, None) == EINVAL      # 40 B records: 8 B
        assert chunk(h, pb, nbytes, pd, n, 0, pr, po + 8, None) == EINVAL      # d_opt: 16 B
        assert chunk(cctx._h, pb, nbytes, pd, n, 0, pr + 8, po, None) == EINVAL   # 16 B records: 16 B
        assert byptr(None, pp, pl, n, pr, po, None) == EINVAL
        assert byptr(h, None, pl, n, pr, po, None) == EINVAL
        assert byptr(h, pp, None, n, pr, po, None) == EINVAL
        assert byptr(h, pp, pl, n, None, po, None) == EINVAL
        assert byptr(h, pp, pl, n, pr, None, None) == EINVAL
        assert byptr(h, pp, pl, n, pr, po + 8, None) == EINVAL
        assert byptr(h, pp, pl, n, pr + 4, po, None) == EINVAL
        host_out = np.zeros(n, RESULT_DTYPE)
        host_opt = np.zeros(n, OPT)
        hb, hd = fx.buf, desc
        host = L.mtcp_gpu_rx_chunk_opts
        assert host(None, hb.ctypes.data, hb.nbytes, hd.ctypes.data, n, 0, host_out.ctypes.data,
                    host_opt.ctypes.data) == EINVAL
        assert host(h, hb.ctypes.data, hb.nbytes, hd.ctypes.data, n, 0, host_out.ctypes.data, None) == EINVAL
        assert host(h, hb.ctypes.data, hb.nbytes, hd.ctypes.data, n, 0, None, host_opt.ctypes.data) == EINVAL
        assert host(h, hb.ctypes.data, hb.nbytes, hd.ctypes.data, n, 17, host_out.ctypes.data,
                    host_opt.ctypes.data) == EINVAL
        # empty batches: no launch, null pointers allowed
        assert chunk(h, None, 0, None, 0, 0, None, None, None) == 0
        assert byptr(h, None, None, 0, None, None, None) == 0
        assert host(h, None, 0, None, 0, 0, None, None) == 0
        torch.cuda.synchronize()
        assert (opt.cpu().numpy() == SENTINEL).all()                           # nothing was launched
        # the context still works after the rejections
        assert chunk(h, pb, nbytes, pd, n, 0, pr, po, None) == 0
        ctx.sync()
    raw = opt.cpu().numpy()
    assert_records(raw[:n * 16].view(OPT), fx.want[:n], "after the rejections")
    assert (raw[n * 16:] == SENTINEL).all()


def test_abandoned_context_answers_eio_and_writes_nothing(gpu, fx):
    """mtcp_gpu_rx_chunk_opts behind a stall, past the wait limit:
    MTCP_GPU_ETIMEDOUT, neither out nor opts written then or after the stall
    has ended; the option entry points of the abandoned context answer
    MTCP_GPU_EIO without a launch."""
    from mtcp_amd._lib import lib
    from tests.test_gpu_bounded import stall_lib, stream_wait
    L, T = lib(), stall_lib()
    n = 2048
    desc = as_desc(fx.desc[:n])
    ctx = gpu.Context(0)
    handle = ctx.stream
    out, opts = ctx.rx_chunk_opts(fx.buf, desc, 0)          # unbounded first: stages sized, kernels loaded
    assert_records(opts, fx.want[:n], "before the stall")
    ctx.wait_limit = 20_000
    out = np.full(n * 40, SENTINEL, np.uint8)
    opts = np.full(n * 16, SENTINEL, np.uint8)
    assert T.mtcp_gpu_debug_stall(ctx._h, 250_000) == 0
    rc = L.mtcp_gpu_rx_chunk_opts(ctx._h, fx.buf.ctypes.data, fx.buf.nbytes, desc.ctypes.data, n, 0,
                                  out.ctypes.data, opts.ctypes.data)
    assert rc == ETIMEDOUT, rc
    b, d, res = to_dev(fx.buf), to_dev(desc), to_dev(fx.res[:n])
    d_opt = torch.full((n * 16,), SENTINEL, dtype=torch.uint8, device=DEV)
    assert L.mtcp_gpu_rx_tcpopt_chunk_dev(ctx._h, b.data_ptr(), b.numel(), d.data_ptr(), n, 0, res.data_ptr(),
                                          d_opt.data_ptr(), None) == EIO
    ptrs = torch.from_numpy(desc["offset"].astype(np.int64) + b.data_ptr()).to(DEV)
    lens = torch.from_numpy(desc["len"].astype(np.int16)).to(DEV)
    assert L.mtcp_gpu_rx_tcpopt_ptrs_dev(ctx._h, ptrs.data_ptr(), lens.data_ptr(), n, res.data_ptr(),
                                         d_opt.data_ptr(), None) == EIO
    assert L.mtcp_gpu_rx_chunk_opts(ctx._h, fx.buf.ctypes.data, fx.buf.nbytes, desc.ctypes.data, n, 0,
                                    out.ctypes.data, opts.ctypes.data) == EIO
    ctx.close()
    stream_wait(handle)                                     # the stall and what was queued behind it end
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and (opts == SENTINEL).all()
    assert (d_opt.cpu().numpy() == SENTINEL).all()
