"""Every rx / tx kernel over the deterministic edge batches of
tests/edge_frames.py, on the MI355X, bit-exact against the oracle (which
tests/test_edge_frames.py pins on the reference's own code for these frames).

The batches put frames on the kernels' own boundaries — every chunk count
k * g - 1, k * g, k * g + 1 of each kernel's granule g at every even start
phase, every (ihl, doff, phase) header geometry, Ethernet padding on both
sides of the wave kernel's fast path, every ICMP length, checksums whose
correct value is 0x0000, descriptor positions at and past 2^32 at off_shift
0..16 — inside non-zero, non-0xFF garbage, so that a byte read too many or too
few changes a checksum.  Each of the six MTCP_GPU_SCHED kernels runs each
family in chunk mode (with RSS and the fused flow bins) and as a pointer
burst; mtcp_gpu_last_kernel shows that rx_kernel's four schedules and both
wave instantiations ran the sweep.  No frame is left out of any comparison."""
import functools

import numpy as np
import pytest

import oracle
from mtcp_amd import RESULT16_DTYPE, RESULT_DTYPE, compact_of
from tests import edge_frames as ef
from tests.test_gpu_parity import DEV, assert_same, dev_results, run_rx_dev, to_dev
from tests.test_gpu_wave import SCHEDS, ctx_for, ptr_burst

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

RSS = dict(rss=True, rss_queues=8, rss_endian=True)
SMALL = {"row": "rx_group_kernel<row>", "quad": "rx_group_kernel<quad>", "oct": "rx_group_kernel<oct>",
         "span": "rx_span_kernel"}
# the kernel a forced schedule must reach on a family in chunk mode
# (dispatch.hpp big_schedule / kWaveShortUpToSlot; tests/test_edge_frames.py
# test_slot_conditions holds the families' average slots there)
CHUNK_KERNEL = {("big", "S"): "rx_kernel<sorted>", ("big", "Mt"): "rx_kernel<unrolled>",
                ("big", "J"): "rx_kernel<unrolled,line-aligned>",
                ("wave", "M"): "rx_wave_kernel<2 loads>", ("wave", "J"): "rx_wave_kernel<10 loads>"}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")
    from mtcp_amd import gpu as g
    return g


def expect_kernel(sched, name, ptrs, got):
    if sched in SMALL:
        assert got == SMALL[sched], got
    elif sched == "wave":
        assert got == ("rx_wave_kernel<2 loads>" if ptrs else CHUNK_KERNEL.get((sched, name), got)), got
        assert got.startswith("rx_wave_kernel<"), got
    else:
        assert got == ("rx_kernel<sorted,line-aligned>" if ptrs else CHUNK_KERNEL.get((sched, name), got)), got
        assert got.startswith("rx_kernel<"), got


def assert_same16(got, want, what):
    for f in RESULT16_DTYPE.names:
        diff = np.nonzero(got[f] != want[f])[0]
        assert len(diff) == 0, f"{what} field {f}: {len(diff)} mismatches, first #{diff[0]}"


def rx_family(gpu, monkeypatch, sched, name, compact=False, burst=True):
    buf, desc = ef.get(name)
    n = len(desc)
    want = ef.oracle_rx(name)
    want_bins = oracle.flow_bins(want)
    rec, dt = (16, RESULT16_DTYPE) if compact else (40, RESULT_DTYPE)
    same = assert_same16 if compact else assert_same
    want_rec = compact_of(want) if compact else want
    with ctx_for(gpu, monkeypatch, sched, compact=compact, **RSS) as ctx:
        if not compact:
            same(run_rx_dev(ctx, buf, desc, 0), want_rec, f"{sched} {name} chunk")
            expect_kernel(sched, name, False, ctx.last_kernel)
        b, d = to_dev(buf), to_dev(desc)
        out = torch.full((n * rec,), 0xEE, dtype=torch.uint8, device=DEV)
        bins = torch.full((n,), 7, dtype=torch.int32, device=DEV)
        ctx.rx_chunk_flow_dev(b, d, n, 0, out, bins)
        torch.cuda.synchronize()
        expect_kernel(sched, name, False, ctx.last_kernel)
        same(out.cpu().numpy().view(dt), want_rec, f"{sched} {name} chunk + bins")
        assert np.array_equal(bins.cpu().numpy().view(np.uint32), want_bins), f"{sched} {name} chunk bins"
        if burst:
            ptrs, lens = ptr_burst(b, desc)
            out.fill_(0xEE)
            bins.fill_(7)
            ctx.rx_ptrs_flow_dev(ptrs, lens, n, out, bins)
            torch.cuda.synchronize()
            expect_kernel(sched, name, True, ctx.last_kernel)
            same(out.cpu().numpy().view(dt), want_rec, f"{sched} {name} pointers + bins")
            assert np.array_equal(bins.cpu().numpy().view(np.uint32), want_bins), f"{sched} {name} pointer bins"
            out.fill_(0xEE)
            ctx.rx_ptrs_dev(ptrs, lens, n, out)
            torch.cuda.synchronize()
            same(out.cpu().numpy().view(dt), want_rec, f"{sched} {name} pointers")


@pytest.mark.parametrize("name", ["S", "M", "J", "H", "P", "I", "Z", "Zf"])
@pytest.mark.parametrize("sched", SCHEDS)
def test_rx_edge_family(gpu, monkeypatch, sched, name):
    rx_family(gpu, monkeypatch, sched, name)


@pytest.mark.parametrize("name", ["H", "J"])
@pytest.mark.parametrize("sched", SCHEDS)
def test_rx_edge_family_compact(gpu, monkeypatch, sched, name):
    rx_family(gpu, monkeypatch, sched, name, compact=True)


def test_rx_unrolled_schedule_on_tiled_sweep(gpu, monkeypatch):
    """More than 65 536 frames of 1 024..1 536 B average slots: the only way
    to rx_kernel's unrolled rounds (1 536 B trips, M's 2 048..4 130 B frames on
    two and three of them)."""
    rx_family(gpu, monkeypatch, "big", "Mt", burst=False)


# ---- tx fill -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tx_case(name):
    """A family with the check fields of a third of its frames set to 0x0000,
    a third to 0xFFFF and a third to random values; the oracle's fill of it
    and the number of frames it fills."""
    buf, desc = ef.get(name)
    src = buf.copy()
    rng = np.random.default_rng(2000 + len(desc))
    o = desc["offset"].astype(np.int64)
    tcp = o + 14 + 4 * (src[o + 14] & 15).astype(np.int64) + 16
    fits = tcp + 2 <= o + desc["len"]
    kind = np.arange(len(desc)) % 3
    for at, ok in ((o + 24, np.ones(len(desc), bool)), (tcp, fits)):
        for j in (0, 1):
            r = rng.integers(0, 256, len(desc), dtype=np.uint8)
            v = np.where(kind == 0, 0, np.where(kind == 1, 0xFF, r)).astype(np.uint8)
            src[(at + j)[ok]] = v[ok]
    want = src.copy()
    filled = oracle.tx_fill(want, desc, 0)
    for a in (src, want):
        a.setflags(write=False)
    return src, want, filled


def tx_family(gpu, monkeypatch, sched, name, host=True):
    _, desc = ef.get(name)
    src, want, filled = tx_case(name)
    n = len(desc)
    # the frames the fill takes are the family's well-formed ones: those rx answers TCP_OK for
    assert filled == (ef.oracle_rx(name)["verdict"] == 0).sum() > 0
    with ctx_for(gpu, monkeypatch, sched) as ctx:
        b = to_dev(src)
        ctx.tx_fill_dev(b, to_dev(desc), n, 0)
        torch.cuda.synchronize()
        # (the span kernel is rx only: a forced span fills on rx_kernel)
        assert ctx.last_kernel.startswith({"wave": "rx_wave_kernel<", "span": "rx_kernel<", "big": "rx_kernel<"}
                                          .get(sched) or SMALL[sched]), ctx.last_kernel
        if (sched, name) == ("big", "Mt"):
            assert ctx.last_kernel == "rx_kernel<unrolled>"
        assert np.array_equal(b.cpu().numpy(), want), f"{sched} {name} tx_fill_dev"
        if host:
            h = src.copy()
            assert ctx.tx_fill(h, desc, 0) == filled
            assert np.array_equal(h, want), f"{sched} {name} tx_fill"
        if sched in ("wave", "row", "quad", "oct"):
            b = to_dev(src)
            ptrs, lens = ptr_burst(b, desc)
            ctx.tx_fill_ptrs_dev(ptrs, lens, n)
            torch.cuda.synchronize()
            assert np.array_equal(b.cpu().numpy(), want), f"{sched} {name} tx_fill_ptrs_dev"
            h = src.copy()
            assert ctx.tx_fill_ptrs(h, desc["offset"].astype(np.int64), desc["len"]) == filled
            assert np.array_equal(h, want), f"{sched} {name} tx_fill_ptrs"
    if name == "Z":
        o = desc["offset"].astype(np.int64)
        assert filled == n
        assert not want[np.concatenate([o + 24, o + 25, o + 50, o + 51])].any()


@pytest.mark.parametrize("name", ["S", "M", "J", "H", "P", "Z"])
@pytest.mark.parametrize("sched", SCHEDS)
def test_tx_edge_family(gpu, monkeypatch, sched, name):
    """Only the check fields of the frames the oracle fills change (the whole
    buffer is compared), whatever they held before; Z's both fill to 0x0000."""
    tx_family(gpu, monkeypatch, sched, name)


def test_tx_unrolled_schedule_on_tiled_sweep(gpu, monkeypatch):
    tx_family(gpu, monkeypatch, "big", "Mt", host=False)


# ---- descriptors ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def d_tx_case(s):
    buf, desc, nv, _ = ef.get(f"D{s}")
    src = buf.copy()
    for o in desc["offset"][:nv].astype(np.int64) << s:
        src[[o + 24, o + 25, o + 50, o + 51]] = (0, 0xFF, 0xFF, 0)
    want = src.copy()
    assert oracle.tx_fill(want, desc, s) == nv
    assert np.array_equal(want, buf)
    return src, want


@pytest.mark.parametrize("s", ef.SHIFTS)
@pytest.mark.parametrize("sched", SCHEDS)
def test_descriptor_arithmetic_every_kernel(gpu, monkeypatch, sched, s):
    """offset << off_shift in 64 bits in every kernel: positions at and past
    2^32 (which truncate onto valid frames), offset 0xFFFFFFFF, the frame
    ending at buf_len and the ones past it; the tx fill touches no refused
    descriptor's bytes."""
    buf, desc, nv, cases = ef.get(f"D{s}")
    want = ef.oracle_rx(f"D{s}")
    src, filled = d_tx_case(s)
    n = len(desc)
    with ctx_for(gpu, monkeypatch, sched, **RSS) as ctx:
        out = dev_results(n)
        ctx.rx_chunk_dev(to_dev(buf), to_dev(desc), n, s, out)
        torch.cuda.synchronize()
        assert_same(out.cpu().numpy().view(RESULT_DTYPE), want, f"{sched} shift {s}: {cases}")
        b = to_dev(src)
        ctx.tx_fill_dev(b, to_dev(desc), n, s)
        torch.cuda.synchronize()
        assert np.array_equal(b.cpu().numpy(), filled), f"{sched} shift {s} tx"


@pytest.mark.parametrize("s", ef.SHIFTS)
def test_descriptor_arithmetic_host_paths(gpu, s):
    """mtcp_gpu_rx_chunk / mtcp_gpu_tx_fill (the streamed spans of sorted
    descriptors, the whole-chunk path of shuffled ones), with no wait limit
    and with a generous one (the bounce-buffer path)."""
    buf, desc, nv, _ = ef.get(f"D{s}")
    src, filled = d_tx_case(s)
    orders = {"sorted": np.argsort(desc["offset"], kind="stable"),
              "shuffled": np.random.default_rng(5 + s).permutation(len(desc))}
    for limit in (0, 30_000_000):
        for how, order in orders.items():
            d = np.ascontiguousarray(desc[order])
            want = oracle.rx_chunk(buf, d, s, oracle.rss_cfg(None, 8, 1))
            with gpu.Context(0, **RSS) as ctx:
                ctx.wait_limit = limit
                assert_same(ctx.rx_chunk(buf, d, s), want, f"host rx shift {s} {how} limit {limit}")
                h = src.copy()
                assert ctx.tx_fill(h, d, s) == nv
                assert np.array_equal(h, filled), f"host tx shift {s} {how} limit {limit}"


def test_host_rx_span_ending_off_the_chunk_grid(gpu):
    """A host chunk whose buf_len is no multiple of 16 and whose last frame
    ends at buf_len, after a larger call on the same context has left non-zero
    bytes behind the span in the stage: the last chunk's bytes past buf_len
    are whatever the stage holds, and must not count."""
    sbuf, sdesc = ef.get("S")
    ends = sdesc["offset"].astype(np.int64) + sdesc["len"]
    m = 1000 + int(np.nonzero(ends[1000:] % 16 == 9)[0][0]) + 1
    buf, desc = sbuf[:ends[m - 1]].copy(), sdesc[:m]
    assert len(buf) % 16 == 9
    rng = np.random.default_rng(77)
    junk = rng.integers(1, 255, 4 << 20, dtype=np.uint8)
    jd = np.zeros(4096, desc.dtype)
    jd["offset"] = np.arange(4096) * 1024
    jd["len"] = 1024
    rss = oracle.rss_cfg(None, 8, 1)
    want = oracle.rx_chunk(buf, desc, 0, rss)
    assert (want["verdict"] == 0).all()
    for limit in (0, 30_000_000):
        with gpu.Context(0, **RSS) as ctx:
            ctx.wait_limit = limit
            assert_same(ctx.rx_chunk(junk, jd, 0), oracle.rx_chunk(junk, jd, 0, rss), "garbage frames")
            assert_same(ctx.rx_chunk(buf, desc, 0), want, f"span ending at buf_len, limit {limit}")
    # and the shift-16 descriptor family behind the same garbage
    dbuf, ddesc, _, _ = ef.get("D16")
    d = np.ascontiguousarray(ddesc[np.argsort(ddesc["offset"], kind="stable")])
    with gpu.Context(0, **RSS) as ctx:
        ctx.rx_chunk(junk, jd, 0)
        assert_same(ctx.rx_chunk(dbuf, d, 16), oracle.rx_chunk(dbuf, d, 16, rss), "D16 after garbage")
