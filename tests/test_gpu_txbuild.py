"""The frame builder on the GPU (include/mtcp_gpu_txbuild.h, mtcp_amd/csrc/
txbuild_kernels.hpp): every byte of every buffer is compared against the
frames the reference wrote (tests/golden/txbuild_frames.*.bin), the model
(tests/txbuild_model.py) or the oracle, never against the kernel's own output.

All four kernel shapes run every device case: the shape goes by
payload_bytes / n, so unused bytes in front of the payload buffer's first
segment (`lead`) move a batch from the row shape to the half-wave and the wave
shape without changing a frame, and ACKs without payload appended behind the
batch (`shaped`) bring it down to the 8-lane shape."""
import time

import numpy as np
import pytest

import oracle
from mtcp_amd import DESC_DTYPE, RESULT_DTYPE, TCPOPT_DTYPE
from tests import tcpopt_model, txbuild_model as m

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EINVAL, EIO, ETIMEDOUT = -22, -5, -110
GUARD = 4096
SENT = 0xA5
SLOT = 2048
OCT, ROW, HALF, WAVE = ("txbuild_kernel<oct>", "txbuild_kernel<row>", "txbuild_kernel<half>",
                        "txbuild_kernel<wave>")
SHAPES = [OCT, ROW, HALF, WAVE]
OCT_UP_TO, ROW_UP_TO, HALF_UP_TO = 48, 384, 4096     # dispatch.hpp kTxBuild*UpToPayload
PAD_SLOT = 128


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
def fixture_case():
    """The reference's 4 054 frames as segments (garbage in the fields the
    builders never read), and the expected image of 2 048 B slots."""
    frames = m.load_fixture()
    seg, payload, links = m.segs_from_frames(frames)
    seg = m.garbage_unread_fields(seg)
    lens = np.array([len(f) for f in frames])
    want = np.full(SLOT * len(frames), SENT, dtype=np.uint8)
    for i, f in enumerate(frames):
        want[i * SLOT:i * SLOT + len(f)] = f
    want.flags.writeable = False
    return seg, payload, links, lens, want


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)


def lead_for(shape, seg, payload):
    """Unused bytes in front of the payload that give the batch `shape`."""
    n, total = len(seg), len(payload)
    if shape == OCT:
        assert total // n <= OCT_UP_TO, "shaped() appends the ACKs that make this an 8-lane batch"
        return 0
    if shape == ROW:
        assert total // n <= ROW_UP_TO, "this batch is no row batch as it is"
        return max(0, (OCT_UP_TO + 1) * n - total)
    if shape == HALF:
        assert total // n <= HALF_UP_TO, "this batch is a wave batch as it is"
        return max(0, (ROW_UP_TO + 1) * n - total)
    return max(0, (HALF_UP_TO + 1) * n - total)


def shaped(shape, seg, payload, links, desc, nbytes, off_shift=0):
    """The batch as `shape` runs it: (seg, desc, nbytes, lead).  For the
    8-lane shape ACKs without payload follow the batch, their 128 B slots
    behind its image, until payload_bytes / n is small enough."""
    if shape != OCT or len(payload) // len(seg) <= OCT_UP_TO:
        return seg, desc, nbytes, lead_for(shape, seg, payload)
    k = len(payload) // OCT_UP_TO + 1 - len(seg)
    rng = np.random.default_rng(k)
    pad = np.zeros(k, dtype=m.SEG_DTYPE)
    pad["flags"] = m.ACK
    pad["saddr"], pad["daddr"], pad["seq"], pad["ack"] = rng.integers(1, 1 << 32, (4, k), dtype=np.uint64)
    pad["sport"], pad["dport"], pad["window"], pad["ip_id"] = rng.integers(1, 1 << 16, (4, k))
    first = (nbytes + 127) // 128 * 128
    pdesc = m.slots([66] * k, PAD_SLOT, off_shift, first=first)
    return np.concatenate([seg, pad]), np.concatenate([desc, pdesc]), first + PAD_SLOT * k, 0


def assert_pads(image, status, seg, links, n, nbytes, no_csum=False):
    """The appended ACKs' part of a shaped batch against the model."""
    if len(seg) == n:
        return
    assert not status[n:].any()
    first = (nbytes + 127) // 128 * 128
    assert (image[nbytes:first] == SENT).all()
    got = image[first:].reshape(-1, PAD_SLOT)
    assert np.array_equal(got[:, :66], m.build_uniform(seg[n:], np.zeros(0, np.uint8), links, no_csum))
    assert (got[:, 66:] == SENT).all()


def repack(seg, payload):
    """The segments' payloads back to back with gaps of 0..2 bytes (every
    source alignment), the buffer ending at the last segment's last byte."""
    seg = seg.copy()
    ends, at = [], 1
    for i, s in enumerate(seg):
        ends.append((at, int(s["payload_off"]), int(s["payload_len"])))
        at += int(s["payload_len"]) + i % 3
    last = ends[-1][0] + ends[-1][2]
    out = np.zeros(last, dtype=np.uint8)
    for (to, frm, ln), s in zip(ends, seg):
        out[to:to + ln] = payload[frm:frm + ln]
        s["payload_off"] = to
    return seg, out


class Built:
    """One device run: guards of 0xA5 around the image, the payload buffer
    ending exactly at its last byte."""

    def __init__(self, ctx, seg, payload, links, desc, nbytes, off_shift=0, max_mss=0, flags=0, lead=0, stream=None):
        self.n, self.nbytes = len(seg), nbytes
        seg = seg.copy()
        seg["payload_off"] += lead
        self.d_seg, self.d_links, self.d_desc = up(seg), up(links), up(desc)
        self.d_payload = up(np.concatenate([np.zeros(lead, np.uint8), payload]))
        self.whole = torch.full((GUARD + nbytes + GUARD,), SENT, dtype=torch.uint8, device=DEV)
        self.d_buf = self.whole[GUARD:GUARD + nbytes]
        self.d_status = torch.full((self.n + GUARD,), SENT, dtype=torch.uint8, device=DEV)
        self.args = (ctx, off_shift, max_mss, flags, stream)
        torch.cuda.synchronize()             # the fills above are done before a launch on another stream

    def launch(self):
        ctx, off_shift, max_mss, flags, stream = self.args
        ctx.tx_build_dev(self.d_seg, self.n, self.d_payload, self.d_links, self.d_buf, self.d_desc, off_shift,
                         self.d_status[:self.n], max_mss=max_mss, flags=flags, stream=stream)

    def read(self):
        torch.cuda.synchronize()
        whole, status = self.whole.cpu().numpy(), self.d_status.cpu().numpy()
        assert (whole[:GUARD] == SENT).all() and (whole[GUARD + self.nbytes:] == SENT).all(), "guard written"
        assert (status[self.n:] == SENT).all()
        return whole[GUARD:GUARD + self.nbytes], status[:self.n]


def build(ctx, shape, seg, payload, links, desc, nbytes, **kw):
    """(image, status) of the batch run as `shape`; what `shaped` appended is
    checked here and cut off."""
    n = len(seg)
    seg2, desc2, nbytes2, lead = shaped(shape, seg, payload, links, desc, nbytes, kw.get("off_shift", 0))
    b = Built(ctx, seg2, payload, links, desc2, nbytes2, lead=lead, **kw)
    b.launch()
    image, status = b.read()
    assert ctx.last_kernel == shape
    assert_pads(image, status, seg2, links, n, nbytes, bool(kw.get("flags", 0) & m.NO_CSUM))
    return image[:nbytes], status[:n]


def assert_image(got, want, desc, off_shift, what):
    if np.array_equal(got, want):
        return
    bad = np.flatnonzero(got != want)
    offs = desc["offset"].astype(np.int64) << off_shift
    i = int(np.searchsorted(offs, bad[0], side="right")) - 1
    raise AssertionError(f"{what}: {len(bad)} bytes differ, first at byte {bad[0]} "
                         f"(segment {i}, frame byte {bad[0] - offs[i]}, len {desc['len'][i]})")


# ---- 1. the reference's frames --------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("off_shift", [6, 0])
def test_fixture_frames(ctx, fixture_case, shape, off_shift):
    seg, payload, links, lens, want = fixture_case
    desc = m.slots(lens, SLOT, off_shift)
    image, status = build(ctx, shape, seg, payload, links, desc, len(want), off_shift=off_shift)
    assert not status.any()
    assert_image(image, want, desc, off_shift, f"fixture {shape} shift {off_shift}")


# ---- 2. NO_CSUM, then the tx fill ------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_no_csum_then_tx_fill_gives_the_fixture(ctx, fixture_case, shape):
    seg, payload, links, lens, want = fixture_case
    desc = m.slots(lens, SLOT)
    n, nbytes = len(seg), len(want)
    seg2, desc2, nbytes2, lead = shaped(shape, seg, payload, links, desc, nbytes)
    b = Built(ctx, seg2, payload, links, desc2, nbytes2, flags=m.NO_CSUM, lead=lead)
    b.launch()
    bare, status = b.read()
    assert ctx.last_kernel == shape
    assert_pads(bare, status, seg2, links, n, nbytes, no_csum=True)
    bare, status = bare[:nbytes], status[:n]
    assert not status.any()
    offs = desc["offset"].astype(np.int64)
    assert not bare[offs + 24].any() and not bare[offs + 25].any()
    assert not bare[offs + 50].any() and not bare[offs + 51].any()
    zeroed = np.array(want)
    for k in (24, 25, 50, 51):
        zeroed[offs + k] = 0
    assert_image(bare, zeroed, desc, 0, "NO_CSUM")
    ctx.tx_fill_dev(b.d_buf, b.d_desc, b.n, 0)
    filled, status = b.read()
    assert_pads(filled, status, seg2, links, n, nbytes)
    assert_image(filled[:nbytes], want, desc, 0, "NO_CSUM + tx_fill")


# ---- 3. alignments ---------------------------------------------------------------------
STARTS = (0, 2, 4, 6, 8, 10, 12, 14, 62, 126)
PLENS = tuple(range(81)) + (127, 128, 129, 1023, 1024, 1025, 1447, 1448, 1449, 1459, 1460)
CROSS_PLENS = (0, 1, 2, 3, 15, 16, 17, 33, 130, 1025)


def sweep_case():
    """Every payload length x frame start x (form, SYN) with the source
    alignment cycling through 0..15, then every source alignment x frame
    start x (form, SYN) at ten lengths: 10 080 segments.  The payload
    buffer ends at the last segment's last byte."""
    rng = np.random.default_rng(5)
    combos = [(p, s, f, y, (7 * i + p) % 16) for i, (p, s, f, y) in enumerate(
        (p, s, f, y) for p in PLENS for s in STARTS for f in (0, 1) for y in (0, m.SYN))]
    combos += [(p, s, f, y, a) for p in CROSS_PLENS for a in range(16) for s in STARTS for f in (0, 1)
               for y in (0, m.SYN)]
    n = len(combos)
    seg = np.zeros(n, dtype=m.SEG_DTYPE)
    desc = np.zeros(n, dtype=DESC_DTYPE)
    seg["saddr"], seg["daddr"] = rng.integers(1, 1 << 32, (2, n), dtype=np.uint64)
    seg["sport"], seg["dport"], seg["window"], seg["ip_id"], seg["mss"] = rng.integers(1, 1 << 16, (5, n))
    seg["seq"], seg["ack"], seg["ts_val"], seg["ts_ecr"] = rng.integers(0, 1 << 32, (4, n), dtype=np.uint64)
    seg["wscale"], seg["link"] = rng.integers(0, 15, n), rng.integers(0, 2, n)
    src, dst, seen = 0, 0, set()
    for i, (plen, start, form, syn, align) in enumerate(combos):
        src += (align - src) % 16
        dst = (dst + 127) // 128 * 128 + start
        flags = syn | (m.ACK, m.ACK | m.PSH, 0, m.FIN | m.ACK)[i % 4]
        seg[i]["payload_off"], seg[i]["payload_len"], seg[i]["form"], seg[i]["flags"] = src, plen, form, flags
        desc[i]["offset"], desc[i]["len"] = dst, m.frame_len(flags, plen)
        seen.add((align, start))
        src += plen
        dst += int(desc[i]["len"])
    assert len(seen) == 160
    payload = rng.integers(0, 256, src, dtype=np.uint8)
    links = np.zeros(2, dtype=m.LINK_DTYPE)
    links["dst"], links["src"] = rng.integers(0, 256, (2, 6)), rng.integers(0, 256, (2, 6))
    nbytes = (dst + 15) // 16 * 16
    want, status = m.build_frames(seg, payload, links, desc, np.full(nbytes, SENT, np.uint8))
    assert not status.any()
    return seg, payload, links, desc, nbytes, want


@pytest.fixture(scope="module")
def sweep():
    return sweep_case()


@pytest.mark.parametrize("shape", SHAPES)
def test_alignment_sweep(ctx, sweep, shape):
    seg, payload, links, desc, nbytes, want = sweep
    image, status = build(ctx, shape, seg, payload, links, desc, nbytes)
    assert not status.any()
    assert_image(image, want, desc, 0, f"sweep {shape}")


# ---- 4. packed slots -------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_packed_slots(ctx, sweep, shape):
    """Frames back to back at even offsets: a store before a frame's start or
    past its end lands in a neighbour (or the guard)."""
    seg, payload, links, _, _, _ = sweep
    seg, payload = repack(seg[::3], payload)
    lens = m.frame_len(0, 0) + np.where(seg["flags"] & m.SYN, 8, 0) + seg["payload_len"].astype(np.int64)
    desc = np.zeros(len(seg), dtype=DESC_DTYPE)
    desc["offset"] = np.concatenate([[0], np.cumsum((lens + 1) & ~1)[:-1]]) + 2
    desc["len"] = lens
    nbytes = (int(desc["offset"][-1]) + int(lens[-1]) + 15) // 16 * 16
    want, status = m.build_frames(seg, payload, links, desc, np.full(nbytes, SENT, np.uint8))
    assert not status.any() and (lens & 1).any()
    image, status = build(ctx, shape, seg, payload, links, desc, nbytes)
    assert not status.any()
    assert_image(image, want, desc, 0, f"packed {shape}")


# ---- 5. jumbo payloads and the length limit ----------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_jumbo_and_the_length_limit(ctx, shape):
    rng = np.random.default_rng(9)
    n, slot, mss = 64 + 4, 9216, 8960
    seg = np.zeros(n, dtype=m.SEG_DTYPE)
    seg["payload_len"] = 8948
    seg["flags"] = np.where(np.arange(n) % 5 == 0, m.SYN, m.ACK)
    seg["form"] = np.arange(n) % 2
    # at the limit and one byte past it, without and with SYN
    seg["flags"][64:] = (m.ACK, m.ACK, m.SYN, m.SYN)
    seg["payload_len"][64:] = (mss + 12, mss + 13, mss + 20, mss + 21)
    seg["saddr"], seg["daddr"] = rng.integers(1, 1 << 32, (2, n), dtype=np.uint64)
    seg["sport"], seg["dport"], seg["window"], seg["ip_id"], seg["mss"] = rng.integers(1, 1 << 16, (5, n))
    seg["seq"], seg["ack"], seg["ts_val"], seg["ts_ecr"] = rng.integers(0, 1 << 32, (4, n), dtype=np.uint64)
    seg["payload_off"] = 3 + np.arange(n) * 8999
    payload = rng.integers(0, 256, int(seg["payload_off"][-1]) + int(seg["payload_len"][-1]), dtype=np.uint8)
    links = np.zeros(1, dtype=m.LINK_DTYPE)
    links["dst"], links["src"] = rng.integers(0, 256, (1, 6)), rng.integers(0, 256, (1, 6))
    desc = m.slots([m.frame_len(int(s["flags"]), int(s["payload_len"])) for s in seg], slot, first=2)
    nbytes = slot * n
    want, wstat = m.build_frames(seg, payload, links, desc, np.full(nbytes, SENT, np.uint8), max_mss=mss)
    assert wstat[64:].tolist() == [m.BUILT, m.BAD_SEG, m.BUILT, m.BAD_SEG] and not wstat[:64].any()
    if shape in (ROW, HALF):    # a jumbo batch is a wave batch: ACKs without payload bring the average down
        pad = np.zeros(n * (40 if shape == ROW else 3), dtype=m.SEG_DTYPE)
        pad["flags"], pad["saddr"], pad["daddr"] = m.ACK, 1, 2
        pdesc = m.slots([66] * len(pad), 128, first=nbytes)
        seg, desc = np.concatenate([seg, pad]), np.concatenate([desc, pdesc])
        want, wstat = m.build_frames(seg, payload, links, desc,
                                     np.full(nbytes + 128 * len(pad), SENT, np.uint8), max_mss=mss)
        nbytes += 128 * len(pad)
    image, status = build(ctx, shape, seg, payload, links, desc, nbytes, max_mss=mss)
    assert np.array_equal(status, wstat)
    assert_image(image, want, desc, 0, f"jumbo {shape}")


# ---- 6. loopback through rx --------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_loopback_through_rx_and_the_option_records(gpu, shape):
    seg, payload, links, desc, nbytes = m.mixed_segments(seed=21)
    if shape != WAVE:
        keep = seg["payload_len"] <= (3 if shape == OCT else 127 if shape == ROW else 4000)
        seg, desc = seg[keep], desc[keep]
        seg, payload = repack(seg, payload)
    n, Q = len(seg), 8
    want_img, wstat = m.build_frames(seg, payload, links, desc, np.zeros(nbytes, np.uint8), max_mss=8960)
    assert not wstat.any()
    want = oracle.rx_chunk(want_img, desc, 0, oracle.rss_cfg(oracle.KEY_MICROSOFT, Q, 0))
    st = torch.cuda.Stream(device=DEV)
    with gpu.Context(0, rss=True, rss_key=oracle.KEY_MICROSOFT, rss_queues=Q, rss_endian=False) as c:
        b = Built(c, seg, payload, links, desc, nbytes, max_mss=8960, lead=lead_for(shape, seg, payload), stream=st)
        d_res = torch.zeros(n * 40, dtype=torch.uint8, device=DEV)
        d_opt = torch.zeros(n * 16, dtype=torch.uint8, device=DEV)
        b.launch()
        assert c.last_kernel == shape
        c.rx_chunk_dev(b.d_buf, b.d_desc, n, 0, d_res, stream=st)
        c.rx_tcpopt_chunk_dev(b.d_buf, b.d_desc, n, 0, d_res, d_opt, stream=st)
        _, status = b.read()
    assert not status.any()
    got = d_res.cpu().numpy().view(RESULT_DTYPE)
    assert got.tobytes() == want.tobytes()
    assert (got["verdict"] == 0).all() and not got["ip_csum"].any() and not got["tcp_csum"].any()
    for f in ("saddr", "daddr", "sport", "dport", "seq", "window", "payload_len"):
        assert np.array_equal(got[f], seg[f]), f
    assert np.array_equal(got["ack_seq"], np.where(seg["flags"] & m.ACK, seg["ack"], 0))
    assert np.array_equal(got["tcp_flags"], seg["flags"])
    opt = d_opt.cpu().numpy().view(TCPOPT_DTYPE)
    syn1 = 0
    for s, o in zip(seg, opt):
        if s["flags"] & m.RST:
            assert not o["flags"] & tcpopt_model.TS_FOUND
        else:
            assert o["flags"] & tcpopt_model.TS_FOUND and (o["ts_val"], o["ts_ref"]) == (s["ts_val"], s["ts_ecr"])
        if s["form"] == 1 and s["flags"] & m.SYN:
            assert (o["mss"], o["wscale"], o["ts_recent"]) == (s["mss"], s["wscale"], s["ts_val"])
            assert o["flags"] & (tcpopt_model.MSS | tcpopt_model.WSCALE | tcpopt_model.SAW_TS) == \
                tcpopt_model.MSS | tcpopt_model.WSCALE | tcpopt_model.SAW_TS
            syn1 += 1
    assert syn1 >= 4


# ---- 7. rejects ------------------------------------------------------------------------
def reject_case():
    """One segment of each reject between built neighbours, payloads 0..1447."""
    seg, payload, links, desc, _ = m.mixed_segments(seed=22)
    seg = seg[[0, 1, 2, 3, 4, 5, 6, 7, 0, 1, 8, 4, 5, 6]].copy()
    payload = payload[:int((seg["payload_off"] + seg["payload_len"]).max())].copy()
    desc = m.slots([m.frame_len(int(s["flags"]), int(s["payload_len"])) for s in seg], 9216)
    nbytes = 9216 * 14
    seg["flags"][1] |= 0x20                                    # BAD_SEG: an unknown flag bit
    seg["form"][3] = 2                                         # BAD_SEG: form
    seg["link"][5] = len(links)                                # BAD_SEG: link
    desc["len"][7] += 1                                        # BAD_DESC: len
    desc["offset"][9] += 1                                     # BAD_DESC: odd
    seg["payload_off"][11] = len(payload) - int(seg["payload_len"][11]) + 1     # BAD_PAYLOAD
    desc["offset"][13] = 0xFFFFFFF0                            # BAD_DESC: past buf_len
    want_status = [0, 1, 0, 1, 0, 1, 0, 2, 0, 2, 0, 3, 0, 2]
    return seg, payload, links, desc, nbytes, want_status


@pytest.mark.parametrize("shape", SHAPES)
def test_rejects_between_built_neighbours(ctx, shape):
    seg, payload, links, desc, nbytes, want_status = reject_case()
    want, wstat = m.build_frames(seg, payload, links, desc, np.full(nbytes, SENT, np.uint8))
    assert wstat.tolist() == want_status
    image, status = build(ctx, shape, seg, payload, links, desc, nbytes)
    assert status.tolist() == want_status
    assert_image(image, want, desc, 0, f"rejects {shape}")
    for i in np.flatnonzero(wstat):
        assert (image[i * 9216:(i + 1) * 9216] == SENT).all()


# ---- 8. a captured graph -----------------------------------------------------------------
def test_captured_build_and_rx_replay(gpu):
    seg, payload, links, desc, nbytes = m.mixed_segments(seed=23)
    n = len(seg)
    want_img, _ = m.build_frames(seg, payload, links, desc, np.full(nbytes, SENT, np.uint8), max_mss=8960)
    want = oracle.rx_chunk(want_img, desc, 0)
    st = torch.cuda.Stream(device=DEV)
    with gpu.Context(0) as c:
        b = Built(c, seg, payload, links, desc, nbytes, max_mss=8960, stream=st)
        d_res = torch.zeros(n * 40, dtype=torch.uint8, device=DEV)

        def launch():
            b.launch()
            c.rx_chunk_dev(b.d_buf, b.d_desc, n, 0, d_res, stream=st)

        launch()                                           # kernels loaded before the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            launch()
        seen = []
        for _ in range(2):
            b.whole.fill_(SENT)
            b.d_status.fill_(SENT)
            d_res.zero_()
            torch.cuda.synchronize()
            g.replay()
            image, status = b.read()
            assert not status.any()
            assert_image(image, want_img, desc, 0, "replay")
            res = d_res.cpu().numpy()
            assert res.tobytes() == want.tobytes()
            seen.append((image.tobytes(), res.tobytes()))
        assert seen[0] == seen[1]
        del g


# ---- 9. the host call -----------------------------------------------------------------
@pytest.mark.parametrize("limit", [0, 5_000_000], ids=["unbounded", "bounded"])
def test_host_call(gpu, fixture_case, limit):
    """A small batch at the staging's first size, the fixture past it (the
    staging grows), the small batch again in the grown staging; the rejects'
    slots stay as they were and n_built counts the built frames."""
    fseg, fpayload, flinks, flens, fwant = fixture_case
    rseg, rpayload, rlinks, rdesc, rbytes, rstatus = reject_case()
    rwant, _ = m.build_frames(rseg, rpayload, rlinks, rdesc, np.full(rbytes, SENT, np.uint8))
    with gpu.Context(0) as c:
        c.wait_limit = limit
        for what in ("small", "fixture", "small"):
            if what == "small":
                buf = np.full(rbytes, SENT, np.uint8)
                status, built = c.tx_build(rseg, rpayload, rlinks, buf, rdesc)
                assert status.tolist() == rstatus and built == rstatus.count(0)
                assert_image(buf, rwant, rdesc, 0, f"host {what} limit {limit}")
            else:
                buf = np.full(len(fwant), SENT, np.uint8)
                desc = m.slots(flens, SLOT, 6)
                status, built = c.tx_build(fseg, fpayload, flinks, buf, desc, off_shift=6)
                assert not status.any() and built == len(fseg)
                assert_image(buf, fwant, desc, 6, f"host {what} limit {limit}")


def test_host_call_gives_up_at_the_limit(gpu):
    """The stalled-GPU pattern of tests/test_gpu_bounded.py (its helpers, its
    stall and limit values): ETIMEDOUT within the limit, buf and status keep
    their sentinel right after the call and after the stall has ended, the
    context answers EIO, a fresh context builds the model's image."""
    from mtcp_amd._lib import lib
    from tests.test_gpu_bounded import LIMIT_US, SLACK_S, STALL_US, stall_lib, stream_busy, stream_wait
    L, S = lib(), stall_lib()
    seg, payload, links, desc, nbytes, want_status = reject_case()
    want, _ = m.build_frames(seg, payload, links, desc, np.full(nbytes, SENT, np.uint8))
    n = len(seg)

    def call(c):
        buf = np.full(nbytes, SENT, np.uint8)
        status = np.full(n, SENT, np.uint8)
        rc = L.mtcp_gpu_tx_build(c._h, seg.ctypes.data, n, payload.ctypes.data, payload.nbytes, links.ctypes.data,
                                 len(links), buf.ctypes.data, nbytes, desc.ctypes.data, 0, 0, 0,
                                 status.ctypes.data, None)
        return rc, buf, status

    c = gpu.Context(0)
    handle = c.stream
    rc, buf, status = call(c)                               # unbounded: stage sized, kernels loaded
    assert rc == 0 and status.tolist() == want_status
    assert_image(buf, want, desc, 0, "before the stall")
    c.wait_limit = LIMIT_US
    assert S.mtcp_gpu_debug_stall(c._h, STALL_US) == 0
    t0 = time.monotonic()
    rc, buf, status = call(c)
    dt = time.monotonic() - t0
    assert rc == ETIMEDOUT, rc
    assert dt < LIMIT_US / 1e6 + SLACK_S, dt
    assert stream_busy(handle)
    assert (buf == SENT).all() and (status == SENT).all()
    assert L.mtcp_gpu_sync(c._h) == EIO
    rc2, buf2, status2 = call(c)
    assert rc2 == EIO and (buf2 == SENT).all() and (status2 == SENT).all()
    c.close()
    stream_wait(handle)                                     # the stall and what was queued behind it end
    assert (buf == SENT).all() and (status == SENT).all()
    with gpu.Context(0) as fresh:
        fresh.wait_limit = 5_000_000
        rc, buf, status = call(fresh)
        assert rc == 0 and status.tolist() == want_status
        assert_image(buf, want, desc, 0, "fresh context")


# ---- 10. error returns -----------------------------------------------------------------
def test_error_returns(ctx):
    from mtcp_amd._lib import lib
    L = lib()
    seg, payload, links, desc, nbytes, _ = reject_case()
    n = len(seg)
    d_seg, d_links, d_desc, d_payload = up(seg), up(links), up(desc), up(payload)
    pad = torch.zeros(64, dtype=torch.uint8, device=DEV)
    d_buf = torch.full((nbytes,), SENT, dtype=torch.uint8, device=DEV)
    d_status = torch.full((n,), SENT, dtype=torch.uint8, device=DEV)
    good = dict(seg=d_seg.data_ptr(), n=n, payload=d_payload.data_ptr(), payload_bytes=len(payload),
                links=d_links.data_ptr(), n_links=len(links), buf=d_buf.data_ptr(), buf_len=nbytes,
                desc=d_desc.data_ptr(), off_shift=0, max_mss=0, flags=0, status=d_status.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        return L.mtcp_gpu_tx_build_dev(ctx._h, a["seg"], a["n"], a["payload"], a["payload_bytes"], a["links"],
                                       a["n_links"], a["buf"], a["buf_len"], a["desc"], a["off_shift"],
                                       a["max_mss"], a["flags"], a["status"], None)

    assert L.mtcp_gpu_tx_build_dev(None, *[good[k] for k in good], None) == EINVAL
    for k in ("seg", "payload", "links", "buf", "desc", "status"):
        assert call(**{k: None}) == EINVAL, k
    assert call(seg=pad.data_ptr() + 4) == EINVAL
    assert call(desc=pad.data_ptr() + 4) == EINVAL
    assert call(links=pad.data_ptr() + 2) == EINVAL
    assert call(n_links=0) == EINVAL and call(n_links=257) == EINVAL
    assert call(flags=2) == EINVAL and call(off_shift=17) == EINVAL
    # the payload range inside, and one byte into, the frames' range
    assert call(payload=d_buf.data_ptr() + 16, payload_bytes=64) == EINVAL
    assert call(payload=d_buf.data_ptr() + nbytes - 1, payload_bytes=64) == EINVAL
    assert call(buf=d_payload.data_ptr() + len(payload) - 1, buf_len=16) == EINVAL
    torch.cuda.synchronize()
    assert (d_buf.cpu().numpy() == SENT).all() and (d_status.cpu().numpy() == SENT).all()
    # n == 0: OK without a launch, whatever the pointers
    assert call(n=0) == 0
    assert call(n=0, seg=None, payload=None, links=None, buf=None, desc=None, status=None, payload_bytes=0,
                buf_len=0) == 0
    # the host call: the same checks on host pointers
    buf = np.full(nbytes, SENT, np.uint8)
    status = np.full(n, SENT, np.uint8)

    def host(**kw):
        a = dict(dict(seg=seg.ctypes.data, n=n, payload=payload.ctypes.data, payload_bytes=payload.nbytes,
                      links=links.ctypes.data, n_links=len(links), buf=buf.ctypes.data, buf_len=nbytes,
                      desc=desc.ctypes.data, off_shift=0, max_mss=0, flags=0, status=status.ctypes.data), **kw)
        return L.mtcp_gpu_tx_build(ctx._h, a["seg"], a["n"], a["payload"], a["payload_bytes"], a["links"],
                                   a["n_links"], a["buf"], a["buf_len"], a["desc"], a["off_shift"],
                                   a["max_mss"], a["flags"], a["status"], None)

    for k in ("seg", "payload", "links", "buf", "desc", "status"):
        assert host(**{k: None}) == EINVAL, k
    assert host(n_links=0) == EINVAL and host(n_links=257) == EINVAL and host(flags=2) == EINVAL
    assert host(payload=buf.ctypes.data + 8, payload_bytes=8) == EINVAL
    assert host(n=0) == 0
    assert (buf == SENT).all() and (status == SENT).all()
    # the calls above left the context usable
    torch.cuda.synchronize()
    assert call() == 0
    torch.cuda.synchronize()
    assert d_status.cpu().numpy().tolist() == reject_case()[5]
