"""Pure-ACK generation on the GPU (include/mtcp_gpu_ackgen.h,
mtcp_amd/csrc/ackgen_kernels.hpp): every byte of d_seg, d_desc, d_tx,
d_ares[:m] and d_total of every case is compared with tests/ackgen_model.py;
none is sampled.

Guard regions sit behind every output, the workspace is exactly sized and
pre-filled with 0xA5, d_ares past m keeps its sentinel, records of streams
absent from the batch keep every byte.  List lengths around the lane / wave
threshold and around the 6-bit wrap, a list of a few thousand mixed flags,
segment counts around the wave and the workgroup, every room cut, slot sizes
and shifts, every status, BAD records of each kind, hostile inputs, the built
frames, the host-memory form and the error returns."""
import numpy as np
import pytest

from mtcp_amd._types import (ACKGEN_RES_DTYPE, ACKGEN_STATE_DTYPE, DESC_DTYPE, RCV_PLACE_DTYPE, TX_LINK_DTYPE,
                             TX_SEG_DTYPE)
from tests import ackgen_gen as gg
from tests import ackgen_model as am
from tests import group_model as gm
from tests import txbuild_model as xm

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EINVAL, EIO = -22, -5
GUARD = 4096
SENT = 0xA5
NOW, AGG = gg.NOW, gg.AGG


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
def LANE(gpu):
    return gpu.Context.ackgen_lane_len()


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

    def guard_intact(self):
        return bool((self.all[self.nbytes:] == SENT).all().item())

    def numpy(self, dtype=np.uint8):
        return self.t.cpu().numpy().view(dtype)


LINKS = np.zeros(3, dtype=TX_LINK_DTYPE)
LINKS["dst"] = [[2, 0, 0, 0, 0, i] for i in range(3)]
LINKS["src"] = [[2, 1, 0, 0, 0, i] for i in range(3)]


class Call:
    """The device arrays of one call on batch b, the outputs guarded."""

    def __init__(self, gpu, b, nseg=None, image_bytes=0):
        self.b, n, self.max_id = b, b["n"], b["max_id"]
        idx, seg_sid, seg_start = b["group"]
        self.m = min(len(seg_sid) if nseg is None else nseg, n)
        pad = lambda a, k: np.concatenate([a, np.full(max(k - len(a), 0), 0xA5A5A5A5, np.uint32)]).astype(np.uint32)
        self.place = to_dev(b["place"]) if n else to_dev(np.zeros(1, RCV_PLACE_DTYPE))
        self.idx, self.seg_sid = to_dev(pad(idx, 1)), to_dev(pad(seg_sid, max(n, 1)))
        self.seg_start = to_dev(pad(seg_start, n + 1))
        self.nseg = to_dev(np.array([len(seg_sid) if nseg is None else nseg], np.uint32))
        self.seg_stop = to_dev(pad(b["seg_stop"], max(n, 1)))
        self.ack_stop = None if b["ack_stop"] is None else to_dev(pad(b["ack_stop"], max(n, 1)))
        self.state, self.snd = to_dev(b["state"]), to_dev(b["snd"])
        self.tx = Guarded(32 * (self.max_id + 1), b["tx"])
        cap = b["seg_cap"]
        self.seg, self.desc = Guarded(48 * cap), Guarded(8 * cap)
        self.ares, self.total = Guarded(16 * max(n, 1)), Guarded(16)
        self.status = Guarded(cap)
        self.wb = gpu.Context.ackgen_work_bytes(n, self.max_id)
        assert self.wb > 0
        self.work = Guarded(self.wb)
        self.image = Guarded(image_bytes) if image_bytes else None
        self.links = to_dev(LINKS)

    def args(self):
        b = self.b
        return (self.place, b["n"], self.max_id, self.idx, self.seg_sid, self.seg_start, self.nseg, self.seg_stop,
                self.ack_stop, self.state, self.snd, b["cur_ts"], self.tx.t)

    def run(self, ctx):
        b = self.b
        ctx.ackgen_dev(*self.args(), b["n_links"], b["buf_off"], b["buf_len"], b["off_shift"], b["slot_bytes"],
                       self.seg.t, self.desc.t, b["seg_cap"], self.ares.t, self.total.t, self.work.t)

    def send(self, ctx):
        b = self.b
        ctx.ack_send_dev(*self.args(), self.links, self.image.t, b["buf_off"], b["off_shift"], b["slot_bytes"],
                         self.seg.t, self.desc.t, b["seg_cap"], self.ares.t, self.total.t, self.status.t, self.work.t,
                         buf_len=min(b["buf_len"], self.image.nbytes))

    def check(self, want, what=""):
        for name in ("tx", "seg", "desc", "ares", "total", "work", "status"):
            assert getattr(self, name).guard_intact(), f"{what}: bytes behind {name} were written"
        w_seg, w_desc, w_ares, w_total, w_tx = want
        got = (self.seg.numpy(TX_SEG_DTYPE), self.desc.numpy(DESC_DTYPE), self.ares.numpy(ACKGEN_RES_DTYPE),
               self.total.numpy(np.uint64), self.tx.numpy(ACKGEN_STATE_DTYPE))
        m = len(w_ares)
        assert m == self.m
        for g, e, name in ((got[0], w_seg, "seg"), (got[1], w_desc, "desc"), (got[2][:m], w_ares, "ares"),
                           (got[3], w_total, "total"), (got[4], w_tx, "tx")):
            if g.tobytes() != e.tobytes():
                bad = [i for i in range(len(e)) if g[i].tobytes() != e[i].tobytes()]
                raise AssertionError(f"{what}: {len(bad)} of {len(e)} {name} records differ, first at {bad[0]}: "
                                     f"{g[bad[0]]} want {e[bad[0]]}")
        assert (got[2][m:].view(np.uint8) == SENT).all(), f"{what}: ares past m was written"
        return got


def run(gpu, ctx, b, what="", nseg=None):
    want = gg.expect(b, nseg)
    c = Call(gpu, b, nseg)
    c.run(ctx)
    torch.cuda.synchronize()
    c.check(want, what)
    return want


def status_of(want, b, i):
    """The status of stream i of the batch's spec."""
    _, seg_sid, _ = b["group"]
    j = int(np.nonzero(seg_sid == b["ids"][i])[0][0])
    return int(want[2][j]["status"]), want[2][j]


def test_list_lengths(gpu, ctx, LANE):
    lens = [1, LANE - 1, LANE, LANE + 1, 63, 64, 65, 129]
    streams = [dict(len=k, flags="now") for k in lens] + [dict(len=k, flags="mixed") for k in lens]
    b = gg.make(streams, seed=3)
    want = run(gpu, ctx, b, "list lengths")
    for i, k in enumerate(lens):
        st, r = status_of(want, b, i)
        assert st == am.SENT and r["n_ack"] == k % 64, (k, r)       # the 64th NOW wraps the count to 0
    assert int(want[3][0]) > 0


def test_long_mixed_list(gpu, ctx):
    streams = [dict(len=3001, flags="mixed", tx=dict(ack_cnt=62, is_wack=1)), dict(len=2, flags="agg"),
               dict(len=700, flags="agg"), dict(len=641, flags="now", tx=dict(ack_cnt=5)),
               dict(len=200, flags=np.tile(np.array([NOW | AGG, 0, NOW, AGG], np.uint8), 50))]
    run(gpu, ctx, gg.make(streams, seed=4, n_miss=3, n_none=2), "a long mixed list")


@pytest.mark.parametrize("m", [1, 63, 64, 65, 129, 257])
def test_segment_counts(gpu, ctx, m):
    extra = 2 if m > 2 else 0                                       # the MISS and the NONE segment are among the m
    streams = [dict(len=1 + (i % 3), flags=("now", "agg", "mixed")[i % 3]) for i in range(m - extra)]
    b = gg.make(streams, seed=10 + m, n_miss=2 if extra else 0, n_none=1 if extra else 0)
    assert len(b["group"][1]) == m
    run(gpu, ctx, b, f"{m} segments")


def three(**room):
    """Three streams, each with 3 plain ACKs and a probe planned."""
    return gg.make([dict(len=3, flags="now", tx=dict(is_wack=1)) for _ in range(3)], seed=21, **room)


@pytest.mark.parametrize("cut,by", [(c, b) for c in ("first_frame", "before_probe", "boundary", "zero", "all")
                                    for b in ("seg_cap", "buf_len") if (c, b) != ("zero", "seg_cap")])
def test_room(gpu, ctx, cut, by):
    # the second stream's run is records 4-7: 4, 5, 6 plain, 7 the probe
    k = {"first_frame": 5, "before_probe": 7, "boundary": 4, "zero": 0, "all": 12}[cut]
    if by == "seg_cap":
        b = three(seg_cap=k)
    else:                                                           # the slot is 66 B: frame k ends one byte past buf_len
        b = three(seg_cap=16, buf_off=64, buf_len=64 + 66 * k + 65)
    want = run(gpu, ctx, b, f"room {cut} by {by}")
    assert int(want[3][0]) == k and int(want[3][1]) == 66 * k
    second = want[2][1]
    exp = {"first_frame": (am.NO_ROOM, 1, 0), "before_probe": (am.NO_ROOM, 3, 0), "boundary": (am.NO_ROOM, 0, 0),
           "zero": (am.NO_ROOM, 0, 0), "all": (am.SENT, 3, 1)}[cut]
    assert (second["status"], second["n_ack"], second["wack"]) == exp, second
    tx = want[4][int(b["group"][1][1])]
    assert (tx["ack_cnt"], tx["is_wack"]) == (3 - exp[1], 1 - exp[2])


# slot_bytes is a multiple of A = max(2, 1 << off_shift) by contract: 66 with a shift of 6 is EINVAL (below)
@pytest.mark.parametrize("slot_bytes,off_shift", [(s, o) for s in (0, 66, 128) for o in (0, 1, 6) if (s, o) != (66, 6)])
def test_slots(gpu, ctx, slot_bytes, off_shift):
    A = max(2, 1 << off_shift)
    streams = [dict(len=5, flags="mixed", tx=dict(is_wack=i & 1)) for i in range(9)]
    slot = am.slot_of(off_shift, slot_bytes)
    b = gg.make(streams, seed=30, buf_off=3 * A, buf_len=3 * A + 7 * slot + 66, off_shift=off_shift, slot_bytes=slot_bytes)
    want = run(gpu, ctx, b, f"slot {slot_bytes} shift {off_shift}")
    assert int(want[3][0]) == 8 and int(want[3][1]) == 8 * slot


def test_streams(gpu, ctx):
    streams = [
        dict(len=6, flags="now", defer=("seg", 2)),                               # DEFERRED by d_seg_stop, prefix folded
        dict(len=6, flags="now", defer=("ack", 1)),                               # DEFERRED by d_ack_stop
        dict(len=4, flags="none"),                                                # IDLE
        dict(len=4, flags="none", tx=dict(has_rcvbuf=0), put=True),               # IDLE, has_rcvbuf set
        dict(len=3, flags="agg", tx=dict(has_rcvbuf=0)),                          # NOT_TO_ACK: no receive buffer
        dict(len=3, flags="agg", tx=dict(has_rcvbuf=0), put=True),                # SENT: a PUT_* allocates it
        dict(len=3, flags="now", state=dict(rcv_nxt=5000, head_seq=1000, merged_len=3999)),   # NOT_TO_ACK
        dict(len=3, flags="now", state=dict(rcv_nxt=5000, head_seq=1000, merged_len=4000)),   # SENT
        dict(len=5, flags="now", tx=dict(ip_id=65533, is_wack=1)),                # ip_id wraps
        dict(len=2, flags="now", tx=dict(wscale_mine=7), state=dict(rcv_wnd=127)),            # window32 0
        dict(len=2, flags="now", tx=dict(wscale_mine=0), state=dict(rcv_wnd=65536)),          # above 65535
        dict(len=2, flags="now", tx=dict(wscale_mine=2, need_wnd_adv=1), state=dict(rcv_wnd=3)),
        dict(len=2, flags="none", tx=dict(ack_cnt=63)),                           # on the list from before
        dict(len=2, flags="none", tx=dict(is_wack=1)),                            # the probe alone
        dict(len=2, flags="now", state=dict(tcp_state=5)),                        # not ESTABLISHED: DEFERRED
        dict(len=2, flags="now", tx=dict(rsvd=[0, 0, 0, 0, 0, 0, 0, 1])),         # BAD, each kind
        dict(len=2, flags="now", tx=dict(rsvd=[1, 0, 0, 0, 0, 0, 0, 0])),
        dict(len=2, flags="now", tx=dict(ack_cnt=64)),
        dict(len=2, flags="now", tx=dict(is_wack=2)),
        dict(len=2, flags="now", tx=dict(has_rcvbuf=2)),
        dict(len=2, flags="now", tx=dict(need_wnd_adv=2)),
        dict(len=2, flags="now", tx=dict(wscale_mine=32)),
        dict(len=2, flags="now", tx=dict(link=3)),
    ]
    exp = [am.DEFERRED, am.DEFERRED, am.IDLE, am.IDLE, am.NOT_TO_ACK, am.SENT, am.NOT_TO_ACK, am.SENT, am.SENT, am.SENT,
           am.SENT, am.SENT, am.SENT, am.SENT, am.DEFERRED] + [am.BAD] * 8
    for with_ack_stop in (True, False):
        b = gg.make(streams, seed=40, with_ack_stop=with_ack_stop, n_miss=1)
        want = run(gpu, ctx, b, f"streams, ack_stop {with_ack_stop}")
        e = list(exp)
        if not with_ack_stop:
            e[1] = am.SENT
        for i, st in enumerate(e):
            got, r = status_of(want, b, i)
            assert got == st, (i, am_status(got), am_status(st), r)
        tx = want[4]
        assert tx[b["ids"][0]]["ack_cnt"] == 2 and tx[b["ids"][3]]["has_rcvbuf"] == 1
        assert tx[b["ids"][8]]["ip_id"] == (65533 + 6) & 0xFFFF
        assert status_of(want, b, 9)[1]["flags"] & am.NEED_WND_ADV and tx[b["ids"][9]]["need_wnd_adv"] == 1
        assert status_of(want, b, 10)[1]["window"] == 65535


def am_status(v):
    return ("NONE", "BAD", "DEFERRED", "IDLE", "NOT_TO_ACK", "SENT", "NO_ROOM")[v]


def test_empty_batch_and_empty_segment(gpu, ctx):
    b = gg.make([], seed=50, seg_cap=300)                           # n == 0: void records and zero totals
    assert b["n"] == 0
    want = run(gpu, ctx, b, "n == 0")
    assert (want[0]["form"] == am.VOID_FORM).all() and not want[3].any()
    # a table with an empty segment in front of the stream's own (list length 0)
    b = gg.make([dict(len=3, flags="now"), dict(len=2, flags="agg")], seed=51)
    idx, seg_sid, seg_start = b["group"]
    free = [i for i in range(b["max_id"] + 1) if i not in set(int(x) for x in b["ids"])][0]
    b["group"] = (idx, np.concatenate([[free], seg_sid]).astype(np.uint32),
                  np.concatenate([[0], seg_start]).astype(np.uint32))
    b["seg_stop"] = np.concatenate([[0], b["seg_stop"]]).astype(np.uint32)
    b["ack_stop"] = np.concatenate([[0], b["ack_stop"]]).astype(np.uint32)
    b["tx"][free]["is_wack"] = 1
    want = run(gpu, ctx, b, "an empty segment")
    assert want[2][0]["status"] == am.SENT and want[2][0]["wack"] == 1


def test_hostile_inputs(gpu, ctx):
    rng = np.random.default_rng(60)
    streams = [dict(len=int(k), flags="mixed") for k in rng.integers(1, 40, 150)] + [dict(len=300, flags="mixed")]
    for case in range(3):
        b = gg.make(streams, seed=61 + case, n_miss=5, n_none=5, max_id=400, seg_cap=5000)
        n, ids = b["n"], b["max_id"] + 1
        b["place"] = np.frombuffer(rng.bytes(16 * n), dtype=RCV_PLACE_DTYPE).copy()
        b["state"] = np.frombuffer(rng.bytes(64 * ids), dtype=b["state"].dtype).copy()
        b["state"]["tcp_state"][rng.random(ids) < .8] = 4
        b["snd"] = np.frombuffer(rng.bytes(128 * ids), dtype=b["snd"].dtype).copy()
        raw = np.frombuffer(rng.bytes(32 * ids), dtype=am.STATE_DTYPE).copy()
        keep = rng.random(ids) < .6                                 # random bytes in some records, near-valid ones in the rest
        for f in ("ack_cnt", "is_wack", "wscale_mine", "has_rcvbuf", "need_wnd_adv", "ip_id", "link"):
            b["tx"][f] = np.where(keep, b["tx"][f], raw[f])
        b["tx"]["ack_cnt"][keep] = rng.integers(0, 64, int(keep.sum()))
        bad_rsvd = ~keep & (rng.random(ids) < .3)
        b["tx"]["rsvd"][bad_rsvd] = raw["rsvd"][bad_rsvd] | 1
        idx, seg_sid, seg_start = b["group"]
        idx = idx.copy()
        idx[rng.random(n) < .05] = rng.integers(n, 1 << 32, dtype=np.uint64)      # entries at or above n: skipped
        seg_sid = seg_sid.copy()
        seg_sid[rng.integers(0, len(seg_sid), 4)] = b["max_id"] + 1 + rng.integers(0, 1000, 4)   # ids above max_id
        b["group"] = (idx, seg_sid, seg_start)
        nseg = None
        if case == 2:                                               # d_nseg[0] above n: clamped
            nseg = n + 1000
            pad = lambda a, k: np.concatenate([a, rng.integers(0, 1 << 32, max(k - len(a), 0), dtype=np.uint64)]).astype(np.uint32)
            b["group"] = (idx, pad(seg_sid, n), pad(seg_start, n + 1))
            b["group"][1][len(seg_sid):] = gm.FLOW_NONE             # every stream in one segment, by contract
            b["seg_stop"], b["ack_stop"] = pad(b["seg_stop"], n), pad(b["ack_stop"], n)
        run(gpu, ctx, b, f"hostile {case}", nseg=nseg)


def test_absent_streams_and_purity(gpu, ctx):
    b = gg.make([dict(len=20, flags="mixed") for _ in range(70)], seed=70, max_id=999)
    want = gg.expect(b)
    absent = np.setdiff1d(np.arange(1000), b["ids"])
    assert want[4][absent].tobytes() == b["tx"][absent].tobytes()
    c = Call(gpu, b)
    c.run(ctx)
    torch.cuda.synchronize()
    first = c.check(want, "first run")
    c2 = Call(gpu, b)
    c2.work.t.fill_(0x3C)                                           # nothing depends on what the workspace held
    c2.run(ctx)
    torch.cuda.synchronize()
    second = c2.check(want, "second run")
    assert all(a.tobytes() == s.tobytes() for a, s in zip(first, second))


def test_built_frames(gpu, ctx):
    """ack_send_dev: the frames in the buffer are the model's records through
    the frame model; every void record is BAD_SEG with its slot untouched."""
    streams = [dict(len=int(k), flags="mixed", tx=dict(is_wack=int(k) & 1)) for k in range(1, 40)]
    b = gg.make(streams, seed=80, seg_cap=200, buf_off=128, buf_len=128 + 128 * 150, slot_bytes=128)
    want = gg.expect(b)
    c = Call(gpu, b, image_bytes=b["buf_len"])
    c.send(ctx)
    torch.cuda.synchronize()
    c.check(want, "ack_send_dev")
    assert c.image.guard_intact()
    T = int(want[3][0])
    assert 0 < T <= 150
    image, status = c.image.numpy(), c.status.numpy()
    w_image, w_status = xm.build_frames(want[0], np.zeros(0, np.uint8), LINKS, want[1],
                                        np.full(b["buf_len"], SENT, np.uint8))
    assert status.tobytes() == w_status.tobytes()
    assert (status[:T] == xm.BUILT).all() and (status[T:] == xm.BAD_SEG).all()
    assert image.tobytes() == w_image.tobytes()


def test_host_form(gpu, ctx):
    streams = [dict(len=int(k), flags="mixed") for k in range(1, 30)] + [dict(len=100, flags="now", defer=("ack", 3))]
    b = gg.make(streams, seed=90, n_miss=2, seg_cap=777)
    want = gg.expect(b)
    idx, seg_sid, seg_start = b["group"]
    for limit in (0, 5_000_000):
        with gpu.Context(0) as c:
            if limit:
                c.wait_limit = limit
            tx = b["tx"].copy()
            seg, desc, ares, total = c.ackgen(b["place"], b["max_id"], idx, seg_sid, seg_start, b["seg_stop"],
                                              b["ack_stop"], b["state"], b["snd"], b["cur_ts"], tx, b["n_links"],
                                              b["buf_len"], b["seg_cap"])
            for g, e in zip((seg, desc, ares, total, tx), want):
                assert g.tobytes() == e.tobytes()
            e0 = gg.make([], seed=91, seg_cap=9)                    # n == 0: void records, zero totals, tx untouched
            tx = e0["tx"].copy()
            seg, desc, ares, total = c.ackgen(e0["place"], e0["max_id"], *e0["group"], e0["seg_stop"], e0["ack_stop"],
                                              e0["state"], e0["snd"], 5, tx, 3, 1 << 20, 9)
            assert seg.tobytes() == am.void_records(9).tobytes() and not desc.view(np.uint8).any()
            assert len(ares) == 0 and not total.any() and tx.tobytes() == e0["tx"].tobytes()


def test_room_cut_by_the_descriptor_offset(gpu, ctx):
    """Neither seg_cap nor buf_len cuts: record 3's offset would not fit 32 bits."""
    for off_shift, slot_bytes in ((0, 0), (6, 128), (1, 66)):
        slot = am.slot_of(off_shift, slot_bytes)
        last = (0xFFFFFFFF << off_shift) & ~(max(2, 1 << off_shift) - 1)    # the last offset a descriptor can name
        b = three(seg_cap=16, buf_off=last - 2 * slot, buf_len=1 << 62, off_shift=off_shift, slot_bytes=slot_bytes)
        want = run(gpu, ctx, b, f"offset limit, shift {off_shift}")
        assert int(want[3][0]) == 3 and want[1]["offset"][2] == last >> off_shift
        assert [int(r["status"]) for r in want[2]] == [am.NO_ROOM] * 3
        b = three(seg_cap=16, buf_off=last + max(2, 1 << off_shift), buf_len=1 << 62, off_shift=off_shift,
                  slot_bytes=slot_bytes)                            # buf_off itself past the limit: nothing fits
        want = run(gpu, ctx, b, f"past the offset limit, shift {off_shift}")
        assert int(want[3][0]) == 0


def test_error_returns(gpu, ctx):
    """MTCP_GPU_EINVAL for each misuse the header lists, for every pointer of
    mtcp_gpu_ackgen_dev, mtcp_gpu_ack_send_dev and mtcp_gpu_ackgen; d_ack_stop
    NULL is accepted; a refused call writes nothing."""
    from mtcp_amd._lib import lib
    L = lib()
    b = gg.make([dict(len=int(k), flags="mixed") for k in range(1, 20)], seed=92, seg_cap=300)
    want, want_no_stop = gg.expect(b), gg.expect(dict(b, ack_stop=None))
    n, max_id, cap, ts = b["n"], b["max_id"], b["seg_cap"], b["cur_ts"]
    d = Call(gpu, b, image_bytes=66 * cap)
    room = {k: Guarded(64) for k in ("a", "b")}                     # misaligned stand-ins, never dereferenced
    p = lambda t, off=0: t.data_ptr() + off
    big, MAX_ID = (1 << 26) + 1, gm.MAX_ID

    def dev(c=ctx._h, pc=p(d.place), n_=n, mx=max_id, i=p(d.idx), ss=p(d.seg_sid), st=p(d.seg_start), ns=p(d.nseg),
            sp=p(d.seg_stop), asp=p(d.ack_stop), s=p(d.state), sn=p(d.snd), tx=p(d.tx.t), nl=3, bo=0, bl=1 << 40,
            sh=0, sb=0, sg=p(d.seg.t), de=p(d.desc.t), cp=cap, ar=p(d.ares.t), to=p(d.total.t), w=p(d.work.t),
            wbytes=d.wb):
        return L.mtcp_gpu_ackgen_dev(c, pc, n_, mx, i, ss, st, ns, sp, asp, s, sn, ts, tx, nl, bo, bl, sh, sb, sg, de, cp,
                                     ar, to, w, wbytes, None)

    def send(c=ctx._h, pc=p(d.place), i=p(d.idx), ss=p(d.seg_sid), st=p(d.seg_start), ns=p(d.nseg), sp=p(d.seg_stop),
             asp=p(d.ack_stop), s=p(d.state), sn=p(d.snd), tx=p(d.tx.t), lk=p(d.links), nl=3, bf=p(d.image.t), bo=0,
             bl=66 * cap, sh=0, sb=0, fl=0, sg=p(d.seg.t), de=p(d.desc.t), cp=cap, ar=p(d.ares.t), to=p(d.total.t),
             su=p(d.status.t), w=p(d.work.t), wbytes=d.wb):
        return L.mtcp_gpu_ack_send_dev(c, pc, n, max_id, i, ss, st, ns, sp, asp, s, sn, ts, tx, lk, nl, bf, bo, bl, sh, sb,
                                       fl, sg, de, cp, ar, to, su, w, wbytes, None)

    bad = {
        "ctx NULL": dev(c=None), "place NULL": dev(pc=None), "idx NULL": dev(i=None), "seg_sid NULL": dev(ss=None),
        "seg_start NULL": dev(st=None), "nseg NULL": dev(ns=None), "seg_stop NULL": dev(sp=None),
        "state NULL": dev(s=None), "snd NULL": dev(sn=None), "tx NULL": dev(tx=None), "seg NULL": dev(sg=None),
        "desc NULL": dev(de=None), "ares NULL": dev(ar=None), "total NULL": dev(to=None), "work NULL": dev(w=None),
        "seg NULL, n 0": dev(n_=0, sg=None), "desc NULL, n 0": dev(n_=0, de=None), "total NULL, n 0": dev(n_=0, to=None),
        "place misaligned": dev(pc=p(room["a"].t, 8)), "idx misaligned": dev(i=p(room["a"].t, 2)),
        "seg_sid misaligned": dev(ss=p(room["a"].t, 1)), "seg_start misaligned": dev(st=p(room["a"].t, 3)),
        "nseg misaligned": dev(ns=p(room["a"].t, 2)), "seg_stop misaligned": dev(sp=p(room["a"].t, 2)),
        "ack_stop misaligned": dev(asp=p(room["a"].t, 2)), "state misaligned by 32": dev(s=p(d.state, 32)),
        "snd misaligned by 64": dev(sn=p(d.snd, 64)), "tx misaligned by 16": dev(tx=p(d.tx.t, 16)),
        "seg misaligned": dev(sg=p(d.seg.t, 4)), "desc misaligned": dev(de=p(d.desc.t, 4)),
        "ares misaligned": dev(ar=p(d.ares.t, 8)), "total misaligned": dev(to=p(d.total.t, 4)),
        "work misaligned": dev(w=p(d.work.t, 8)), "work too small": dev(wbytes=d.wb - 1), "no work bytes": dev(wbytes=0),
        "n too large": dev(n_=big), "max_id too large": dev(mx=MAX_ID + 1), "seg_cap 0": dev(cp=0),
        "seg_cap too large": dev(cp=(1 << 26) + 1), "off_shift 17": dev(sh=17), "n_links 0": dev(nl=0),
        "n_links 257": dev(nl=257), "slot below 66": dev(sb=64), "slot not a multiple of A": dev(sb=66, sh=6),
        "buf_off odd": dev(bo=1), "buf_off not a multiple of A": dev(bo=32, sh=6),
        "send: ctx NULL": send(c=None), "send: place NULL": send(pc=None), "send: idx NULL": send(i=None),
        "send: seg_sid NULL": send(ss=None), "send: seg_start NULL": send(st=None), "send: nseg NULL": send(ns=None),
        "send: seg_stop NULL": send(sp=None), "send: state NULL": send(s=None), "send: snd NULL": send(sn=None),
        "send: tx NULL": send(tx=None), "send: links NULL": send(lk=None), "send: buf NULL": send(bf=None),
        "send: seg NULL": send(sg=None), "send: desc NULL": send(de=None), "send: ares NULL": send(ar=None),
        "send: total NULL": send(to=None), "send: status NULL": send(su=None), "send: work NULL": send(w=None),
        "send: links misaligned": send(lk=p(d.links, 2)), "send: tx misaligned": send(tx=p(d.tx.t, 16)),
        "send: unknown builder flags": send(fl=2), "send: seg_cap 0": send(cp=0), "send: off_shift 17": send(sh=17),
        "send: n_links 0": send(nl=0), "send: n_links 257": send(nl=257), "send: slot below 66": send(sb=64),
        "send: buf_off odd": send(bo=1), "send: work too small": send(wbytes=d.wb - 1),
    }
    with gpu.Context(0, compact=True) as cc:
        bad["compact context"], bad["send: compact context"] = dev(c=cc._h), send(c=cc._h)
        place = np.ascontiguousarray(b["place"])
        u32 = lambda a: np.ascontiguousarray(a, dtype=np.uint32)
        idx, seg_sid, seg_start = (u32(a) for a in b["group"])
        h_stop, h_astop = u32(b["seg_stop"]), u32(b["ack_stop"])
        nseg = np.array([len(seg_sid)], np.uint32)
        h_tx = b["tx"].copy()
        h_seg, h_desc = np.full(48 * cap, SENT, np.uint8), np.full(8 * cap, SENT, np.uint8)
        h_ares, h_total = np.full(16 * n, SENT, np.uint8), np.full(16, SENT, np.uint8)
        hp = lambda a: a.ctypes.data

        def host(c=ctx._h, pc=hp(place), n_=n, mx=max_id, i=hp(idx), ss=hp(seg_sid), st=hp(seg_start), ns=hp(nseg),
                 sp=hp(h_stop), asp=hp(h_astop), s=hp(b["state"]), sn=hp(b["snd"]), tx=hp(h_tx), nl=3, bo=0,
                 bl=1 << 40, sh=0, sb=0, sg=hp(h_seg), de=hp(h_desc), cp=cap, ar=hp(h_ares), to=hp(h_total)):
            return L.mtcp_gpu_ackgen(c, pc, n_, mx, i, ss, st, ns, sp, asp, s, sn, ts, tx, nl, bo, bl, sh, sb, sg, de, cp,
                                     ar, to)

        bad.update({
            "host: ctx NULL": host(c=None), "host: place NULL": host(pc=None), "host: idx NULL": host(i=None),
            "host: seg_sid NULL": host(ss=None), "host: seg_start NULL": host(st=None), "host: nseg NULL": host(ns=None),
            "host: seg_stop NULL": host(sp=None), "host: state NULL": host(s=None), "host: snd NULL": host(sn=None),
            "host: tx NULL": host(tx=None), "host: seg NULL": host(sg=None), "host: desc NULL": host(de=None),
            "host: ares NULL": host(ar=None), "host: total NULL": host(to=None),
            "host: seg NULL, n 0": host(n_=0, sg=None), "host: total NULL, n 0": host(n_=0, to=None),
            "host: n too large": host(n_=big), "host: max_id too large": host(mx=MAX_ID + 1), "host: seg_cap 0": host(cp=0),
            "host: seg_cap too large": host(cp=(1 << 26) + 1), "host: off_shift 17": host(sh=17),
            "host: n_links 0": host(nl=0), "host: n_links 257": host(nl=257), "host: slot below 66": host(sb=64),
            "host: slot not a multiple of A": host(sb=66, sh=6), "host: buf_off odd": host(bo=1),
            "host: compact context": host(c=cc._h)})
    assert {k: v for k, v in bad.items() if v != EINVAL} == {}
    torch.cuda.synchronize()
    for g in (d.seg, d.desc, d.ares, d.total, d.work, d.status, d.image):    # none of these wrote anything
        assert (g.all == SENT).all().item()
    assert d.tx.numpy().tobytes() == b["tx"].tobytes() and d.tx.guard_intact()
    assert all((a == SENT).all() for a in (h_seg, h_desc, h_ares, h_total)) and h_tx.tobytes() == b["tx"].tobytes()
    assert dev() == 0 and host() == 0                               # and the same arguments, valid, work
    torch.cuda.synchronize()
    d.check(want, "after the refused calls")
    m = len(want[2])
    for g, e in ((h_seg, want[0]), (h_desc, want[1]), (h_ares[:16 * m], want[2]), (h_total, want[3]), (h_tx, want[4])):
        assert g.tobytes() == e.tobytes()
    d.tx.t.copy_(to_dev(b["tx"]))
    h_tx[:] = b["tx"]
    assert dev(asp=None) == 0 and host(asp=None) == 0               # d_ack_stop may be NULL
    torch.cuda.synchronize()
    d.check(want_no_stop, "d_ack_stop NULL")
    assert h_tx.tobytes() == want_no_stop[4].tobytes() and h_seg.tobytes() == want_no_stop[0].tobytes()
    d.tx.t.copy_(to_dev(b["tx"]))
    assert send() == 0 and send(asp=None) == 0                      # both valid
    torch.cuda.synchronize()
    # with n == 0 only seg, desc and total are needed
    assert dev(n_=0, pc=None, i=None, ss=None, st=None, ns=None, sp=None, asp=None, s=None, sn=None, tx=None, ar=None,
               w=None, wbytes=0) == 0
    torch.cuda.synchronize()
    assert d.seg.numpy(TX_SEG_DTYPE).tobytes() == am.void_records(cap).tobytes() and not d.total.numpy().any()



# ---- the reference fixture on the device ----------------------------------------------------------------
def test_fixture_on_the_device(gpu, ctx):
    """Every case of tests/golden/ackgen_cases.bin as a one-stream batch through
    ack_send_dev: the frames in the buffer are the reference's bytes, the tx
    record after is the reference's stream after."""
    cases = am.load_fixture()
    assert len(cases) > 400
    links = to_dev(am.fixture_links())
    for i, c in enumerate(cases):
        opts = [int(o) for o in c["opts"] if int(o) != am.ACK_OPT_WACK]
        k = max(len(opts), 1)                                       # a stream with no EnqueueACK still has a packet
        fl = np.zeros(k, np.uint8)
        fl[:len(opts)] = [NOW if o == am.ACK_OPT_NOW else AGG for o in opts]
        be = c["before"]
        b = gg.make([dict(len=k, flags=fl)], seed=1, max_id=0, seg_cap=80, buf_off=0, buf_len=66 * c["budget"])
        t, st = b["tx"][0], b["state"][0]
        for f in am.STATE_DTYPE.names:
            if f != "rsvd":
                t[f] = be[f]
        if len(opts) != len(c["opts"]):
            t["is_wack"] = 1                                        # EnqueueACK(ACK_OPT_WACK), tcp_out.c:931-933
        for f in ("rcv_nxt", "rcv_wnd", "head_seq", "merged_len", "ts_recent"):
            st[f] = be[f]
        b["snd"][0]["snd_nxt"], b["cur_ts"] = be["snd_nxt"], c["cur_ts"]
        want = gg.expect(b)
        cl = Call(gpu, b, image_bytes=66 * 80)
        cl.links = links
        cl.send(ctx)
        torch.cuda.synchronize()
        cl.check(want, f"fixture case {i}")
        nf = len(c["frames"])
        assert int(want[3][0]) == nf, (i, am.FAMILIES[c["family"]])
        image = cl.image.numpy()
        assert image[:66 * nf].tobytes() == c["frames"].tobytes(), (i, am.FAMILIES[c["family"]])
        assert (image[66 * nf:] == SENT).all() and cl.image.guard_intact()
        after = want[4][0]
        assert all(int(after[f]) == c["after"][f] for f in am.STATE_DTYPE.names if f != "rsvd"), (i, after, c["after"])


# ---- frames in, ACK frames out -----------------------------------------------------------------------------
def make_chain(pkts=3800, extra=296):
    """4 096 frames made from a generated batch of stateful streams, as
    tests/test_gpu_ackwalk.py makes its chain batch (the frames' seq, ack_seq,
    window and timestamps are the batch's, so that the walks move the streams),
    and the three models' answers for them."""
    import oracle
    from mtcp_amd._types import TCPOPT_DTYPE, TCPOPT_TS_FOUND
    from tests import ackwalk_gen as ag
    from tests import flowtab_model as fm
    from tests import rcvwalk_model as rm
    from tests import tcpopt_model as tm
    from tests.test_gpu_ackwalk import lens_for
    rng = np.random.default_rng(146)
    b = ag.batch(rng, lens_for(rng, pkts + extra, extra), extra=extra)
    n = len(b["res"])
    assert n == pkts + extra
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
        f[26:34], f[34:38] = t[:8], t[8:12]
        f[38:42] = int(r["seq"]).to_bytes(4, "big")
        f[42:46] = int(r["ack_seq"]).to_bytes(4, "big")
        f[48:50] = int(r["window"]).to_bytes(2, "big")
        frames.append(f)
    buf, desc = tm.pack_chunk(frames, slot=64)
    tm.fill_checksums(buf, desc)
    for i in np.nonzero(b["sid"] == gm.FLOW_NONE)[0]:
        buf[int(desc["offset"][i]) + 50] ^= 0x55                    # the TCP checksum no longer holds
    desc = desc.astype(oracle.DESC_DTYPE)
    res = oracle.rx_chunk(buf, desc, 0, None)
    ok = res["verdict"] == 0
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
    place, state_after, seg_stop = rm.walk(res, opt, chain["max_id"], *chain["group"], chain["state"])
    chain["place"] = place
    _, snd_after, ack_stop = ag.expect(chain)
    # the tx records: the reverse of each stream's tuple, a receive buffer, some with a probe queued
    tx = np.zeros(chain["max_id"] + 1, dtype=am.STATE_DTYPE)
    for s in ids:
        r = res[first_of[int(s)]]
        t = tx[int(s)]
        t["saddr"], t["daddr"], t["sport"], t["dport"] = r["daddr"], r["saddr"], r["dport"], r["sport"]
        t["ip_id"], t["wscale_mine"], t["link"] = rng.integers(0, 1 << 16), rng.integers(0, 8), rng.integers(0, 3)
        t["has_rcvbuf"], t["is_wack"] = 1, int(rng.random() < .1)
    g = dict(place=place, n=n, max_id=chain["max_id"], group=chain["group"], seg_stop=seg_stop, ack_stop=ack_stop,
             state=state_after, snd=snd_after, tx=tx, n_links=3, cur_ts=chain["cur_ts"], seg_cap=4096,
             buf_off=0, buf_len=128 * 4096, off_shift=6, slot_bytes=128)
    return buf, desc, ent, chain, g


def test_frames_in_ack_frames_out(gpu):
    """rx + tcpopt + lookup + group + receive walk + ACK walk + ack_send_dev on
    one stream for 4 096 frames, then the built frames back through
    rx_chunk_dev: every emitted frame is TCP_OK with the model's ack_seq,
    window and timestamps, every void record BAD_SEG with its slot untouched."""
    from mtcp_amd._types import ACK_STATE_DTYPE, RESULT_DTYPE, TCPOPT_DTYPE, TCPOPT_TS_FOUND
    buf, desc, ent, chain, g = make_chain()
    n, max_id, cap = g["n"], g["max_id"], g["seg_cap"]
    assert n == 4096
    want = gg.expect(g)
    T = int(want[3][0])
    assert 500 < T < cap, T
    d_buf, d_desc, d_ent = to_dev(buf), to_dev(desc), to_dev(ent)
    zeros = lambda k: torch.zeros(k, dtype=torch.uint8, device=DEV)
    d_res, d_opt, sid = zeros(40 * n), zeros(16 * n), Guarded(4 * n)
    grp = (Guarded(4 * n), Guarded(4 * n), Guarded(4 * n + 4), Guarded(4))
    gwork = Guarded(gpu.Context.group_work_bytes(n, max_id))
    rwork = Guarded(gpu.Context.rcvwalk_work_bytes(n, max_id))
    awork = Guarded(gpu.Context.ackwalk_work_bytes(n, max_id))
    state, snd = Guarded(64 * (max_id + 1), chain["state"]), Guarded(128 * (max_id + 1), chain["snd"])
    place, rstop, ack, astop = Guarded(16 * n), Guarded(4 * n), Guarded(16 * n), Guarded(4 * n)
    cl = Call(gpu, g, image_bytes=g["buf_len"])
    st = torch.cuda.Stream(device=DEV)
    r2, o2 = zeros(40 * cap), zeros(16 * cap)
    with gpu.Context(0) as cx, gpu.FlowTable(cx, 12) as tab:
        tab.update_dev(None, 0, d_ent, len(ent), stream=st)
        gt = tuple(x.t for x in grp)
        cx.rx_chunk_dev(d_buf, d_desc, n, 0, d_res, stream=st)
        cx.rx_tcpopt_chunk_dev(d_buf, d_desc, n, 0, d_res, d_opt, stream=st)
        tab.lookup_dev(d_res, n, sid.t, None, stream=st)
        cx.group_dev(sid.t, n, max_id, *gt, gwork.t, stream=st)
        cx.rcvwalk_dev(d_res, d_opt, n, max_id, *gt, state.t, place.t, rstop.t, rwork.t, stream=st)
        cx.ackwalk_dev(d_res, d_opt, place.t, n, max_id, *gt, g["cur_ts"], snd.t, ack.t, astop.t, awork.t, stream=st)
        cx.ack_send_dev(place.t, n, max_id, *gt, rstop.t, astop.t, state.t, snd.t, g["cur_ts"], cl.tx.t, cl.links,
                        cl.image.t, 0, 6, 128, cl.seg.t, cl.desc.t, cap, cl.ares.t, cl.total.t, cl.status.t,
                        cl.work.t, stream=st)
        cx.rx_chunk_dev(cl.image.t, cl.desc.t, cap, 6, r2, stream=st)
        cx.rx_tcpopt_chunk_dev(cl.image.t, cl.desc.t, cap, 6, r2, o2, stream=st)
        st.synchronize()
    for x in (sid, *grp, gwork, rwork, awork, state, snd, place, rstop, ack, astop, cl.image):
        assert x.guard_intact()
    assert state.numpy(g["state"].dtype).tobytes() == g["state"].tobytes()
    assert snd.numpy(ACK_STATE_DTYPE).tobytes() == g["snd"].tobytes()
    cl.check(want, "behind the walks")
    status = cl.status.numpy()
    assert (status[:T] == xm.BUILT).all() and (status[T:] == xm.BAD_SEG).all()
    image = cl.image.numpy().reshape(cap, 128)
    assert (image[T:] == SENT).all() and (image[:T, 66:] == SENT).all()
    res = r2.cpu().numpy().view(RESULT_DTYPE)[:T]
    opt = o2.cpu().numpy().view(TCPOPT_DTYPE)[:T]
    seg = want[0][:T]
    assert (res["verdict"] == 0).all()                              # TCP_OK
    assert np.array_equal(res["ack_seq"], seg["ack"]) and np.array_equal(res["window"], seg["window"])
    assert np.array_equal(res["seq"], seg["seq"]) and (res["payload_len"] == 0).all() and (res["tcp_flags"] == 0x10).all()
    assert ((opt["flags"] & TCPOPT_TS_FOUND) != 0).all()
    assert np.array_equal(opt["ts_val"], seg["ts_val"]) and np.array_equal(opt["ts_ref"], seg["ts_ecr"])
    assert (seg["ts_val"] == g["cur_ts"]).all()


# ---- past the wait limit -------------------------------------------------------------------------------------
def test_timeout_abandons(gpu):
    """The stalled-GPU pattern of tests/test_gpu_bounded.py (its helpers, its
    stall and limit values), as tests/test_gpu_rcvwalk.py does it:
    ETIMEDOUT within the limit, nothing of the caller's is written (tx[]
    included) right after the call and after the stall has ended, the context
    answers EIO to the host form and to the device forms."""
    import time
    from mtcp_amd._lib import MtcpGpuError, lib
    from tests.test_gpu_bounded import ETIMEDOUT, LIMIT_US, SLACK_S, STALL_US, stall_lib, stream_busy, stream_wait
    L, S = lib(), stall_lib()
    b = gg.make([dict(len=int(k), flags="mixed") for k in range(1, 30)], seed=95, seg_cap=600)
    want = gg.expect(b)
    idx, seg_sid, seg_start = b["group"]

    def host_call(c):
        tx = b["tx"].copy()
        try:
            out = c.ackgen(b["place"], b["max_id"], idx, seg_sid, seg_start, b["seg_stop"], b["ack_stop"], b["state"],
                           b["snd"], b["cur_ts"], tx, b["n_links"], b["buf_len"], b["seg_cap"])
            return 0, out, tx
        except MtcpGpuError as e:
            return e.code, None, tx

    c = gpu.Context(0)
    handle = c.stream
    rc, out, tx = host_call(c)                                      # unbounded: stage sized, kernels loaded
    assert rc == 0 and tx.tobytes() == want[4].tobytes()
    c.wait_limit = LIMIT_US
    rc, out, tx = host_call(c)                                      # bounded, no stall: the bounce buffers sized
    assert rc == 0 and all(g.tobytes() == e.tobytes() for g, e in zip((*out, tx), want))
    assert S.mtcp_gpu_debug_stall(c._h, STALL_US) == 0
    t0 = time.monotonic()
    rc, out, tx = host_call(c)
    dt = time.monotonic() - t0
    assert rc == ETIMEDOUT, rc
    assert dt < LIMIT_US / 1e6 + SLACK_S, dt
    assert stream_busy(handle)
    assert tx.tobytes() == b["tx"].tobytes()
    assert L.mtcp_gpu_sync(c._h) == EIO
    rc2, _, tx2 = host_call(c)
    assert rc2 == EIO and tx2.tobytes() == b["tx"].tobytes()
    own = torch.cuda.Stream(device=DEV)
    d = Call(gpu, b, image_bytes=66 * 600)
    for send in (False, True):
        with pytest.raises(MtcpGpuError) as e:
            (d.send if send else d.run)(c)
        assert e.value.code == EIO
    c.close()
    stream_wait(handle)                                             # the stall and what was queued behind it end
    own.synchronize()
    assert tx.tobytes() == b["tx"].tobytes() and tx2.tobytes() == b["tx"].tobytes()
    for x in (d.seg, d.desc, d.ares, d.total, d.work, d.status, d.image):
        assert (x.all == SENT).all().item()
    assert d.tx.numpy().tobytes() == b["tx"].tobytes()
    with gpu.Context(0) as fresh:
        fresh.wait_limit = 5_000_000
        rc, out, tx = host_call(fresh)
        assert rc == 0 and all(g.tobytes() == e.tobytes() for g, e in zip((*out, tx), want))
