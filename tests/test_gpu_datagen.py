"""Data segment generation on the GPU (include/mtcp_gpu_datagen.h,
mtcp_amd/csrc/datagen_kernels.hpp): every byte of d_seg, d_desc, d_dres[:m],
d_total, d_snd, d_tx and d_dtx of every case is compared with
tests/datagen_model.py; none is sampled.

Guard regions sit behind every output, the workspace is exactly sized and
pre-filled with 0xA5, d_dres past m keeps its sentinel, records of streams
absent from the batch keep every byte.  Segment counts around the wave and the
workgroup, list lengths around the lane threshold with the two flags on the
first, the last and both records, every status, every room cut, packed and
fixed slots at three shifts, records of random bytes, n == 0, NULL d_ack, two
workspace fills, the reference's fixture down to the frames, the host-memory
form and the error returns."""
import numpy as np
import pytest

from mtcp_amd._types import (ACK_REC_DTYPE, ACK_STATE_DTYPE, ACKGEN_STATE_DTYPE, DATAGEN_RES_DTYPE,
                             DATAGEN_STATE_DTYPE, DESC_DTYPE, RCV_STATE_DTYPE, TX_LINK_DTYPE, TX_SEG_DTYPE)
from tests import datagen_model as dm
from tests import group_model as gm
from tests import txbuild_model as xm

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EINVAL = -22
GUARD = 4096
SENT = 0xA5
FAST_RTX, REMOVE = dm.ACK_FAST_RTX, dm.ACK_SEND_LIST_REMOVE
KINDS = ("open", "cwnd", "peer_old", "control", "no_sndbuf", "empty", "behind", "beyond", "bad_dtx", "state", "idle",
         "payload_range", "host_tail", "zero_window", "mid", "bad_tx", "bad_snd", "mss12")


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
    return gpu.Context.datagen_lane_len()


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

    def numpy(self, dtype=np.uint8):
        return self.t.cpu().numpy().view(dtype)


LINKS = np.zeros(3, dtype=TX_LINK_DTYPE)
LINKS["dst"] = [[2, 0, 0, 0, 0, i] for i in range(3)]
LINKS["src"] = [[2, 1, 0, 0, 0, i] for i in range(3)]
ROOMY = dict(buf_off=0, buf_len=1 << 40, off_shift=0, slot_bytes=0)


def make(streams, seed=1, n_miss=0, n_none=0, with_ack=True, seg_cap=None, **room):
    """A batch: streams is a list of dicts with len (packets), kind (KINDS) and
    flags ({position: flag bits} on the stream's list)."""
    rng = np.random.default_rng(seed)
    S = len(streams)
    max_id = max(2 * S, 7)
    ids = rng.choice(max_id + 1, size=S, replace=False).astype(np.uint32)
    sid = np.concatenate([np.full(int(s["len"]), ids[i], np.uint32) for i, s in enumerate(streams)] +
                         [np.full(n_miss, gm.FLOW_MISS, np.uint32), np.full(n_none, gm.FLOW_NONE, np.uint32)])
    sid = sid[rng.permutation(len(sid))]
    n = len(sid)
    R = max_id + 1
    snd = np.zeros(R, dtype=ACK_STATE_DTYPE)
    snd["user"] = rng.integers(0, 256, (R, 40))
    mss = rng.choice([13, 14, 64, 536], R)
    snd["mss"], snd["eff_mss"] = mss, mss - 12
    snd["sb_head_seq"] = rng.integers(0, 1 << 32, R, dtype=np.uint64)
    snd.view(np.uint8).reshape(R, 128)[::5, 64:68] = 0xFF                       # some heads near the wrap
    snd["sb_len"] = (mss - 12) * rng.integers(0, 5, R) + rng.integers(1, 12, R)
    snd["sb_size"], snd["tcp_state"], snd["has_sndbuf"] = 1 << 16, 4, 1
    snd["snd_una"] = snd["snd_nxt"] = snd["sb_head_seq"]
    snd["cwnd"] = snd["sb_len"] + rng.integers(0, 3000, R)
    snd["peer_wnd"] = snd["sb_len"] + rng.integers(0, 3000, R)
    snd["rto"], snd["ts_rto"] = rng.integers(1, 3000, R), rng.integers(0, 1 << 32, R, dtype=np.uint64)
    snd["on_rto"] = rng.integers(0, 2, R)
    state = np.zeros(R, dtype=RCV_STATE_DTYPE)
    for f in ("rcv_nxt", "ts_recent"):
        state[f] = rng.integers(0, 1 << 32, R, dtype=np.uint64)
    state["rcv_wnd"], state["tcp_state"] = rng.integers(1 << 15, 1 << 22, R), 4
    tx = np.zeros(R, dtype=ACKGEN_STATE_DTYPE)
    for f in ("saddr", "daddr", "ts_lastack_sent"):
        tx[f] = rng.integers(0, 1 << 32, R, dtype=np.uint64)
    for f in ("sport", "dport"):
        tx[f] = rng.integers(0, 1 << 16, R)
    tx["ip_id"] = np.where(rng.random(R) < 0.2, 65535, rng.integers(0, 1 << 16, R))
    tx["ack_cnt"], tx["wscale_mine"], tx["link"] = rng.integers(0, 8, R), rng.integers(0, 15, R), rng.integers(0, 3, R)
    tx["has_rcvbuf"] = 1
    dtx = np.zeros(R, dtype=DATAGEN_STATE_DTYPE)
    dtx["on_send_list"] = 1
    back = rng.integers(0, 50, R)                                              # the pair refers to a byte behind the head
    dtx["sb_base_seq"] = snd["sb_head_seq"] - back
    at = 1
    for i in range(R):
        dtx[i]["sb_off"] = at
        at += int(back[i]) + int(snd[i]["sb_len"]) + 1 + 2 * int(rng.integers(0, 3))
    payload = rng.integers(0, 256, at + 8, dtype=np.uint8)
    cur_ts = int(rng.integers(0, 1 << 32))
    idx, seg_sid, seg_start = gm.group(sid, max_id)
    seg_stop = seg_start[1:].copy()
    seg_stop[seg_sid > max_id] = seg_start[:-1][seg_sid > max_id]
    ack_stop = seg_stop.copy()
    ack = np.zeros(n, dtype=ACK_REC_DTYPE)
    ack["verdict"], ack["flags"] = 12, rng.integers(0, 1 << 9, n) & ~(FAST_RTX | REMOVE)
    seg_of = {int(s): j for j, s in enumerate(seg_sid)}
    for i, s in enumerate(streams):
        r, k, kind = int(ids[i]), int(s["len"]), s.get("kind", "open")
        at_pk = np.nonzero(sid == ids[i])[0]
        for pos, fl in s.get("flags", {}).items():
            ack["flags"][at_pk[pos]] |= fl
        sb_len, m1 = int(snd[r]["sb_len"]), int(mss[r]) - 12
        if kind == "cwnd":
            snd[r]["cwnd"] = int(rng.integers(0, sb_len))
        elif kind == "peer_old":
            snd[r]["peer_wnd"] = int(rng.integers(0, min(sb_len, m1)))
            tx[r]["ts_lastack_sent"] = (cur_ts - int(rng.choice([499, 500, 501, 502, 4294968, 4295469]))) & dm.M32
        elif kind == "control":
            dtx[r]["on_control_list"] = 1
        elif kind == "no_sndbuf":
            snd[r]["has_sndbuf"] = 0
        elif kind == "empty":
            snd[r]["sb_len"] = 0
        elif kind == "behind":
            snd[r]["snd_nxt"] = snd[r]["snd_una"] = (int(snd[r]["sb_head_seq"]) - 1 - int(rng.integers(0, 99))) & dm.M32
        elif kind == "beyond":
            snd[r]["snd_nxt"] = (int(snd[r]["sb_head_seq"]) + sb_len + 1) & dm.M32
        elif kind == "bad_dtx":
            dtx[r]["rsvd"][int(rng.integers(0, 2))] = 1
        elif kind == "bad_tx":
            tx[r]["link"] = 3
        elif kind == "bad_snd":
            snd[r]["eff_mss"] = 0
        elif kind == "state":
            (snd if rng.integers(0, 2) else state)[r]["tcp_state"] = 5
        elif kind == "idle":
            dtx[r]["on_send_list"] = 0
        elif kind == "payload_range":
            dtx[r]["sb_off"] = len(payload) - sb_len + 1
        elif kind == "host_tail" and k > 1:
            j = seg_of[r]
            (ack_stop if rng.integers(0, 2) else seg_stop)[j] = seg_start[j] + int(rng.integers(0, k))
        elif kind == "zero_window":
            tx[r]["wscale_mine"], state[r]["rcv_wnd"] = 14, int(rng.integers(0, 1 << 14))
        elif kind == "mid":
            snd[r]["snd_nxt"] = (int(snd[r]["sb_head_seq"]) + int(rng.integers(0, sb_len + 1))) & dm.M32
        elif kind == "mss12":
            snd[r]["mss"] = 12
    m = len(seg_sid)
    b = dict(n=n, max_id=max_id, ids=ids, idx=idx, seg_sid=seg_sid, seg_start=seg_start, seg_stop=seg_stop,
             ack=ack if with_ack else None, ack_stop=ack_stop if with_ack else None, state=state, snd=snd, tx=tx,
             dtx=dtx, cur_ts=cur_ts, payload=payload, n_links=3, seg_cap=seg_cap if seg_cap is not None else 6 * m + 3)
    b.update(ROOMY)
    b.update(room)
    return b


def expect(b, nseg=None):
    return dm.run_batch(b, b.get("ack"), b.get("ack_stop"), nseg)[:7]


class Call:
    """The device arrays of one call on batch b, the outputs guarded."""

    def __init__(self, gpu, b, nseg=None, image_bytes=0, work_fill=SENT):
        self.b, n, R = b, b["n"], b["max_id"] + 1
        self.m = min(len(b["seg_sid"]) if nseg is None else nseg, n)
        pad = lambda a, k: np.concatenate([a, np.full(max(k - len(a), 0), 0xA5A5A5A5, np.uint32)]).astype(np.uint32)
        self.ack = None if b.get("ack") is None else to_dev(b["ack"] if n else np.zeros(1, ACK_REC_DTYPE))
        self.ack_stop = None if b.get("ack_stop") is None else to_dev(pad(b["ack_stop"], max(n, 1)))
        self.idx, self.seg_sid = to_dev(pad(b["idx"], 1)), to_dev(pad(b["seg_sid"], max(n, 1)))
        self.seg_start = to_dev(pad(b["seg_start"], n + 1))
        self.nseg = to_dev(np.array([len(b["seg_sid"]) if nseg is None else nseg], np.uint32))
        self.seg_stop = to_dev(pad(b["seg_stop"], max(n, 1)))
        self.state = to_dev(b["state"])
        self.snd, self.tx, self.dtx = Guarded(128 * R, b["snd"]), Guarded(32 * R, b["tx"]), Guarded(16 * R, b["dtx"])
        cap = b["seg_cap"]
        self.seg, self.desc = Guarded(48 * cap), Guarded(8 * cap)
        self.dres, self.total, self.status = Guarded(16 * max(n, 1)), Guarded(16), Guarded(cap)
        self.wb = gpu.Context.datagen_work_bytes(n, b["max_id"])
        assert self.wb > 0
        self.work = Guarded(self.wb, work_fill)
        self.payload = to_dev(b["payload"])
        self.image = Guarded(image_bytes) if image_bytes else None
        self.links = to_dev(LINKS)

    def args(self):
        b = self.b
        return (self.ack, self.ack_stop, b["n"], b["max_id"], self.idx, self.seg_sid, self.seg_start, self.nseg,
                self.seg_stop, self.state, self.snd.t, self.tx.t, self.dtx.t, b["cur_ts"])

    def run(self, ctx, stream=None):
        b = self.b
        ctx.datagen_dev(*self.args(), len(b["payload"]), b["n_links"], b["buf_off"], b["buf_len"], b["off_shift"],
                        b["slot_bytes"], self.seg.t, self.desc.t, b["seg_cap"], self.dres.t, self.total.t, self.work.t,
                        max_mss=b.get("max_mss", 0), stream=stream)

    def send(self, ctx):
        b = self.b
        ctx.data_send_dev(*self.args(), self.payload, self.links, self.image.t, b["buf_off"], b["off_shift"],
                          b["slot_bytes"], self.seg.t, self.desc.t, b["seg_cap"], self.dres.t, self.total.t,
                          self.status.t, self.work.t, buf_len=min(b["buf_len"], self.image.nbytes))

    def outputs(self):
        return (self.seg.numpy(TX_SEG_DTYPE), self.desc.numpy(DESC_DTYPE), self.dres.numpy(DATAGEN_RES_DTYPE),
                self.total.numpy(np.uint64), self.snd.numpy(ACK_STATE_DTYPE), self.tx.numpy(ACKGEN_STATE_DTYPE),
                self.dtx.numpy(DATAGEN_STATE_DTYPE))

    def check(self, want, what=""):
        for name in ("snd", "tx", "dtx", "seg", "desc", "dres", "total", "work", "status"):
            assert getattr(self, name).guard_intact(), f"{what}: bytes behind {name} were written"
        got = self.outputs()
        m = len(want[2])
        assert m == self.m
        for g, e, name in zip(got, want, ("seg", "desc", "dres", "total", "snd", "tx", "dtx")):
            g = g[:m] if name == "dres" else g
            if g.tobytes() != e.tobytes():
                bad = [i for i in range(len(e)) if g[i].tobytes() != e[i].tobytes()]
                raise AssertionError(f"{what}: {len(bad)} of {len(e)} {name} records differ, first at {bad[0]}: "
                                     f"{g[bad[0]]} want {e[bad[0]]}")
        assert (got[2][m:].view(np.uint8) == SENT).all(), f"{what}: dres past m was written"
        return got


def mixed_streams(m, rng, maxlen=6):
    out, other = [], 0
    for i in range(m):
        k = int(rng.integers(1, maxlen + 1))
        flags = {}
        if rng.random() < 0.4:
            flags[int(rng.integers(0, k))] = int(rng.choice([FAST_RTX, REMOVE, FAST_RTX | REMOVE]))
        if rng.random() < 0.2:
            flags[int(rng.integers(0, k))] = int(rng.choice([FAST_RTX, REMOVE]))
        out.append(dict(len=k, kind=KINDS[other % len(KINDS)] if i % 3 else "open", flags=flags))
        other += 1 if i % 3 else 0
    return out


@pytest.mark.parametrize("m", [1, 63, 64, 65, 257])
def test_segment_counts_and_every_status(gpu, ctx, m):
    rng = np.random.default_rng(m)
    b = make(mixed_streams(m, rng), seed=m, n_miss=3 if m > 1 else 0, n_none=2 if m > 1 else 0,
             seg_cap=400 if m == 257 else None)                             # 257: the room ends inside the batch
    c = Call(gpu, b)
    c.run(ctx)
    got = c.check(expect(b), f"m={m}")
    if m == 257:
        assert set(range(12)) == set(int(s) for s in got[2][:c.m]["status"])
        fl = np.bitwise_or.reduce(got[2][:c.m]["flags"])
        assert fl == 0x1F, hex(fl)
        absent = np.setdiff1d(np.arange(b["max_id"] + 1), b["ids"])
        for k, name in ((4, "snd"), (5, "tx"), (6, "dtx")):
            assert got[k][absent].tobytes() == b[name][absent].tobytes()


@pytest.mark.parametrize("where", ["first", "last", "both"])
def test_list_lengths_around_the_lane_length(gpu, ctx, LANE, where):
    streams = []
    for k in (LANE - 1, LANE, LANE + 1, 2 * LANE + 1):
        for first, last in ((FAST_RTX, REMOVE), (REMOVE, FAST_RTX), (FAST_RTX | REMOVE, 0), (0, FAST_RTX | REMOVE)):
            for on in ("open", "idle"):
                fl = {0: first} if where == "first" else {k - 1: last or first} if where == "last" else \
                    {0: first, k - 1: last}
                streams.append(dict(len=k, kind=on, flags=fl))
    b = make(streams, seed=LANE)
    c = Call(gpu, b)
    c.run(ctx)
    got = c.check(expect(b), where)
    assert {dm.IDLE, dm.SENT} <= set(int(s) for s in got[2][:c.m]["status"])


def test_room_cuts_slots_and_shifts(gpu, ctx):
    rng = np.random.default_rng(3)
    streams = [dict(len=int(rng.integers(1, 4)), kind="open" if i % 4 else "cwnd") for i in range(40)]
    for off_shift in (0, 1, 6):
        A = max(2, 1 << off_shift)
        for slot_bytes in (0, 640):
            b = make(streams, seed=9, buf_off=4 * A, off_shift=off_shift, slot_bytes=slot_bytes)
            _, desc, _, total, *_ = expect(b)
            T = int(total[0])
            assert T > 20
            cut = T // 2
            end = (int(desc[cut - 1]["offset"]) << off_shift) + int(desc[cut - 1]["len"])
            far = ((0xFFFFFFFF << off_shift) // A + 1) * A - ((int(desc[cut]["offset"]) << off_shift) - 4 * A)
            for what, over in (("none", {}), ("seg_cap", dict(seg_cap=cut)), ("buf_len", dict(buf_len=end)),
                               ("buf_len_short", dict(buf_len=end - 1)), ("offset", dict(buf_off=far, buf_len=1 << 62)),
                               ("exact", dict(seg_cap=T))):
                bb = dict(b, **over)
                c = Call(gpu, bb)
                c.run(ctx)
                got = c.check(expect(bb), f"shift {off_shift} slot {slot_bytes} {what}")
                if what in ("seg_cap", "buf_len", "offset"):
                    assert int(got[3][0]) == cut and dm.NO_ROOM in got[2][:c.m]["status"]


def test_random_bytes_in_every_record(gpu, ctx):
    rng = np.random.default_rng(17)
    b = make(mixed_streams(130, rng), seed=17, n_miss=5)
    R = b["max_id"] + 1
    for name, dt in (("snd", ACK_STATE_DTYPE), ("tx", ACKGEN_STATE_DTYPE), ("dtx", DATAGEN_STATE_DTYPE),
                     ("state", RCV_STATE_DTYPE)):
        raw = np.frombuffer(rng.bytes(dt.itemsize * R), dtype=dt).copy()
        keep = rng.random(R) < 0.5                                            # every second record stays sane
        raw[keep] = b[name][keep]
        b[name] = raw
    b["ack"] = np.frombuffer(rng.bytes(16 * b["n"]), dtype=ACK_REC_DTYPE).copy()
    c = Call(gpu, b)
    c.run(ctx)
    got = c.check(expect(b), "random bytes")
    assert dm.BAD in got[2][:c.m]["status"]


def test_n_zero_null_ack_nseg_clamp_and_workspace_fills(gpu, ctx):
    rng = np.random.default_rng(23)
    b = make(mixed_streams(70, rng), seed=23)
    e = dict(b, n=0, idx=b["idx"][:0], seg_sid=b["seg_sid"][:0], seg_start=b["seg_start"][:1],
             seg_stop=b["seg_stop"][:0], ack=b["ack"][:0], ack_stop=b["ack_stop"][:0], seg_cap=5)
    c = Call(gpu, e)
    c.run(ctx)
    c.check(expect(e), "n == 0")
    nb = dict(b, ack=None, ack_stop=None)
    c = Call(gpu, nb)
    c.run(ctx)
    c.check(expect(nb), "NULL d_ack")
    # d_nseg above n is clamped to n: the table padded to n entries with NONE segments
    big = dict(b, seg_sid=np.concatenate([b["seg_sid"], np.full(b["n"] - len(b["seg_sid"]), gm.FLOW_NONE, np.uint32)]),
               seg_start=np.concatenate([b["seg_start"], np.full(b["n"] - len(b["seg_sid"]), b["n"], np.uint32)]),
               seg_stop=np.concatenate([b["seg_stop"], np.full(b["n"] - len(b["seg_sid"]), b["n"], np.uint32)]),
               ack_stop=np.concatenate([b["ack_stop"], np.full(b["n"] - len(b["seg_sid"]), b["n"], np.uint32)]))
    c = Call(gpu, big, nseg=0xFFFFFFFF)
    c.run(ctx)
    c.check(expect(big, nseg=0xFFFFFFFF), "nseg clamped")
    outs = []
    for fill in (0x00, 0xFF):
        c = Call(gpu, b, work_fill=fill)
        c.run(ctx)
        outs.append([a.tobytes() for a in c.check(expect(b), f"workspace {fill:#x}")])
    assert outs[0] == outs[1]


def test_fixture_through_data_send_dev(gpu, ctx):
    from tests import ackgen_model as am
    links = am.fixture_links()
    for i, case in enumerate(dm.load_fixture()):
        b = dm.case_batch(case)
        b["ack"] = b["ack_stop"] = None
        want = expect(b)
        c = Call(gpu, b, image_bytes=max(b["buf_len"], 16))
        c.image.t.zero_()
        c.send(ctx)
        got = c.check(want, f"fixture case {i}")
        image, status = xm.build_frames(want[0], b["payload"], links, want[1], np.zeros(c.image.nbytes, np.uint8))
        assert c.image.guard_intact() and c.image.numpy().tobytes() == image.tobytes(), i
        assert c.status.numpy().tobytes() == status.tobytes(), i
        k = 0
        for s in case["streams"]:
            for f in s["frames"]:
                at = int(got[1][k]["offset"])
                assert c.image.numpy()[at:at + len(f)].tobytes() == f.tobytes(), (i, k)
                k += 1
        assert k == int(got[3][0])


def test_host_form_without_and_with_a_wait_limit(gpu, ctx):
    rng = np.random.default_rng(31)
    b = make(mixed_streams(90, rng), seed=31, buf_len=1 << 30)
    want = expect(b)
    for limit in (0, 30_000_000):
        ctx.wait_limit = limit
        try:
            snd, tx, dtx = b["snd"].copy(), b["tx"].copy(), b["dtx"].copy()
            seg, desc, dres, total = ctx.datagen(b["ack"], b["ack_stop"], b["max_id"], b["idx"], b["seg_sid"],
                                                 b["seg_start"], b["seg_stop"], b["state"], snd, tx, dtx, b["cur_ts"],
                                                 len(b["payload"]), b["n_links"], b["buf_len"], b["seg_cap"])
        finally:
            ctx.wait_limit = 0
        for g, e, name in zip((seg, desc, dres, total, snd, tx, dtx), want,
                              ("seg", "desc", "dres", "total", "snd", "tx", "dtx")):
            assert g.tobytes() == e.tobytes(), (limit, name)


def test_error_returns(gpu, ctx):
    """MTCP_GPU_EINVAL for each misuse the header lists, for every pointer of
    mtcp_gpu_datagen_dev, mtcp_gpu_data_send_dev and mtcp_gpu_datagen; d_ack and
    d_ack_stop both NULL is accepted; a refused call launches nothing and
    writes nothing.  MTCP_GPU_EIO on an abandoned context is not tested: a
    context is abandoned only by a call that outlasts its wait limit, which
    takes a stalled GPU."""
    from mtcp_amd._lib import lib
    L = lib()
    rng = np.random.default_rng(41)
    b = make(mixed_streams(20, rng), seed=41, seg_cap=200)
    want = expect(b)
    n, max_id, cap, ts, pb = b["n"], b["max_id"], b["seg_cap"], b["cur_ts"], len(b["payload"])
    d = Call(gpu, b, image_bytes=1 << 16)
    room = Guarded(64)                                               # misaligned stand-ins, never dereferenced
    p = lambda t, off=0: t.data_ptr() + off
    big, MAX_ID = (1 << 24) + 1, gm.MAX_ID

    def dev(c=ctx._h, ak=p(d.ack), asp=p(d.ack_stop), n_=n, mx=max_id, i=p(d.idx), ss=p(d.seg_sid), st=p(d.seg_start),
            ns=p(d.nseg), sp=p(d.seg_stop), s=p(d.state), sn=p(d.snd.t), tx=p(d.tx.t), dt=p(d.dtx.t), nl=3, bo=0,
            bl=1 << 40, sh=0, sb=0, sg=p(d.seg.t), de=p(d.desc.t), cp=cap, dr=p(d.dres.t), to=p(d.total.t), w=p(d.work.t),
            wbytes=d.wb):
        return L.mtcp_gpu_datagen_dev(c, ak, asp, n_, mx, i, ss, st, ns, sp, s, sn, tx, dt, ts, pb, nl, bo, bl, sh, sb, 0,
                                      sg, de, cp, dr, to, w, wbytes, None)

    def send(c=ctx._h, ak=p(d.ack), asp=p(d.ack_stop), i=p(d.idx), ss=p(d.seg_sid), st=p(d.seg_start), ns=p(d.nseg),
             sp=p(d.seg_stop), s=p(d.state), sn=p(d.snd.t), tx=p(d.tx.t), dt=p(d.dtx.t), pl=p(d.payload), pbytes=pb,
             lk=p(d.links), nl=3, bf=p(d.image.t), bo=0, bl=1 << 16, sh=0, sb=0, fl=0, sg=p(d.seg.t), de=p(d.desc.t),
             cp=cap, dr=p(d.dres.t), to=p(d.total.t), su=p(d.status.t), w=p(d.work.t), wbytes=d.wb):
        return L.mtcp_gpu_data_send_dev(c, ak, asp, n, max_id, i, ss, st, ns, sp, s, sn, tx, dt, ts, pl, pbytes, lk, nl, bf,
                                        bo, bl, sh, sb, 0, fl, sg, de, cp, dr, to, su, w, wbytes, None)

    bad = {
        "ctx NULL": dev(c=None), "ack NULL alone": dev(ak=None), "ack_stop NULL alone": dev(asp=None),
        "idx NULL": dev(i=None), "seg_sid NULL": dev(ss=None), "seg_start NULL": dev(st=None), "nseg NULL": dev(ns=None),
        "seg_stop NULL": dev(sp=None), "state NULL": dev(s=None), "snd NULL": dev(sn=None), "tx NULL": dev(tx=None),
        "dtx NULL": dev(dt=None), "seg NULL": dev(sg=None), "desc NULL": dev(de=None), "dres NULL": dev(dr=None),
        "total NULL": dev(to=None), "work NULL": dev(w=None), "seg NULL, n 0": dev(n_=0, sg=None),
        "desc NULL, n 0": dev(n_=0, de=None), "total NULL, n 0": dev(n_=0, to=None), "work NULL, n 0": dev(n_=0, w=None),
        "ack misaligned": dev(ak=p(room.t, 8)), "ack_stop misaligned": dev(asp=p(room.t, 2)),
        "idx misaligned": dev(i=p(room.t, 2)), "seg_sid misaligned": dev(ss=p(room.t, 1)),
        "seg_start misaligned": dev(st=p(room.t, 3)), "nseg misaligned": dev(ns=p(room.t, 2)),
        "seg_stop misaligned": dev(sp=p(room.t, 2)), "state misaligned by 32": dev(s=p(d.state, 32)),
        "snd misaligned by 64": dev(sn=p(d.snd.t, 64)), "tx misaligned by 16": dev(tx=p(d.tx.t, 16)),
        "dtx misaligned by 8": dev(dt=p(d.dtx.t, 8)), "seg misaligned": dev(sg=p(d.seg.t, 4)),
        "desc misaligned": dev(de=p(d.desc.t, 4)), "dres misaligned": dev(dr=p(d.dres.t, 8)),
        "total misaligned": dev(to=p(d.total.t, 4)), "work misaligned": dev(w=p(d.work.t, 8)),
        "work too small": dev(wbytes=d.wb - 1), "no work bytes": dev(wbytes=0), "n too large": dev(n_=big),
        "max_id too large": dev(mx=MAX_ID + 1), "seg_cap 0": dev(cp=0), "seg_cap too large": dev(cp=(1 << 26) + 1),
        "off_shift 17": dev(sh=17), "n_links 0": dev(nl=0), "n_links 257": dev(nl=257), "slot below 67": dev(sb=66),
        "slot odd": dev(sb=641), "slot not a multiple of A": dev(sb=96, sh=6), "buf_off odd": dev(bo=1),
        "buf_off not a multiple of A": dev(bo=32, sh=6),
        "send: ctx NULL": send(c=None), "send: ack NULL alone": send(ak=None), "send: ack_stop NULL alone": send(asp=None),
        "send: idx NULL": send(i=None), "send: seg_sid NULL": send(ss=None), "send: seg_start NULL": send(st=None),
        "send: nseg NULL": send(ns=None), "send: seg_stop NULL": send(sp=None), "send: state NULL": send(s=None),
        "send: snd NULL": send(sn=None), "send: tx NULL": send(tx=None), "send: dtx NULL": send(dt=None),
        "send: payload NULL": send(pl=None), "send: links NULL": send(lk=None), "send: buf NULL": send(bf=None),
        "send: seg NULL": send(sg=None), "send: desc NULL": send(de=None), "send: dres NULL": send(dr=None),
        "send: total NULL": send(to=None), "send: status NULL": send(su=None), "send: work NULL": send(w=None),
        "send: links misaligned": send(lk=p(d.links, 2)), "send: dtx misaligned": send(dt=p(d.dtx.t, 8)),
        "send: ack misaligned": send(ak=p(room.t, 8)), "send: unknown builder flags": send(fl=2),
        "send: payload inside buf": send(pl=p(d.image.t, 64), pbytes=128), "send: seg_cap 0": send(cp=0),
        "send: off_shift 17": send(sh=17), "send: n_links 0": send(nl=0), "send: n_links 257": send(nl=257),
        "send: slot below 67": send(sb=66), "send: slot not a multiple of A": send(sb=96, sh=6),
        "send: buf_off odd": send(bo=1), "send: work too small": send(wbytes=d.wb - 1),
    }
    with gpu.Context(0, compact=True) as cc:
        bad["compact context"], bad["send: compact context"] = dev(c=cc._h), send(c=cc._h)
        u32 = lambda a: np.ascontiguousarray(a, dtype=np.uint32)
        ack, idx, seg_sid, seg_start = np.ascontiguousarray(b["ack"]), u32(b["idx"]), u32(b["seg_sid"]), u32(b["seg_start"])
        h_stop, h_astop = u32(b["seg_stop"]), u32(b["ack_stop"])
        nseg = np.array([len(seg_sid)], np.uint32)
        h_snd, h_tx, h_dtx = b["snd"].copy(), b["tx"].copy(), b["dtx"].copy()
        h_seg, h_desc = np.full(48 * cap, SENT, np.uint8), np.full(8 * cap, SENT, np.uint8)
        h_dres, h_total = np.full(16 * n, SENT, np.uint8), np.full(16, SENT, np.uint8)
        hp = lambda a: a.ctypes.data

        def host(c=ctx._h, ak=hp(ack), asp=hp(h_astop), n_=n, mx=max_id, i=hp(idx), ss=hp(seg_sid), st=hp(seg_start),
                 ns=hp(nseg), sp=hp(h_stop), s=hp(b["state"]), sn=hp(h_snd), tx=hp(h_tx), dt=hp(h_dtx), nl=3, bo=0,
                 bl=1 << 40, sh=0, sb=0, sg=hp(h_seg), de=hp(h_desc), cp=cap, dr=hp(h_dres), to=hp(h_total)):
            return L.mtcp_gpu_datagen(c, ak, asp, n_, mx, i, ss, st, ns, sp, s, sn, tx, dt, ts, pb, nl, bo, bl, sh, sb, 0,
                                      sg, de, cp, dr, to)

        bad.update({
            "host: ctx NULL": host(c=None), "host: ack NULL alone": host(ak=None), "host: ack_stop NULL alone": host(asp=None),
            "host: idx NULL": host(i=None), "host: seg_sid NULL": host(ss=None), "host: seg_start NULL": host(st=None),
            "host: nseg NULL": host(ns=None), "host: seg_stop NULL": host(sp=None), "host: state NULL": host(s=None),
            "host: snd NULL": host(sn=None), "host: tx NULL": host(tx=None), "host: dtx NULL": host(dt=None),
            "host: seg NULL": host(sg=None), "host: desc NULL": host(de=None), "host: dres NULL": host(dr=None),
            "host: total NULL": host(to=None), "host: seg NULL, n 0": host(n_=0, sg=None),
            "host: total NULL, n 0": host(n_=0, to=None), "host: n too large": host(n_=big),
            "host: max_id too large": host(mx=MAX_ID + 1), "host: seg_cap 0": host(cp=0),
            "host: seg_cap too large": host(cp=(1 << 26) + 1), "host: off_shift 17": host(sh=17),
            "host: n_links 0": host(nl=0), "host: n_links 257": host(nl=257), "host: slot below 67": host(sb=66),
            "host: slot not a multiple of A": host(sb=96, sh=6), "host: buf_off odd": host(bo=1),
            "host: compact context": host(c=cc._h)})
    assert {k: v for k, v in bad.items() if v != EINVAL} == {}
    torch.cuda.synchronize()
    for g in (d.seg, d.desc, d.dres, d.total, d.work, d.status, d.image):    # none of these wrote anything
        assert (g.all == SENT).all().item()
    for g, name in ((d.snd, "snd"), (d.tx, "tx"), (d.dtx, "dtx")):
        assert g.numpy().tobytes() == b[name].tobytes() and g.guard_intact()
    assert all((a == SENT).all() for a in (h_seg, h_desc, h_dres, h_total))
    assert all(h.tobytes() == b[k].tobytes() for h, k in ((h_snd, "snd"), (h_tx, "tx"), (h_dtx, "dtx")))
    assert gpu.Context.datagen_work_bytes(big, 7) == 0 and gpu.Context.datagen_work_bytes(7, MAX_ID + 1) == 0
    assert dev(ak=None, asp=None, n_=0) == 0                       # n == 0 needs none of the batch's arrays
    d.seg.t.fill_(SENT), d.desc.t.fill_(SENT), d.total.t.fill_(SENT)
    assert dev() == 0 and host() == 0                               # and the same arguments, valid, work
    torch.cuda.synchronize()
    d.check(want, "after the refused calls")
    m = len(want[2])
    for g, e in ((h_seg, want[0]), (h_desc, want[1]), (h_dres[:16 * m], want[2]), (h_total, want[3]), (h_snd, want[4]),
                 (h_tx, want[5]), (h_dtx, want[6])):
        assert g.tobytes() == e.tobytes()
