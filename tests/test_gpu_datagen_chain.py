"""Frames in, data frames out (include/mtcp_gpu_datagen.h): rx + tcpopt +
lookup + group + receive walk + ACK walk + ack_send_dev + data_send_dev on one
stream for the 4 096 stateful frames of tests/test_gpu_ackgen.py's chain, so
that the data call reads the ACK walk's own FAST_RTX / SEND_LIST_REMOVE records
and rewound snd_nxt and the d_tx that ack_send_dev left.  Every byte of the
data call's outputs and of d_snd, d_tx and d_dtx is compared with the models
chained the same way; the built data frames go back through rx_chunk_dev and
must be TCP_OK records equal to the oracle's for the model's image.  Then the
chain's tail (ACK walk, ack_send_dev, data_send_dev) is captured on one stream
and replayed twice from reset state."""
import numpy as np
import pytest

from mtcp_amd._types import (ACK_REC_DTYPE, ACK_STATE_DTYPE, DATAGEN_STATE_DTYPE, RESULT_DTYPE)
from tests import datagen_model as dm
from tests import txbuild_model as xm
from tests.test_gpu_datagen import DEV, SENT, Call, Guarded, to_dev

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")
    from mtcp_amd import gpu as g
    return g


def make_data_chain():
    """The ACK chain of tests/test_gpu_ackgen.py with the send side behind it:
    a payload arena holding every stream's send buffer as it was before the
    batch, the d_dtx records that place them, and the models' answers."""
    from tests import ackgen_gen as gg
    from tests import ackwalk_gen as ag
    from tests.test_gpu_ackgen import make_chain
    buf, desc, ent, chain, g = make_chain()
    ack, snd_after, ack_stop = ag.expect(chain)
    assert snd_after.tobytes() == g["snd"].tobytes()
    want_ack = gg.expect(g)
    rng = np.random.default_rng(15)
    R = g["max_id"] + 1
    ids = np.unique(chain["sid"][chain["sid"] <= g["max_id"]])
    dtx = np.zeros(R, dtype=DATAGEN_STATE_DTYPE)
    at = 1
    for s in ids:
        s0 = chain["snd"][int(s)]
        dtx[int(s)]["sb_off"], dtx[int(s)]["sb_base_seq"] = at, s0["sb_head_seq"]      # as the host's last SBPut left them
        dtx[int(s)]["on_send_list"] = int(rng.random() < 0.5)
        dtx[int(s)]["on_control_list"] = int(rng.random() < 0.03)
        at += int(s0["sb_len"]) + 1 + 2 * int(rng.integers(0, 3))
    payload = rng.integers(0, 256, at + 64, dtype=np.uint8)
    idx, seg_sid, seg_start = g["group"]
    b = dict(n=g["n"], max_id=g["max_id"], idx=idx, seg_sid=seg_sid, seg_start=seg_start, seg_stop=g["seg_stop"],
             ack=ack, ack_stop=ack_stop, state=g["state"], snd=snd_after, tx=want_ack[4], dtx=dtx, cur_ts=g["cur_ts"],
             payload=payload, n_links=3, buf_off=0, buf_len=1 << 40, off_shift=6, slot_bytes=0, seg_cap=1 << 16)
    total = dm.run_batch(b, ack, ack_stop)[3]
    b["buf_len"], b["seg_cap"] = int(total[1]), int(total[0]) + 37                      # the ring's free bytes, exactly
    want = dm.run_batch(b, ack, ack_stop)[:7]
    return dict(buf=buf, desc=desc, ent=ent, chain=chain, g=g, b=b, want=want, want_ack=want_ack)


@pytest.fixture(scope="module")
def data_chain():
    return make_data_chain()


class DataChain:
    """The device arrays of the whole chain; the two senders' outputs guarded."""

    def __init__(self, gpu, dc):
        from tests.test_gpu_ackgen import Call as AckCall
        self.dc, g, b = dc, dc["g"], dc["b"]
        n, max_id = g["n"], g["max_id"]
        self.n, self.max_id = n, max_id
        self.d_buf, self.d_desc, self.d_ent = to_dev(dc["buf"]), to_dev(dc["desc"]), to_dev(dc["ent"])
        zeros = lambda k: torch.zeros(k, dtype=torch.uint8, device=DEV)
        self.d_res, self.d_opt, self.sid = zeros(40 * n), zeros(16 * n), Guarded(4 * n)
        self.grp = (Guarded(4 * n), Guarded(4 * n), Guarded(4 * n + 4), Guarded(4))
        self.gwork = Guarded(gpu.Context.group_work_bytes(n, max_id))
        self.rwork = Guarded(gpu.Context.rcvwalk_work_bytes(n, max_id))
        self.awork = Guarded(gpu.Context.ackwalk_work_bytes(n, max_id))
        self.state = Guarded(64 * (max_id + 1), dc["chain"]["state"])
        self.place, self.rstop, self.ack, self.astop = Guarded(16 * n), Guarded(4 * n), Guarded(16 * n), Guarded(4 * n)
        self.ac = AckCall(gpu, g, image_bytes=g["buf_len"])                 # its tx is the chain's d_tx
        self.c = Call(gpu, dict(b, snd=dc["chain"]["snd"], tx=g["tx"]), image_bytes=b["buf_len"])
        self.c.tx = self.ac.tx                                              # one d_tx for both senders
        self.r2 = zeros(40 * b["seg_cap"])

    def head(self, cx, tab, st):
        n, max_id, gt = self.n, self.max_id, tuple(x.t for x in self.grp)
        cx.rx_chunk_dev(self.d_buf, self.d_desc, n, 0, self.d_res, stream=st)
        cx.rx_tcpopt_chunk_dev(self.d_buf, self.d_desc, n, 0, self.d_res, self.d_opt, stream=st)
        tab.lookup_dev(self.d_res, n, self.sid.t, None, stream=st)
        cx.group_dev(self.sid.t, n, max_id, *gt, self.gwork.t, stream=st)
        cx.rcvwalk_dev(self.d_res, self.d_opt, n, max_id, *gt, self.state.t, self.place.t, self.rstop.t, self.rwork.t,
                       stream=st)

    def tail(self, cx, st):
        n, max_id, gt = self.n, self.max_id, tuple(x.t for x in self.grp)
        g, b, ac, c = self.dc["g"], self.dc["b"], self.ac, self.c
        cx.ackwalk_dev(self.d_res, self.d_opt, self.place.t, n, max_id, *gt, g["cur_ts"], c.snd.t, self.ack.t,
                       self.astop.t, self.awork.t, stream=st)
        cx.ack_send_dev(self.place.t, n, max_id, *gt, self.rstop.t, self.astop.t, self.state.t, c.snd.t, g["cur_ts"],
                        ac.tx.t, ac.links, ac.image.t, 0, 6, 128, ac.seg.t, ac.desc.t, g["seg_cap"], ac.ares.t,
                        ac.total.t, ac.status.t, ac.work.t, stream=st)
        cx.data_send_dev(self.ack.t, self.astop.t, n, max_id, *gt, self.rstop.t, self.state.t, c.snd.t, ac.tx.t,
                         c.dtx.t, b["cur_ts"], c.payload, c.links, c.image.t, 0, 6, 0, c.seg.t, c.desc.t, b["seg_cap"],
                         c.dres.t, c.total.t, c.status.t, c.work.t, buf_len=b["buf_len"], stream=st)
        cx.rx_chunk_dev(c.image.t, c.desc.t, b["seg_cap"], 6, self.r2, stream=st)

    def reset_tail(self):
        dc, c, ac = self.dc, self.c, self.ac
        c.snd.t.copy_(to_dev(dc["chain"]["snd"]))
        ac.tx.t.copy_(to_dev(dc["g"]["tx"]))
        c.dtx.t.copy_(to_dev(dc["b"]["dtx"]))
        for x in (self.ack, self.astop, ac.seg, ac.desc, ac.ares, ac.total, ac.status, ac.image, c.seg, c.desc, c.dres,
                  c.total, c.status, c.image):
            x.t.fill_(SENT)
        for x in (self.awork, ac.work, c.work):
            x.t.fill_(0x3C)
        self.r2.zero_()

    def check(self, what):
        import oracle
        dc, c, b = self.dc, self.c, self.dc["b"]
        for x in (self.sid, *self.grp, self.gwork, self.rwork, self.awork, self.state, self.place, self.rstop, self.ack,
                  self.astop, self.ac.image, c.image):
            assert x.guard_intact(), what
        assert self.ack.numpy(ACK_REC_DTYPE).tobytes() == b["ack"].tobytes(), what
        assert self.state.numpy(b["state"].dtype).tobytes() == b["state"].tobytes(), what
        # the ACK sender's own outputs, but d_tx: the data call has advanced it since
        got_ack = (self.ac.seg.numpy(), self.ac.desc.numpy(), self.ac.total.numpy(np.uint64))
        for g_, e in zip(got_ack, (dc["want_ack"][0], dc["want_ack"][1], dc["want_ack"][3])):
            assert g_.tobytes() == e.tobytes(), what
        got = c.check(dc["want"], what)
        T = int(got[3][0])
        assert T + 37 == b["seg_cap"] and T > 100, T
        image, status = xm.build_frames(dc["want"][0], b["payload"], c.links.cpu().numpy().view(xm.LINK_DTYPE),
                                        dc["want"][1], np.full(b["buf_len"], SENT, np.uint8), off_shift=6)
        assert (status[:T] == xm.BUILT).all() and (status[T:] == xm.BAD_SEG).all()
        assert c.status.numpy().tobytes() == status.tobytes(), what
        assert c.image.numpy().tobytes() == image.tobytes(), what
        # the built frames parsed again: TCP_OK, and the records the oracle gives for the model's image
        ref = oracle.rx_chunk(image, dc["want"][1][:T].astype(oracle.DESC_DTYPE), 6, None)
        res = self.r2.cpu().numpy().view(RESULT_DTYPE)[:T]
        assert (ref["verdict"] == 0).all() and res.tobytes() == ref.tobytes(), what
        seg = dc["want"][0][:T]
        assert np.array_equal(res["seq"], seg["seq"]) and np.array_equal(res["ack_seq"], seg["ack"])
        assert np.array_equal(res["payload_len"], seg["payload_len"]) and (res["tcp_flags"] == 0x10).all()
        return got


def test_the_chain_reaches_the_send_side(data_chain):
    """What the batch asks of the data call, from the models alone: fast
    retransmissions that go out from the rewound snd_nxt, windows that an ACK
    opened, streams the fold put on the list and took off it."""
    b, dres = data_chain["b"], data_chain["want"][2]
    sid_of = {int(s): j for j, s in enumerate(b["seg_sid"])}
    status = np.bincount(dres["status"], minlength=12)
    assert status[dm.SENT] > 10 and status[dm.WINDOW] > 10 and status[dm.IDLE] > 10, status.tolist()
    rtx = np.unique(data_chain["chain"]["sid"][(b["ack"]["flags"] & dm.ACK_FAST_RTX) != 0])
    assert len(rtx) > 20
    sent = 0
    for s in rtx:
        r = dres[sid_of[int(s)]]
        if r["n_seg"] and int(r["status"]) >= dm.SENT:
            first = data_chain["want"][0][int(r["first_seg"])]
            assert int(first["seq"]) == int(b["snd"][int(s)]["snd_nxt"])            # tcp_in.c:406 set it back
            sent += 1
    assert sent > 10, sent
    added = [j for j in range(len(dres)) if dres[j]["flags"] & dm.ON_LIST_AFTER and not dres[j]["flags"] & dm.ON_LIST_BEFORE
             or (dres[j]["n_seg"] and not dres[j]["flags"] & dm.ON_LIST_BEFORE)]
    assert len(added) > 5, len(added)


def test_frames_in_data_frames_out(gpu, data_chain):
    ch = DataChain(gpu, data_chain)
    st = torch.cuda.Stream(device=DEV)
    with gpu.Context(0) as cx, gpu.FlowTable(cx, 12) as tab:
        tab.update_dev(None, 0, ch.d_ent, len(data_chain["ent"]), stream=st)
        ch.head(cx, tab, st)
        ch.tail(cx, st)
        st.synchronize()
    ch.check("behind the walks and the ACK sender")


def test_captured_tail_replayed_twice(gpu, data_chain):
    """ACK walk, ack_send_dev, data_send_dev and the parse of the built frames
    captured once on one stream (the data call's own launches are f8's
    multi-launch form here: 4 096 bursts) and replayed twice, each time from
    reset records and refilled outputs and workspaces."""
    ch = DataChain(gpu, data_chain)
    st = torch.cuda.Stream(device=DEV)
    with gpu.Context(0) as cx, gpu.FlowTable(cx, 12) as tab:
        tab.update_dev(None, 0, ch.d_ent, len(data_chain["ent"]), stream=st)
        ch.head(cx, tab, st)
        ch.tail(cx, st)                                                      # kernels loaded before the capture
        st.synchronize()
        ch.check("before the capture")
        ch.reset_tail()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            ch.tail(cx, st)
        for k in range(2):
            ch.reset_tail()
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            ch.check(f"replay {k}")
        del graph
