"""mtcp_gpu_tx_segment_plan (the C closed form, host only) against
tests/txseg_model.py (FlushTCPSendingBuffer's loop restated literally,
mtcp/src/tcp_out.c:357-449), and the model against itself.  No GPU needed."""
import numpy as np
import pytest

from tests import txseg_model as m

EDGE = m.edge_lists()


def plan(bursts, **kw):
    from mtcp_amd import gpu
    from mtcp_amd._types import TX_BURST_DTYPE
    return gpu.Context.tx_segment_plan(bursts.astype(TX_BURST_DTYPE), kw["payload_bytes"], kw["n_links"],
                                       kw["buf_off"], kw["buf_len"], kw["off_shift"], kw["slot_bytes"],
                                       kw["seg_cap"], kw.get("max_mss", 0))


def assert_plan_is_model(bursts, **kw):
    _, _, want, want_total = m.expand(bursts, **kw)
    got, got_total = plan(bursts, **kw)
    bad = np.flatnonzero(got.view(np.uint8).reshape(-1, 16) != want.view(np.uint8).reshape(-1, 16)) // 16
    assert len(bad) == 0, (f"burst {bad[0]}: {bursts[bad[0]]} plan {got[bad[0]]} model {want[bad[0]]}")
    assert got_total.tolist() == want_total.tolist()


def check_model(bursts, seg, desc, res, total, kw):
    """The model against itself."""
    k = int(total[0])
    # first_seg is the exclusive prefix sum of n_seg
    assert np.array_equal(res["first_seg"], np.cumsum(res["n_seg"]) - res["n_seg"])
    assert int(res["n_seg"].sum()) == k and (res["n_seg"][res["status"] != 0] == 0).all()
    assert (seg["form"][k:] == m.VOID_FORM).all() and not desc[k:].view(np.uint8).any()
    z = seg[k:].copy()
    z["form"] = 0
    assert not z.view(np.uint8).any()
    for b, r in zip(bursts, res):
        s = seg[int(r["first_seg"]):int(r["first_seg"]) + int(r["n_seg"])]
        # payload ranges tile [payload_off, payload_off + bytes)
        at = int(b["payload_off"])
        for j, x in enumerate(s):
            assert int(x["payload_off"]) == at and int(x["ip_id"]) == (int(b["ip_id"]) + j) & 0xFFFF
            assert int(x["seq"]) == (int(b["seq"]) + at - int(b["payload_off"])) & 0xFFFFFFFF
            at += int(x["payload_len"])
        assert at == int(b["payload_off"]) + int(r["bytes"]) and int(r["bytes"]) <= int(b["len"])
        if r["status"] == 0 and r["stop"] == 0:
            assert int(r["bytes"]) == int(b["len"])
    # slots never overlap, lie in [buf_off, buf_len) and are aligned
    A = m.align_of(kw["off_shift"])
    off = desc["offset"][:k].astype(object) * (1 << kw["off_shift"])
    end = off + desc["len"][:k].astype(object)
    assert all(o % A == 0 for o in off)
    assert (desc["len"][:k] == 66 + seg["payload_len"][:k].astype(np.int64)).all()
    if k:
        assert off[0] == kw["buf_off"] and end[-1] <= kw["buf_len"]
        assert all(e <= o for e, o in zip(end[:-1], off[1:]))
        assert kw["buf_off"] + int(total[1]) >= end[-1]


@pytest.mark.parametrize("name,bursts,kw", EDGE, ids=[e[0] for e in EDGE])
def test_plan_equals_model_on_edge_lists(name, bursts, kw):
    seg, desc, res, total = m.expand(bursts, **kw)
    check_model(bursts, seg, desc, res, total, kw)
    assert_plan_is_model(bursts, **kw)


def test_edge_lists_cover_what_they_claim():
    by = {name: m.expand(b, **kw)[2] for name, b, kw in EDGE}
    assert {0, 1, 3} <= set(by["windows"]["stop"].tolist())
    assert set(by["refusals"]["status"].tolist()) == {0, 1, 2}
    assert by["refusals"]["status"].tolist() == [0, 1, 0, 1, 1, 1, 0, 1, 1, 1, 0, 1, 0, 2, 2, 0, 0, 2]
    assert by["frame_above_slot"]["status"].tolist() == [1, 1, 0, 1]     # only the mss 536 burst fits 1 024 B slots
    assert by["frame_above_64k"]["status"].tolist() == [1, 0]
    for tag in ("shift0_packed", "shift1_fixed", "shift6_packed", "shift6_fixed"):
        assert by[f"room_none_{tag}"]["n_seg"].sum() == 18
        for kind in ("cap", "buf", "off"):
            assert by[f"room_{kind}_boundary_{tag}"]["n_seg"].tolist() == [3, 3, 0, 0, 0, 0, 0, 0], (kind, tag)
            assert by[f"room_{kind}_boundary_{tag}"]["stop"].tolist() == [0, 0, 0, 4, 3, 4, 4, 4], (kind, tag)
            assert by[f"room_{kind}_inside_{tag}"]["n_seg"].tolist() == [3, 3, 0, 1, 0, 0, 0, 0], (kind, tag)
    assert by["room_buf_off_past_32_bits"]["n_seg"].sum() == 0


@pytest.mark.parametrize("off_shift,slot_bytes,seg_cap,buf_len", [
    (6, 0, 1 << 18, 1 << 40), (0, 9216, 1 << 18, 1 << 40), (1, 0, 40000, 1 << 40), (6, 0, 1 << 18, 60 << 20)])
def test_plan_equals_model_on_random_bursts(off_shift, slot_bytes, seg_cap, buf_len):
    nbytes = 1 << 22
    bursts = m.random_bursts(20000, 5 + off_shift, nbytes)
    bursts["rsvd0"][::977] = 1
    bursts["link"][::1013] = 3
    bursts["payload_off"][::1031] = nbytes
    kw = dict(payload_bytes=nbytes, n_links=3, buf_off=64, buf_len=buf_len, off_shift=off_shift,
              slot_bytes=slot_bytes, seg_cap=seg_cap, max_mss=8960)
    seg, desc, res, total = m.expand(bursts, **kw)
    assert {0, 1, 2} <= set(res["status"].tolist()) and {0, 1, 3} <= set(res["stop"].tolist())
    if seg_cap == 40000 or buf_len == 60 << 20:
        assert 4 in res["stop"].tolist()
    assert_plan_is_model(bursts, **kw)
    few = bursts[:1500]
    check_model(few, *m.expand(few, **kw), kw)


def test_plan_saturates_without_wrapping():
    """Planned counts and slot bytes far past 32 and 64 bits' worth of room."""
    b = np.concatenate([m._burst(len=0xFFFFFFF0, mss=13, payload_off=0) for _ in range(40)] +
                       [m._burst(len=3000, payload_off=0)])
    kw = dict(payload_bytes=1 << 33, n_links=3, buf_off=0, buf_len=1 << 63, off_shift=16, slot_bytes=65536,
              seg_cap=300, max_mss=0)
    assert_plan_is_model(b, **kw)
    res, total = plan(b, **kw)
    assert total.tolist() == [300, 300 * 65536] and res["n_seg"].tolist() == [300] + [0] * 40
    assert res["first_seg"].tolist() == [0] + [300] * 40 and set(res["stop"].tolist()) == {4}


def test_plan_argument_errors():
    from mtcp_amd import _lib
    L = _lib.lib()
    b = m._burst(len=100)
    res = np.zeros(1, m.RESULT_DTYPE)
    total = np.zeros(2, np.uint64)
    good = dict(burst=b.ctypes.data, n_burst=1, payload_bytes=1000, n_links=2, buf_off=0, buf_len=1 << 20, off_shift=0,
                slot_bytes=0, seg_cap=8, max_mss=0, res=res.ctypes.data, total=total.ctypes.data)
    call = lambda **kw: L.mtcp_gpu_tx_segment_plan(*{**good, **kw}.values())
    assert call() == 0 and total.tolist() == [1, 166]
    for bad in (dict(burst=None), dict(res=None), dict(total=None), dict(off_shift=17), dict(n_links=0),
                dict(n_links=257), dict(seg_cap=0), dict(seg_cap=(1 << 26) + 1), dict(n_burst=(1 << 24) + 1),
                dict(buf_off=1), dict(slot_bytes=1535), dict(off_shift=6, slot_bytes=1504),
                dict(off_shift=6, buf_off=32)):
        before = (res.tobytes(), total.tobytes())
        assert call(**bad) == -22, bad
        assert (res.tobytes(), total.tobytes()) == before
    assert call(n_burst=0, burst=None, res=None) == 0 and total.tolist() == [0, 0]
    assert L.mtcp_gpu_tx_segment_work_bytes((1 << 24) + 1) == 0
    assert L.mtcp_gpu_tx_segment_work_bytes(0) >= 16 and L.mtcp_gpu_tx_segment_tile() >= 64


def test_dtypes_match_the_package():
    from mtcp_amd._types import TX_BURST_DTYPE, TX_BURST_RESULT_DTYPE
    assert TX_BURST_DTYPE == m.BURST_DTYPE and TX_BURST_RESULT_DTYPE == m.RESULT_DTYPE
