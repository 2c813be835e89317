"""tests/ackgen_model.py against the reference: tests/golden/ackgen_cases.bin
holds, per case, a stream before, a sequence of EnqueueACK options, cur_ts, a
slot budget, the frames the reference's own EnqueueACK, WriteTCPACKList,
SendTCPPacket, IPOutput and EthernetOutput wrote, and the stream after
(tests/c/ref_ackgen_gen.c).  The per-case form of the model must give the same
stream and, through tests/txbuild_model.py, the same frames byte for byte; the
grouped-batch form is held to the per-case form; mtcp_gpu_ackgen_work_bytes'
rules.  No GPU."""
import numpy as np
import pytest

from tests import ackgen_gen as gg
from tests import ackgen_model as am
from tests import txbuild_model as xm

CASES = am.load_fixture()
LINKS = am.fixture_links()


def test_fixture_has_every_family():
    fam = np.bincount([c["family"] for c in CASES], minlength=len(am.FAMILIES))
    assert len(fam) == len(am.FAMILIES) and (fam > 0).all(), dict(zip(am.FAMILIES, fam))
    nows = sorted(len(c["opts"]) for c in CASES if c["family"] == 1)
    assert nows == list(range(1, 71))                                 # 63, 64 and 65 are in it
    wack = [c for c in CASES if c["family"] == 3]
    assert any(c["before"]["is_wack"] and len(c["frames"]) == 1 for c in wack)       # the probe alone
    assert any(c["before"]["is_wack"] and len(c["frames"]) > 1 for c in wack)
    assert all(len(c["frames"]) == 0 and not c["after"]["on_ack_list"] and c["after"]["ack_cnt"] == 0
               for c in CASES if c["family"] in (4, 5) and not am.seq_leq(c["before"]["rcv_nxt"], (c["before"]["head_seq"] + c["before"]["merged_len"]) & am.M32) or c["family"] == 4)
    cuts = [c for c in CASES if c["family"] == 6]
    k = lambda c: len(c["opts"])
    assert any(c["budget"] == 0 for c in cuts) and any(c["before"]["is_wack"] and c["budget"] == k(c) for c in cuts)
    assert any(0 < c["budget"] < k(c) for c in cuts)
    w32 = {(c["before"]["rcv_wnd"] >> c["before"]["wscale_mine"]) for c in CASES if c["family"] == 7}
    assert {0, 1, 65535, 65536} <= w32 and max(w32) > 65536
    assert {c["before"]["wscale_mine"] for c in CASES if c["family"] == 7} == set(range(15))
    assert all(((c["before"]["ip_id"] - 65532) & 0xFFFF) <= 6 for c in CASES if c["family"] == 8)    # 65532 .. 2
    assert any(c["after"]["ip_id"] < c["before"]["ip_id"] for c in CASES if c["family"] == 8)


def test_model_equals_the_reference():
    for i, c in enumerate(CASES):
        recs, after = am.run_case(c["before"], c["opts"], c["cur_ts"], c["budget"])
        assert after == c["after"], (i, am.FAMILIES[c["family"]], after, c["after"])
        assert len(recs) == len(c["frames"]), (i, len(recs), len(c["frames"]))
        for k, (r, f) in enumerate(zip(recs, c["frames"])):
            assert r["payload_len"] == 0 and r["flags"] == 0x10 and r["form"] == 1
            got = xm.build_frame(r, np.zeros(0, np.uint8), LINKS[int(r["link"])])
            assert got.tobytes() == f.tobytes(), (i, k, am.FAMILIES[c["family"]], got, f)


def per_stream(b):
    """The batch's answer from the per-case form, stream by stream in the
    table's order: the expected (records, tx after, statuses)."""
    idx, seg_sid, seg_start = b["group"]
    slot = am.slot_of(b["off_shift"], b["slot_bytes"])
    E = am.room_of(b["buf_off"], b["buf_len"], b["off_shift"], slot, b["seg_cap"])
    tx, recs, status = b["tx"].copy(), [], []
    planned_before = 0
    for j, sid in enumerate(seg_sid):
        sid = int(sid)
        if sid > b["max_id"]:
            status.append(am.NONE)
            continue
        t = tx[sid]
        if am.is_bad(t, b["n_links"]):
            status.append(am.BAD)
            continue
        start, end = int(seg_start[j]), int(seg_start[j + 1])
        stop = min(max(int(b["seg_stop"][j]), start), end)
        deferred = int(b["seg_stop"][j]) < end or (b["ack_stop"] is not None and int(b["ack_stop"][j]) < end) or \
            b["state"][sid]["tcp_state"] != 4
        opts, put = [], False
        for p in idx[start:stop]:
            if p >= b["n"]:
                continue
            fl = int(b["place"][p]["flags"])
            opts += [am.ACK_OPT_NOW] * bool(fl & 2) + [am.ACK_OPT_AGGREGATE] * bool(fl & 4)
            put |= int(b["place"][p]["verdict"]) in am.PUT_VERDICTS
        s = {f: int(t[f]) for f in am.STATE_DTYPE.names if f != "rsvd"}
        s["on_ack_list"] = 1 if (s["ack_cnt"] or s["is_wack"]) else 0
        s["snd_nxt"] = int(b["snd"][sid]["snd_nxt"])
        s.update({f: int(b["state"][sid][f]) for f in ("rcv_nxt", "rcv_wnd", "head_seq", "merged_len", "ts_recent")})
        s["has_rcvbuf"] |= int(put)
        if deferred:
            for o in opts:
                am.enqueue_ack(s, o)
            out = []
            status.append(am.DEFERRED)
        else:
            full, _ = am.run_case(s, opts, b["cur_ts"], 1 << 30)
            out, s = am.run_case(s, opts, b["cur_ts"], max(E - planned_before, 0))
            planned_before = min(planned_before + len(full), b["seg_cap"])
            status.append(None)
        for f in ("ip_id", "ack_cnt", "is_wack", "has_rcvbuf", "need_wnd_adv", "ts_lastack_sent"):
            tx[sid][f] = s[f]
        recs += out
    return recs, tx, status


@pytest.mark.parametrize("seed", range(6))
def test_grouped_form_equals_per_stream_application(seed):
    rng = np.random.default_rng(100 + seed)
    streams = []
    for i in range(int(rng.integers(3, 14))):
        k = int(rng.integers(1, 90))
        s = dict(len=k, flags="mixed", tx=dict(ack_cnt=int(rng.integers(0, 64)) if rng.random() < .3 else 0,
                                               is_wack=int(rng.random() < .3), has_rcvbuf=int(rng.random() < .8)))
        if k > 2 and rng.random() < .25:
            s["defer"] = (("seg", "ack")[int(rng.integers(2))], int(rng.integers(0, k - 1)))
        if rng.random() < .1:
            s["tx"]["wscale_mine"] = 40
        streams.append(s)
    room = [dict(), dict(seg_cap=int(rng.integers(1, 60))), dict(buf_off=128, buf_len=128 + 128 * int(rng.integers(0, 40)), slot_bytes=128, off_shift=6)][seed % 3]
    b = gg.make(streams, seed=200 + seed, n_miss=2, n_none=1, with_ack_stop=bool(seed & 1), **room)
    seg, desc, ares, total, tx = gg.expect(b)
    recs, w_tx, status = per_stream(b)
    assert int(total[0]) == len(recs)
    assert seg[:len(recs)].tobytes() == b"".join(r.tobytes() for r in recs)
    assert (seg[len(recs):]["form"] == am.VOID_FORM).all() and not desc[len(recs):].view(np.uint8).any()
    assert tx.tobytes() == w_tx.tobytes()
    for j, st in enumerate(status):
        if st is not None:
            assert ares[j]["status"] == st, (j, ares[j], st)
    assert (np.diff(ares["first_seg"].astype(np.int64)) >= 0).all()
    assert int(ares["n_ack"].sum()) + int(ares["wack"].sum()) == len(recs)


def test_work_bytes_rules():
    from mtcp_amd import gpu
    wb = gpu.Context.ackgen_work_bytes
    assert wb(0, 0) > 0 and wb(1, 0) > 0
    assert wb((1 << 26) + 1, 0) == 0 and wb(1, 0xFFFFFFF0) == 0 and wb(1 << 26, 0xFFFFFFEF) > 0
    last = 0
    for n in (0, 1, 2, 255, 256, 257, 4096, 65536, 1 << 20, 1 << 26):
        for max_id in (0, 1, 1000, 0xFFFFFFEF):
            assert wb(n, max_id) >= last and wb(n, max_id) >= wb(n, 0)
        last = wb(n, 0)
    assert gpu.Context.ackgen_lane_len() >= 1
