"""tests/rtosweep_model.py against the reference: tests/golden/rtosweep_cases.bin
holds, per case, 1-16 streams before and, per CheckRtmTimeout call, the streams
that fired and every stream's fields and stub counts after, from the
reference's own AddtoRTOList, CheckRtmTimeout and HandleRTO
(tests/c/ref_rtosweep_gen.c).  The wheel model must give every field and count;
the sweep model (the header's contract) must fire the same set per call and
leave the ESTABLISHED streams as the reference does; the cap is held to a plain
loop; the table goes through tests/datagen_model.py with ack None.  No GPU."""
import numpy as np

from mtcp_amd import _lib
from tests import datagen_model as dm
from tests import rtosweep_model as rm

CASES = rm.load_fixture()
FIELDS = ("snd_nxt", "snd_una", "peer_wnd", "cwnd", "ssthresh", "rto", "ts_rto", "srtt", "rttvar", "fss", "mss", "state",
          "nrtx", "max_nrtx", "on_rto", "has_sndbuf", "on_send_list", "has_socket", "close_reason")


def test_fixture_has_every_family():
    fam = np.bincount([c["family"] for c in CASES], minlength=len(rm.FAMILIES))
    assert len(fam) == len(rm.FAMILIES) and (fam > 0).all(), dict(zip(rm.FAMILIES, fam))
    B = [s for c in CASES for s in c["before"]]
    A = [(b, a) for c in CASES for _, recs in c["calls"] for b, a in zip(c["before"], recs) if a["fired"]]
    est = [(b, a) for b, a in A if b["state"] == rm.ST_ESTABLISHED]
    assert set(range(17)) <= {b["nrtx"] for b, _ in est}
    assert {0, 1} == {b["has_socket"] for b, a in est if b["nrtx"] >= 16}
    assert any(a["error_event"] for _, a in est) and any(a["destroy"] for _, a in est)
    assert any(a["rto"] == b["rto"] and ((b["srtt"] >> 3) + b["rttvar"]) & rm.M32 == 0 for b, a in est)
    assert any(b["rttvar"] == 0x02000000 and a["rto"] == b["rto"] for b, a in est)          # 0x02000000 << 7
    assert any(a["ssthresh"] == 2 * b["mss"] for b, a in est) and any(a["ssthresh"] > 2 * b["mss"] for b, a in est)
    assert any(b["cwnd"] > b["peer_wnd"] for b, _ in est) and any(b["cwnd"] < b["peer_wnd"] for b, _ in est)
    assert any(b["on_send_list"] and a["send_list"] for b, a in est)
    assert any(not b["has_sndbuf"] and a["send_list"] for b, a in est)
    assert any(a["control_list"] for _, a in A) and any(b["state"] != rm.ST_ESTABLISHED for b in B)
    assert any(len(c["calls"]) > 1 and sum(a["fired"] for a in recs) > 2 for c in CASES for _, recs in c["calls"])
    ts = [t for c in CASES for t, _ in c["calls"]]
    assert any(t > 0xFFFFFF00 for t in ts) and any(t < 0x100 for t in ts)
    for c in CASES:                                           # cur_ts - 1, cur_ts, cur_ts + 1 in family 0
        if c["family"] == 0:
            t = c["calls"][0][0]
            assert [(s["ts_rto"] - t) & rm.M32 for s in c["before"][:3]] == [rm.M32, 0, 1]


def run_wheel(c):
    """The case through the wheel model: per call (fired ids, records)."""
    streams = [dict(b, on_rto_idx=-1, id=i) for i, b in enumerate(c["before"])]
    w = rm.Wheel()
    for s in streams:
        if s.pop("on_rto"):
            rm.add_to_rto_list(w, s)
            assert 0 <= rm.s32(s["ts_rto"] - w.rto_now_ts) < rm.RTO_HASH
    out = []
    for cur_ts, _ in c["calls"]:
        calls = [dict.fromkeys(rm.CALLS, 0) for _ in streams]
        fired = rm.check_rtm_timeout(w, cur_ts, 1 << 20, lambda s: calls[s["id"]])
        out.append(([s["id"] for s in fired],
                    [dict({f: s[f] for f in FIELDS if f != "on_rto"}, on_rto=int(s["on_rto_idx"] >= 0), **calls[i])
                     for i, s in enumerate(streams)]))
    return out


def test_wheel_model_equals_the_reference():
    for i, c in enumerate(CASES):
        for k, ((fired, recs), (_, want)) in enumerate(zip(run_wheel(c), c["calls"])):
            assert sorted(fired) == [j for j, a in enumerate(want) if a["fired"]], (i, k)
            for j, (got, a) in enumerate(zip(recs, want)):
                a = {f: a[f] for f in FIELDS + rm.CALLS}
                assert got == a, (i, k, j, rm.FAMILIES[c["family"]], {f: (got[f], a[f]) for f in a if got[f] != a[f]})


def test_sweep_fires_the_wheels_set_and_steps_like_handle_rto():
    for i, c in enumerate(CASES):
        snd, dtx = rm.mirrors(c["before"])
        for k, (cur_ts, want) in enumerate(c["calls"]):
            before = snd.copy()
            snd, dtx, rec, seg_sid, seg_start, seg_stop, nseg, total = rm.sweep(snd, dtx, cur_ts, len(snd))
            assert set(seg_sid.tolist()) == {j for j, a in enumerate(want) if a["fired"]}, (i, k)
            assert list(seg_sid) == sorted(seg_sid) and nseg == len(rec) == total[0] == total[1]
            assert not seg_start.any() and not seg_stop.any() and len(seg_start) == len(seg_stop) + 1
            for r in rec:
                j, a, tag = int(r["sid"]), want[int(r["sid"])], (i, k, int(r["sid"]))
                if before[j]["tcp_state"] != rm.ST_ESTABLISHED:
                    assert r["verdict"] == rm.DEFER_STATE and snd[j] == before[j], tag
                    # the thread's own HandleRTO ran: it refreshes the mirror
                    for f in ("snd_nxt", "cwnd", "ssthresh", "rto", "nrtx", "on_rto"):
                        snd[j][f] = a[f]
                    snd[j]["tcp_state"] = a["state"]
                    continue
                got = {f: int(snd[j][f]) for f in ("snd_nxt", "snd_una", "peer_wnd", "cwnd", "ssthresh", "rto", "ts_rto",
                                                   "srtt", "rttvar", "mss", "nrtx", "on_rto", "has_sndbuf")}
                assert got == {f: a[f] for f in got} and snd[j]["tcp_state"] == a["state"], tag
                assert (r["rto"], r["nrtx"]) == (a["rto"], a["nrtx"]), tag
                if r["verdict"] == rm.LOST:
                    assert a["close_reason"] == rm.CONN_LOST and a["error_event"] + a["destroy"] == 1, tag
                    assert a["send_list"] == 0 and dtx[j]["on_send_list"] == c["before"][j]["on_send_list"], tag
                else:
                    assert r["verdict"] == rm.RETRANSMIT and a["send_list"] == 1 and a["close_reason"] == 0, tag
                    assert max(c["before"][j]["max_nrtx"], int(r["nrtx"])) == a["max_nrtx"], tag
                    b = c["before"][j]
                    assert dtx[j]["on_send_list"] == (1 if b["has_sndbuf"] else b["on_send_list"]), tag
                    assert bool(r["flags"] & rm.SEND_LIST_ADD) == bool(b["has_sndbuf"] and not b["on_send_list"]), tag
            keep = np.setdiff1d(np.arange(len(snd)), seg_sid)
            assert (snd[keep] == before[keep]).all(), (i, k)


def plain_sweep(snd, dtx, cur_ts, cap):
    """The contract as a loop over ids, one stream at a time."""
    snd, dtx, handled, due = snd.copy(), dtx.copy(), [], 0
    for i in range(len(snd)):
        s = snd[i]
        if s["on_rto"] != 1 or rm.s32(cur_ts - int(s["ts_rto"])) < 0:
            continue
        due += 1
        if len(handled) == cap:
            continue
        one = rm.sweep(snd[i:i + 1], dtx[i:i + 1], cur_ts, 1)
        snd[i], dtx[i] = one[0][0], one[1][0]
        r = one[2][0].copy()
        r["sid"] = i
        handled.append(r)
    return snd, dtx, handled, due


def test_the_cap_takes_the_first_in_id_order():
    rng = np.random.default_rng(11)
    recs = [b for c in CASES for b in c["before"]]
    for trial in range(40):
        pick = [recs[int(k)] for k in rng.integers(0, len(recs), 70)]
        snd, dtx = rm.mirrors(pick)
        cur_ts = int(rng.integers(0, 1 << 32))
        snd["ts_rto"] = (cur_ts + rng.integers(-3, 2, len(snd))) & rm.M32
        if trial % 4 == 0:                                    # random bytes: BAD records, every state, any nrtx
            raw = rng.integers(0, 256, (len(snd), 128), dtype=np.uint8)
            raw[:, 85] = rng.integers(0, 3, len(snd))
            snd = raw.view(rm.ACK_STATE_DTYPE).reshape(-1).copy()
            snd["ts_rto"] = (cur_ts + rng.integers(-3, 2, len(snd))) & rm.M32
            dtx = rng.integers(0, 256, (len(snd), 16), dtype=np.uint8).view(rm.DATAGEN_STATE_DTYPE).reshape(-1).copy()
            dtx["rsvd"][rng.random(len(snd)) < 0.8] = 0
            dtx["on_send_list"] &= 1
            dtx["on_control_list"] &= 1
        due = len(rm.due_ids(snd, cur_ts))
        assert due > 3
        for cap in (1, due - 1, due, due + 1):
            s1, d1, rec, seg_sid, _, _, nseg, total = rm.sweep(snd, dtx, cur_ts, cap)
            s2, d2, handled, due2 = plain_sweep(snd, dtx, cur_ts, cap)
            assert s1.tobytes() == s2.tobytes() and d1.tobytes() == d2.tobytes(), (trial, cap)
            assert rec.tobytes() == b"".join(r.tobytes() for r in handled) and list(total) == [due2, len(handled)]
            assert nseg == min(due, cap) and list(seg_sid) == list(rm.due_ids(snd, cur_ts)[:cap])
            rest = rm.due_ids(snd, cur_ts)[cap:]
            assert (s1[rest] == snd[rest]).all() and (d1[rest] == dtx[rest]).all()
            # a second sweep takes exactly the rest (a DEFER_STATE or BAD stream stays due: the host's)
            again = rm.sweep(s1, d1, cur_ts, len(snd))
            stay = [int(r["sid"]) for r in rec if r["verdict"] in (rm.BAD, rm.DEFER_STATE)]
            assert sorted(again[3].tolist()) == sorted(rest.tolist() + stay), (trial, cap)


def test_the_table_through_the_data_generation():
    """Behind the sweep every RETRANSMIT stream that is on the send list flushes
    from snd_una under MIN(mss, peer_wnd): whole packets, as tcp_out.c:401-443
    sends them (rm.flush_bytes), and is armed again with RTO_ADD if a segment
    went out.  Every other verdict changes nothing."""
    seen = set()
    for i, c in enumerate(CASES):
        snd, dtx = rm.mirrors(c["before"])
        n = len(snd)
        state, tx, payload = rm.send_side(n, i)
        cur_ts = c["calls"][-1][0]
        cap = n + (i % 3)
        sw, dg = rm.send(snd, dtx, cur_ts, cap, state, tx, len(payload), 8 * n)
        snd1, dtx1, rec, seg_sid, _, _, nseg, _ = sw
        seg, desc, dres, total, snd2, tx2, dtx2, _ = dg
        assert len(dres) == nseg
        for j, (r, dr) in enumerate(zip(rec, dres)):
            sid = int(r["sid"])
            b, s1 = snd[sid], snd1[sid]
            if r["verdict"] != rm.RETRANSMIT:
                assert dr["status"] == (dm.BAD if r["verdict"] == rm.BAD else dm.DEFERRED) and not dr["n_seg"]
                assert snd2[sid] == s1 and dtx2[sid] == dtx1[sid] and tx2[sid] == tx[sid], (i, sid)
                seen.add(int(r["verdict"]))
                continue
            if not b["has_sndbuf"]:
                assert dr["status"] in (dm.IDLE, dm.NO_SNDBUF) and not dr["n_seg"] and snd2[sid] == s1, (i, sid)
                seen.add("nobuf")
                continue
            if b["mss"] < 13 or b["mss"] - 12 > 1460 + 12:    # row f8 takes no such mss (mtcp_gpu_txseg.h)
                assert dr["status"] == dm.BAD_BURST and not dr["n_seg"] and snd2[sid] == s1, (i, sid)
                seen.add("bad burst")
                continue
            segs, nbytes = rm.flush_bytes(int(b["mss"]), int(b["peer_wnd"]), int(b["sb_len"]))
            assert (int(dr["n_seg"]), int(dr["bytes"])) == (segs, nbytes), (i, sid, dr, b)
            assert snd2[sid]["snd_nxt"] == (int(b["snd_una"]) + nbytes) & rm.M32, (i, sid)
            if segs:
                first = seg[int(dr["first_seg"])]
                assert first["seq"] == b["snd_una"] and dr["flags"] & dm.RTO_ADD, (i, sid)
                assert snd2[sid]["on_rto"] == 1 and snd2[sid]["ts_rto"] == (cur_ts + int(s1["rto"])) & rm.M32
                seen.add("sent")
            else:
                assert not dr["flags"] & dm.RTO_ADD and snd2[sid]["on_rto"] == 0
                seen.add("stopped")
        rest = np.setdiff1d(np.arange(n), seg_sid)
        assert (snd2[rest] == snd[rest]).all() and (dtx2[rest] == dtx[rest]).all() and (tx2[rest] == tx[rest]).all()
    assert {"sent", "nobuf", rm.LOST, rm.DEFER_STATE} <= seen, seen


def test_the_header_declares_what_the_library_exports():
    import os
    import re
    src = open(os.path.join(os.path.dirname(rm.__file__), "..", "include", "mtcp_gpu_rtosweep.h")).read()
    assert "#define MTCP_GPU_HAS_RTOSWEEP" in src
    decl = set(re.findall(r"\b(mtcp_gpu_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))
    assert decl == {"mtcp_gpu_rto_sweep_work_bytes", "mtcp_gpu_rto_sweep_tile", "mtcp_gpu_rto_sweep_dev",
                    "mtcp_gpu_rto_sweep", "mtcp_gpu_rto_send_dev"} and decl <= set(_lib.EXPORTS)
    L = _lib.lib()
    assert all(hasattr(L, f) for f in decl) and L.mtcp_gpu_abi_version() == 5
    wb = L.mtcp_gpu_rto_sweep_work_bytes
    assert wb(0, 0) == 0 and wb(0, (1 << 24) + 1) == 0 and wb(0xFFFFFFF0, 1) == 0
    prev = 0
    for max_id in (0, 1, 4095, 4096, 65535, (1 << 20) - 1, 1 << 24, 0xFFFFFFEF):
        got = [wb(max_id, cap) for cap in (1, 4096, 4097, 1 << 24)]
        assert got[0] > 0 and got == sorted(got) and got[0] >= prev
        prev = got[-1]
