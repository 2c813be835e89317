"""The ProcessACK walk on the CPU (include/mtcp_gpu_ackwalk.h): tests/ackwalk_model.py
against a fixture the reference's own code wrote
(tests/golden/ackwalk_cases.bin, written by tests/make_ackwalk_golden.py; this
test reads only the fixture), the fixture's coverage, the statistics of the
family the GPU tests share, a built case for every DEFER reason and every BAD
rule, the header's layouts and citations, the workspace size, and the kernels'
own step function compiled for the host (tools/ackwalk_pattern.hip) against the
model."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

from mtcp_amd import _types as T
from mtcp_amd._types import ACK_REC_DTYPE, ACK_STATE_DTYPE, RCV_PLACE_DTYPE, RESULT_DTYPE, TCPOPT_DTYPE, TCPOPT_TS_FOUND
from tests import ackwalk_gen as ag
from tests import ackwalk_model as am
from tests import group_model as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACK = 0x10
FLAG_BITS = [getattr(T, "ACK_" + f) for f in T.ACK_FLAGS]
RCV_ACK_ONLY, RCV_SEQ_OLD = 12, 10


# ---- the fixture ---------------------------------------------------------------------------------
def read_golden():
    """[(initial 88 B record, family, [(inputs, outputs)])] of tests/golden/ackwalk_cases.bin
    (tests/c/ref_ackwalk_gen.c has the layout)."""
    raw = open(os.path.join(ROOT, "tests", "golden", "ackwalk_cases.bin"), "rb").read()
    magic, version, walks, per = struct.unpack_from("<4I", raw, 0)
    assert magic == 0x574B4341 and version == 1 and per == 16
    off, out = 16, []
    for _ in range(walks):
        first = np.frombuffer(raw[off:off + 88] + bytes(40), ACK_STATE_DTYPE)[0]
        fam, npkt = struct.unpack_from("<2I", raw, off + 88)
        off += 96
        pk = []
        for _ in range(npkt):
            seq, ack_seq, ts_ref, cur_ts, window, ln, has_ack, has_ts, ret, z0 = struct.unpack_from("<4I2H2BbB", raw, off)
            counts = struct.unpack_from("<6BH", raw, off + 24)
            removed, = struct.unpack_from("<I", raw, off + 32)
            words = struct.unpack_from("<18I", raw, off + 36)
            dup_acks, nrtx, on_rto, z1 = struct.unpack_from("<4B", raw, off + 108)
            off += 112
            assert z0 == 0 and z1 == 0 and counts[6] == 0
            pk.append(((seq, ack_seq, ts_ref, cur_ts, window, ln, has_ack, has_ts, ret),
                       (counts[:6], removed, words + (dup_acks, nrtx, on_rto))))
        out.append((first, fam, pk))
    assert off == len(raw) and len(raw) <= 1 << 20
    return out


@pytest.fixture(scope="module")
def golden():
    return read_golden()


def model_packet(inp):
    seq, ack_seq, ts_ref, cur_ts, window, ln, has_ack, has_ts, ret = inp
    return (seq, ack_seq, ts_ref, window, ln, ACK if has_ack else 0, RCV_ACK_ONLY if ret else RCV_SEQ_OLD, bool(has_ts))


def counts_of(r):
    """What the reference's calls would count for a record tuple: RaiseWriteEvent at tcp_in.c:362 and :521,
    AddtoSendList, RemoveFromSendList, RemoveFromRTOList, AddtoRTOList."""
    f = r[3]
    return tuple(int(bool(f & b)) for b in (T.ACK_WRITE_EVENT_WND, T.ACK_WRITE_EVENT_ROOM, T.ACK_FAST_RTX,
                                            T.ACK_SEND_LIST_REMOVE, T.ACK_RTO_REMOVE, T.ACK_RTO_ADD))


@pytest.fixture(scope="module")
def golden_run(golden):
    """The model walked over the fixture, compared after every packet; returns the verdict and flag counts."""
    verdicts, flags = np.zeros(16, np.int64), np.zeros(len(FLAG_BITS), np.int64)
    for w, (first, fam, pk) in enumerate(golden):
        st = am.Snd.from_record(first)
        for i, (inp, (counts, removed, words)) in enumerate(pk):
            r = am.step(st, model_packet(inp), inp[3])
            what = f"walk {w} (family {fam}) packet {i}: {am.ACK_VERDICTS[r[4]]} flags {r[3]:#x}"
            assert r[4] in am.WALKED, what                   # the generator stays inside what is restated
            assert st.words() == words, what
            assert counts_of(r) == counts and r[0] == removed, what
            assert (r[1], r[2], r[5]) == (st.snd_nxt, st.cwnd, st.dup_acks), what
            assert (r[4] == am.NOT_VALID) == (not inp[8]), what
            verdicts[r[4]] += 1
            flags += [bool(r[3] & b) for b in FLAG_BITS]
    return verdicts, flags


def test_model_matches_the_references_own_walks(golden, golden_run):
    """After every packet: every state word, every count (golden_run asserts them)."""
    assert 500 <= len(golden) <= 1100 and all(len(pk) == 16 for _, _, pk in golden)


def test_fixture_reaches_every_walked_verdict_and_every_flag(golden, golden_run):
    verdicts, flags = golden_run
    for v in am.WALKED:
        assert verdicts[v] >= 20, (am.ACK_VERDICTS[v], int(verdicts[v]))
    for name, c in zip(T.ACK_FLAGS, flags):
        assert c >= 20, (name, int(c))


def test_fixture_holds_every_kind_of_walk(golden):
    firsts = np.array([f for f, _, _ in golden])
    assert 0.3 < (firsts["saw_timestamp"] != 0).mean() < 0.7
    assert (firsts["srtt"] == 0).sum() > 50 and (firsts["srtt"] != 0).sum() > 50
    assert (firsts["on_rto"] == 0).sum() > 50 and (firsts["on_rto"] == 1).sum() > 50
    assert (firsts["snd_wnd"] == 0).sum() > 50                       # a full send buffer
    assert (firsts["has_sndbuf"] == 0).sum() >= 20
    assert (firsts["sb_head_seq"] > 0xFFFFFFFF - 20001).sum() > 50   # the walk wraps
    assert (firsts["cwnd"] < firsts["ssthresh"]).sum() > 50 and (firsts["cwnd"] >= firsts["ssthresh"]).sum() > 50
    runs, up, down, passed, not_passed, all_acked, some_left, crossed = set(), 0, 0, 0, 0, 0, 0, 0
    for first, fam, pk in golden:
        st = am.Snd.from_record(first)
        run = 0
        for inp, _ in pk:
            before = st.copy()
            r = am.step(st, model_packet(inp), inp[3])
            if r[3] & T.ACK_DUP:
                run += 1
            else:
                runs.add(run)
                run = 0
            if r[4] == am.ACK_NEW:
                if st.saw_timestamp and before.srtt:
                    sample = max(1, (inp[3] - inp[2]) & am.M32)
                    up, down = up + (sample > before.srtt >> 3), down + (sample < before.srtt >> 3)
                    hit = am.TCP_SEQ_GT(before.snd_una, before.rtt_seq)
                    passed, not_passed = passed + hit, not_passed + (not hit)
                all_acked, some_left = all_acked + (st.sb_len == 0), some_left + (st.sb_len != 0)
                crossed += before.cwnd < before.ssthresh <= st.cwnd
        runs.add(run)
    assert {1, 2, 3, 4, 5, 6} <= runs, sorted(runs)                  # duplicate-ACK runs of 1 to 6
    assert min(up, down, passed, not_passed, all_acked, some_left) >= 20, (up, down, passed, not_passed, all_acked, some_left)
    assert crossed >= 20                                             # slow start into congestion avoidance


# ---- every DEFER reason and every BAD rule, built ----------------------------------------------------
def plain():
    return am.Snd(snd_nxt=5000, snd_una=1000, sb_head_seq=1000, sb_len=6000, sb_size=8192, snd_wnd=2192, peer_wnd=30000,
                  snd_wl1=7, snd_wl2=1000, last_ack_seq=1000, cwnd=2920, ssthresh=1 << 20, rto=20, saw_timestamp=1)


def test_known_answer():
    st = plain()
    pkt = lambda ack, ln=0: (7, ack, 90, 30000, ln, ACK, RCV_ACK_ONLY, True)
    got = [am.step(st, pkt(a), 100) for a in (2448, 2448, 2448, 2448, 3896)]
    assert got[0] == (1448, 5000, 2920 + 1460, T.ACK_WND_UPDATE | T.ACK_RTO_ADD, am.ACK_NEW, 0)
    # the first sample: srtt = 10 << 3, mdev = rttvar = 20, rto = 30, ts_rto = 100 + 30; the second leaves mdev 15
    assert (st.srtt, st.mdev, st.rttvar, st.rto, st.ts_rto) == (80, 15, 20, 30, 130)
    assert got[1][3:] == (T.ACK_DUP, am.ACK_OLD, 1) and got[2][3:] == (T.ACK_DUP, am.ACK_OLD, 2)
    assert got[3] == (0, 2448, 2920 + 3 * 1460, T.ACK_DUP | T.ACK_FAST_RTX, am.ACK_OLD, 3)      # ssthresh = 2 * mss
    assert got[4][0] == 1448 and got[4][3] == T.ACK_WND_UPDATE | T.ACK_SND_NXT_RECOVERED | T.ACK_RTO_REMOVE
    assert (st.snd_nxt, st.snd_una, st.sb_head_seq, st.sb_len, st.nrtx, st.on_rto) == (3896, 3896, 3896, 3104, 0, 0)


def test_every_defer_reason_and_every_bad_rule():
    ok = (7, 2448, 90, 30000, 0, ACK, RCV_ACK_ONLY, True)
    cases = []
    for field, value in (("rsvd", 1), ("eff_mss", 0), ("wscale_peer", 32), ("sb_size", (1 << 30) + 1), ("sb_len", 8193)):
        st = plain()
        setattr(st, field, value)
        cases.append((st, ok, am.DEFER_BAD_STATE, field))
    st = plain()
    st.tcp_state = 7
    cases.append((st, ok, am.DEFER_STATE, "state"))
    for flag in (0x01, 0x02, 0x04):
        cases.append((plain(), ok[:5] + (ACK | flag,) + ok[6:], am.DEFER_FLAGS, f"flag {flag}"))
    for rv in (0, 1, 2, 3, 4, 5, 6, 16, 255):
        cases.append((plain(), ok[:6] + (rv, True), am.DEFER_RCV, f"placement verdict {rv}"))
    cases.append((plain(), ok[:7] + (False,), am.DEFER_RCV, "no timestamp record on a saw_timestamp stream"))
    st = plain()                                          # mss * packets at tcp_in.c:490: 65535 * 40000
    st.mss, st.eff_mss, st.sb_size, st.sb_len, st.snd_nxt = 65535, 1, 1 << 20, 1 << 20, 1000 + (1 << 20)
    cases.append((st, ok[:1] + (1000 + 40000,) + ok[2:], am.DEFER_ARITH, "mss * packets"))
    st = plain()                                          # packets * mss * mss at :495-497: 1 * 65535 * 65535
    st.mss, st.ssthresh = 65535, 0
    cases.append((st, ok, am.DEFER_ARITH, "packets * mss * mss"))
    st = plain()                                          # / cwnd at :495-497
    st.cwnd = st.ssthresh = 0
    cases.append((st, ok, am.DEFER_ARITH, "cwnd == 0"))
    for st, p, want, what in cases:
        before = ag.record_of(st).tobytes()
        assert am.step(st, p, 100) == am.rec(verdict=want), what
        assert ag.record_of(st).tobytes() == before, what
    with pytest.raises(am.Arith):
        am.step(cases[-1][0], ok, 100, deferral=False)
    # their neighbours are walked: a slow-start step whose guard at tcp_in.c:489 fails multiplies nothing
    st = plain()
    st.mss, st.eff_mss, st.sb_size, st.sb_len, st.snd_nxt, st.cwnd, st.ssthresh = 65535, 1, 1 << 20, 1 << 20, 1000 + (1 << 20), \
        am.M32 - 5, am.M32
    assert am.step(st, ok[:1] + (1000 + 40000,) + ok[2:], 100)[4] == am.ACK_NEW and st.cwnd == am.M32 - 5
    st = plain()
    st.wscale_peer, st.sb_size, st.sb_len = 31, 1 << 30, 1 << 30
    assert am.step(st, ok, 100)[4] == am.ACK_NEW
    for rv in range(7, 12):
        assert am.step(plain(), ok[:6] + (rv, True), 100) == (0, 5000, 2920, 0, am.NOT_VALID, 0)


def test_a_batch_defers_behind_and_keeps_the_state():
    res, opt = np.zeros(6, RESULT_DTYPE), np.zeros(6, TCPOPT_DTYPE)
    res["seq"], res["ack_seq"], res["window"] = 7, [2000, 3000, 4000, 5000, 9, 6000], 30000
    res["tcp_flags"] = [ACK, ACK, ACK | 0x01, ACK, ACK, ACK]
    opt["flags"], opt["ts_ref"] = TCPOPT_TS_FOUND, 90
    place = np.zeros(6, RCV_PLACE_DTYPE)
    place["verdict"] = [12, 12, 3, 6, 0, 6]
    sid = np.array([3, 3, 3, 3, am.FLOW_MISS, 3], np.uint32)
    snd = np.zeros(6, ACK_STATE_DTYPE)
    snd[3], snd[5] = ag.record_of(plain()), ag.record_of(plain())
    snd["user"] = 0x5A
    idx, seg_sid, seg_start = gm.group(sid, 5)
    ack, new, stop = am.walk(res, opt, place, 5, idx, seg_sid, seg_start, 100, snd)
    assert ack["verdict"].tolist() == [am.ACK_NEW, am.ACK_NEW, am.DEFER_FLAGS, am.DEFER_BEHIND, am.NONE, am.DEFER_BEHIND]
    assert stop.tolist() == [2, 5] and ack["rmlen"].tolist() == [1000, 1000, 0, 0, 0, 0]
    assert new[3]["snd_una"] == 3000 and new[3]["sb_len"] == 4000 and (new["user"] == 0x5A).all()
    assert new[5].tobytes() == snd[5].tobytes() and ack[4].tobytes() == bytes(16)
    assert ack[3].tobytes() == bytes(14) + bytes([am.DEFER_BEHIND, 0])


# ---- the header ------------------------------------------------------------------------------------
def test_header_layouts_offsets_and_citations():
    hdr = open(os.path.join(ROOT, "include", "mtcp_gpu_ackwalk.h")).read()
    assert re.search(r"#define MTCP_GPU_HAS_ACKWALK\s+1\b", hdr)
    assert "MTCP_GPU_ABI_VERSION" in hdr and "extern \"C\"" in hdr
    for name, dt in (("mtcp_gpu_ack_state", ACK_STATE_DTYPE), ("mtcp_gpu_ack_rec", ACK_REC_DTYPE)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
        fields = re.findall(r"(\w+)(?:\[\w+\])?;\s*/\*\s*(\d+) ", body)
        assert [(f, int(o)) for f, o in fields] == [(f, dt.fields[f][1]) for f in dt.names], name
    assert ACK_STATE_DTYPE.itemsize == 128 and ACK_REC_DTYPE.itemsize == 16
    for k, v in enumerate(am.ACK_VERDICTS):
        assert re.search(r"MTCP_GPU_ACK_%s\s*=\s*%d\b" % (v, k), hdr), v
    for name, bit in zip(T.ACK_FLAGS, FLAG_BITS):
        assert re.search(r"#define MTCP_GPU_ACK_%s\s+0x%04xu" % (name, bit), hdr), name
    pieces = [hdr[:hdr.index("#ifndef")]]
    for fn in ("mtcp_gpu_ackwalk_work_bytes", "mtcp_gpu_ackwalk_short_len", "mtcp_gpu_ackwalk_dev", "mtcp_gpu_ackwalk"):
        at = re.search(r"\b%s\(" % fn, re.sub(r"/\*.*?\*/", lambda m: " " * len(m.group(0)), hdr, flags=re.S)).start()
        pieces.append(hdr[hdr.rindex("/*", 0, at):at])
    for text in pieces:
        assert "tcp_in.c:302-531" in " ".join(text.replace("*", " ").split()), text[:60]


def test_every_citation_resolves_in_the_reference():
    """file:line and file:line-line in the header name lines the reference has, where it is present."""
    ref = os.environ.get("REF", "/root/reference")
    if not os.path.isdir(os.path.join(ref, "mtcp", "src")):
        pytest.skip("the reference's sources are not present")
    hdr = open(os.path.join(ROOT, "include", "mtcp_gpu_ackwalk.h")).read()
    where = {"tcp_in.c": "mtcp/src/tcp_in.c", "tcp_in.h": "mtcp/src/include/tcp_in.h", "timer.c": "mtcp/src/timer.c",
             "tcp_send_buffer.c": "mtcp/src/tcp_send_buffer.c", "core.c": "mtcp/src/core.c"}
    lines = {f: len(open(os.path.join(ref, p), errors="replace").read().splitlines()) for f, p in where.items()}
    cites = re.findall(r"\b([a-z_]+\.[ch]):(\d+)(?:-(\d+))?((?:,? (?:and )?:\d+(?:-\d+)?)*)", hdr)
    assert len(cites) > 40
    for f, a, b, more in cites:
        assert f in lines, f
        for x, y in [(a, b)] + re.findall(r":(\d+)(?:-(\d+))?", more):
            assert 1 <= int(x) <= int(y or x) <= lines[f], (f, x, y)
    src = open(os.path.join(ref, where["tcp_in.c"]), errors="replace").read().splitlines()
    assert "ProcessACK(" in src[302] and "EstimateRTT(" in src[248] and "SBRemove(" in src[510]
    tim = open(os.path.join(ref, where["timer.c"]), errors="replace").read().splitlines()
    assert "UpdateRetransmissionTimer(" in tim[148]


def test_work_bytes_is_monotonic_and_zero_only_above_the_limits():
    from mtcp_amd import gpu
    wb = gpu.Context.ackwalk_work_bytes
    ns = [0, 1, 2, 63, 64, 65, 4095, 4096, 4097, 1 << 20, (1 << 26) - 1, 1 << 26]
    ids = [0, 1, 255, 65535, 1 << 20, gm.MAX_ID - 1, gm.MAX_ID]
    grid = [[wb(n, i) for i in ids] for n in ns]
    assert all(v > 0 and v % 16 == 0 for row in grid for v in row)
    assert all(grid[a][c] <= grid[a + 1][c] for a in range(len(ns) - 1) for c in range(len(ids)))
    assert all(grid[a][c] <= grid[a][c + 1] for a in range(len(ns)) for c in range(len(ids) - 1))
    assert wb((1 << 26) + 1, 5) == 0 and wb(5, gm.MAX_ID + 1) == 0 and wb(5, gm.FLOW_NONE) == 0
    assert gpu.Context.ackwalk_short_len() >= 1


# ---- the family the GPU tests share ----------------------------------------------------------------
@pytest.fixture(scope="module")
def family():
    b = ag.family()
    ag.expect(b)
    return b


def test_family_defers_little_and_reaches_what_matters(family):
    ack = family["want"][0]
    walked = family["sid"] <= family["max_id"]
    n = int(walked.sum())
    counts = np.bincount(ack["verdict"], minlength=16)
    assert counts[am.NONE] == 150 and len(ack) == n + 150
    assert counts[list(am.DEFERS)].sum() * 20 <= n, counts.tolist()               # at most 5 % deferred
    for name, c in (("ACK_NEW", counts[am.ACK_NEW]), ("ACK_OLD", counts[am.ACK_OLD]),
                    ("DUP", (ack["flags"] & T.ACK_DUP != 0).sum()), ("FAST_RTX", (ack["flags"] & T.ACK_FAST_RTX != 0).sum()),
                    ("WND_UPDATE", (ack["flags"] & T.ACK_WND_UPDATE != 0).sum())):
        assert c * 100 >= n, (name, int(c), n)                                    # each in at least 1 %
    for v in am.WALKED:
        assert counts[v] > 0, am.ACK_VERDICTS[v]
    for name, bit in zip(T.ACK_FLAGS, FLAG_BITS):
        assert (ack["flags"] & bit).any(), name
    assert (family["want"][1]["user"] == family["snd"]["user"]).all()


# ---- the kernels' step function, compiled for the host -----------------------------------------------
def pattern_lib():
    P = ctypes.CDLL(os.path.join(ROOT, "tools", "libackwalk_pattern.so"))
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    P.ackwalk_host_loop.argtypes = [vp, vp, vp, u32, u32, vp, vp, vp, u32, u32, vp, vp, vp]
    P.ackwalk_host_loop.restype = None
    return P


def host_loop(b, P=None):
    P = P or pattern_lib()
    idx, seg_sid, seg_start = b["group"]
    n, m = len(b["res"]), len(seg_sid)
    res, snd, place = np.ascontiguousarray(b["res"]), b["snd"].copy(), np.ascontiguousarray(b["place"])
    opt = np.ascontiguousarray(b["opt"]) if b["opt"] is not None else None
    ack, stop = np.full(16 * n, 0xA5, np.uint8).view(ACK_REC_DTYPE).copy(), np.zeros(m, np.uint32)
    P.ackwalk_host_loop(res.ctypes.data, None if opt is None else opt.ctypes.data, place.ctypes.data, n, b["max_id"],
                        idx.ctypes.data, seg_sid.ctypes.data, seg_start.ctypes.data, m, b["cur_ts"], snd.ctypes.data,
                        ack.ctypes.data, stop.ctypes.data)
    return ack, snd, stop


def same(got, want, what=""):
    for g, w, name in zip(got, want, ("ack", "snd", "ack_stop")):
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, f"{what}: {name} differs at {bad[:5].tolist()}: {g[bad[0]]} want {w[bad[0]]}"


def test_host_compiled_step_function_matches_the_fixture(golden):
    """One call per packet (the fixture's cur_ts differs from packet to packet): the state after every packet,
    the record's rmlen and flags against the reference's counts."""
    P = pattern_lib()
    res, opt, place = np.zeros(1, RESULT_DTYPE), np.zeros(1, TCPOPT_DTYPE), np.zeros(1, RCV_PLACE_DTYPE)
    one = {"res": res, "opt": opt, "place": place, "max_id": 0,
           "group": (np.zeros(1, np.uint32), np.zeros(1, np.uint32), np.array([0, 1], np.uint32))}
    for w, (first, fam, pk) in enumerate(golden):
        snd = np.array([first])
        for i, (inp, (counts, removed, words)) in enumerate(pk):
            seq, ack_seq, ts_ref, cur_ts, window, ln, has_ack, has_ts, ret = inp
            res["seq"], res["ack_seq"], res["window"], res["payload_len"] = seq, ack_seq, window, ln
            res["tcp_flags"], place["verdict"] = ACK if has_ack else 0, RCV_ACK_ONLY if ret else RCV_SEQ_OLD
            opt["ts_ref"], opt["flags"] = ts_ref, TCPOPT_TS_FOUND if has_ts else 0
            ack, snd, stop = host_loop(dict(one, snd=snd, cur_ts=cur_ts), P)
            what = f"walk {w} packet {i}"
            assert am.Snd.from_record(snd[0]).words() == words, what
            r = tuple(int(ack[0][f]) for f in ("rmlen", "snd_nxt", "cwnd", "flags", "verdict", "dup_acks"))
            assert counts_of(r) == counts and r[0] == removed and stop[0] == 1, what
        assert snd[0].tobytes()[72:83] == first.tobytes()[72:83] and snd[0].tobytes()[86:] == first.tobytes()[86:]


def test_host_compiled_step_function_matches_the_model(family):
    same(host_loop(family), family["want"], "the family")
    b = ag.drop_options(dict(family))
    same(host_loop(b), ag.expect(b), "no option records")
    rng = np.random.default_rng(7)
    b = ag.batch(rng, [12] * 300, wrap=True)
    same(host_loop(b), ag.expect(b), "wrapping streams")


def test_host_compiled_step_function_on_random_state_bytes():
    b = ag.garbage_batch(np.random.default_rng(8), 4000, 6)
    want = ag.expect(b)
    counts = np.bincount(want[0]["verdict"], minlength=16)
    assert counts[am.DEFER_BAD_STATE] > 1000 and counts[am.ACK_NEW] > 200 and counts[am.DEFER_ARITH] > 10 and \
        counts[am.DEFER_RCV] > 500 and counts[am.ACK_BEYOND] > 100 and counts[am.ACK_OLD] > 100, counts.tolist()
    same(host_loop(b), want, "random state bytes")
    assert (want[1]["user"] == b["snd"]["user"]).all()
