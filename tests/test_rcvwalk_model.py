"""The receive walk on the CPU (include/mtcp_gpu_rcvwalk.h): tests/rcvwalk_model.py
against a fixture the reference's own code wrote
(tests/golden/rcvwalk_cases.bin, written by tests/make_rcvwalk_golden.py; this
test reads only the fixture), the known answer, the deferral rules, the header's
layouts and citations, the workspace size, the statistics of the family the
GPU tests share, a built case for every DEFER reason, and the kernels' own step
function compiled for the host (tools/rcvwalk_pattern.hip) against the model."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

from mtcp_amd._types import (RCV_ACK_AGGREGATE, RCV_ACK_NOW, RCV_COPY, RCV_PLACE_DTYPE, RCV_READ_EVENT,
                             RCV_STATE_DTYPE, RCV_TS_NEWER, RESULT_DTYPE, TCPOPT_DTYPE, TCPOPT_TS_FOUND,
                             TCPOPT_TS_UNPINNED)
from tests import group_model as gm
from tests import rcvwalk_gen as rg
from tests import rcvwalk_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACK = 0x10


# ---- the fixture ---------------------------------------------------------------------------------
def read_golden():
    """[(irs, size, rcv_wnd, ts_recent, saw_ts, [(inputs, outputs)])] of tests/golden/rcvwalk_cases.bin
    (tests/c/ref_rcvwalk_gen.c has the layout)."""
    raw = open(os.path.join(ROOT, "tests", "golden", "rcvwalk_cases.bin"), "rb").read()
    magic, version, walks, per = struct.unpack_from("<4I", raw, 0)
    assert magic == 0x57564352 and version == 1 and per == 16
    off, out = 16, []
    for _ in range(walks):
        irs, size, wnd, ts_recent, saw_ts, npkt = struct.unpack_from("<6I", raw, off)
        off += 24
        pk = []
        for _ in range(npkt):
            seq, ts_val, ts_ref, ln, read = struct.unpack_from("<3I2H", raw, off)
            ret, n_now, n_agg, n_read, has_ts, nf, zero = struct.unpack_from("<b5BH", raw, off + 16)
            st = struct.unpack_from("<6I", raw, off + 24)
            frags = [list(struct.unpack_from("<2I", raw, off + 48 + 8 * k)) for k in range(nf)]
            off += 48 + 8 * nf
            assert zero == 0
            pk.append(((seq, ts_val, ts_ref, ln, read, has_ts), (ret, n_now, n_agg, n_read, st, frags)))
        out.append((irs, size, wnd, ts_recent, saw_ts, pk))
    assert off == len(raw) and len(raw) <= 1 << 20
    return out


@pytest.fixture(scope="module")
def golden():
    return read_golden()


def state_tuple(st):
    return (st.rcv_nxt, st.rcv_wnd, st.head_seq, st.merged_len, st.ts_recent, st.ts_lastack_rcvd)


def start_of(walk):
    irs, size, wnd, ts_recent, saw_ts, _ = walk
    st = rm.Stream.fresh(irs, size, saw_ts, ts_recent)
    st.rcv_wnd = wnd
    return st


def test_model_matches_the_references_own_walks(golden):
    """After every packet: ValidateSequence's return, the six state words, the
    fragment list, the ACK_OPT_NOW / ACK_OPT_AGGREGATE / RaiseReadEvent counts."""
    assert 800 <= len(golden) <= 1100
    seen = set()
    most_frags = 0
    for w, walk in enumerate(golden):
        st = start_of(walk)
        for i, ((seq, ts_val, ts_ref, ln, read, has_ts), (ret, n_now, n_agg, n_read, want, frags)) in enumerate(walk[5]):
            if read:
                rm.app_read(st, read)
            p = rm.step(st, (seq, ts_val, ts_ref, ln, ACK, TCPOPT_TS_FOUND if has_ts else 0), deferral=False)
            what = f"walk {w} packet {i}: {rm.RCV_VERDICTS[p[4]]}"
            assert (p[4] >= rm.ACK_ONLY) == bool(ret), what
            assert state_tuple(st) == want, what
            assert st.frags == frags, what
            assert (bool(p[5] & RCV_ACK_NOW), bool(p[5] & RCV_ACK_AGGREGATE), bool(p[5] & RCV_READ_EVENT)) == \
                (n_now == 1, n_agg == 1, n_read == 1), what
            assert n_now + n_agg <= 1 and n_read <= n_agg, what
            assert (p[1], p[2]) == (st.rcv_nxt, st.rcv_wnd)
            seen.add(p[4])
            most_frags = max(most_frags, len(frags))
    assert seen == set(rm.WALKED), sorted(seen)            # every walked verdict is in the fixture
    assert most_frags > 4                                  # and lists that grow past four fragments


def test_fixture_holds_every_kind_of_walk(golden):
    ts = sum(1 for w in golden if w[4])
    assert 0.3 < ts / len(golden) < 0.7                    # streams with and without timestamps
    assert {w[1] for w in golden} == {4096, 65536}
    assert sum(1 for w in golden if w[0] > 0xFFFFFFFF - 2001) > 100   # the walk wraps
    far = sum(1 for w in golden for (seq, _, _, ln, _, _), (_, _, _, _, st, _) in w[5]
              if 0x80000000 in (((seq - st[0]) & rm.M32), ((seq + ln - st[0]) & rm.M32)))
    assert far > 50                                        # a distance of exactly 2^31 to rcv_nxt


def test_deferral_agrees_with_the_plain_walk_in_front_of_the_first_deferral(golden):
    deferred = 0
    for walk in golden:
        a, b = start_of(walk), start_of(walk)
        for (seq, ts_val, ts_ref, ln, read, has_ts), _ in walk[5]:
            if read:
                rm.app_read(a, read)
                rm.app_read(b, read)
            pkt = (seq, ts_val, ts_ref, ln, ACK, TCPOPT_TS_FOUND if has_ts else 0)
            before = (state_tuple(b), [list(f) for f in b.frags])
            pb = rm.step(b, pkt)
            if pb[4] in rm.DEFERS:
                assert pb == rm.place(verdict=rm.DEFER_FRAG_FULL) and len(b.frags) == 4
                assert (state_tuple(b), b.frags) == before             # a deferred packet changes nothing
                deferred += 1
                break
            assert pb == rm.step(a, pkt, deferral=False)
            assert (state_tuple(a), a.frags) == (state_tuple(b), b.frags)
    assert deferred > 50


# ---- the known answer ------------------------------------------------------------------------------
def test_known_answer():
    st = rm.Stream.fresh(999, 8192)
    assert (st.rcv_nxt, st.rcv_wnd) == (1000, 8192)
    got = [rm.step(st, (seq, 0, 0, ln, ACK, 0)) for seq, ln in
           ((1000, 1000), (3000, 500), (2000, 1000), (1000, 1000), (2500, 100))]
    agg_read = RCV_ACK_AGGREGATE | RCV_READ_EVENT | RCV_COPY
    assert got == [(0, 2000, 7192, 1000, rm.PUT_STORED, agg_read),
                   (2000, 2000, 7192, 500, rm.PUT_STORED, RCV_ACK_NOW | RCV_COPY),
                   (1000, 3500, 5692, 1000, rm.PUT_STORED, agg_read),
                   (0, 3500, 5692, 0, rm.SEQ_OLD, RCV_ACK_AGGREGATE),
                   (0, 3500, 5692, 0, rm.SEQ_OLD, RCV_ACK_AGGREGATE)]
    assert st.frags == [[1000, 2500]]


def test_the_two_orders_differ_at_exactly_two_to_the_31():
    a, b = 5, (5 + 0x80000000) & rm.M32
    assert rm.TCP_SEQ_LT(a, b) and rm.TCP_SEQ_LT(b, a)             # (int32_t)0x80000000 < 0 both ways
    assert rm.GetMinSeq(a, b) == b and rm.GetMinSeq(b, a) == b      # 2^31 > MAXSEQ/2: the larger value is "before"
    assert rm.GetMinSeq(a, (b - 1) & rm.M32) == a and rm.TCP_SEQ_LT(a, b - 1) and not rm.TCP_SEQ_LT(b - 1, a)


# ---- every DEFER reason, built ---------------------------------------------------------------------
def four_fragments():
    st = rm.Stream.fresh(99, 65536)
    for seq in (1000, 2000, 3000, 4000):
        assert rm.step(st, (seq, 0, 0, 100, ACK, 0))[4] == rm.PUT_STORED
    assert len(st.frags) == 4
    return st


def raw_state(st):
    return rg.record_of(st).tobytes()


def test_every_defer_reason():
    pkt = (100, 0, 0, 10, ACK, 0)
    cases = []
    st = rm.Stream.fresh(99, 4096)
    st.tcp_state = 7
    cases.append((st, pkt, True, rm.DEFER_STATE))
    for field, value in (("rsvd", 1), ("nfrag_field", 5), ("size", (1 << 30) + 1), ("merged_len", 4097)):
        st = rm.Stream.fresh(99, 4096)
        setattr(st, field, value)
        cases.append((st, pkt, True, rm.DEFER_BAD_STATE))
    st = rm.Stream.fresh(99, 4096)
    st.frags = [[100, 1 << 31]]
    st.nfrag_field = 1
    cases.append((st, pkt, True, rm.DEFER_BAD_STATE))
    for flag in (0x01, 0x02, 0x04):
        cases.append((rm.Stream.fresh(99, 4096), (100, 0, 0, 10, ACK | flag, 0), True, rm.DEFER_FLAGS))
    cases.append((rm.Stream.fresh(99, 4096, 1), (100, 5, 0, 10, ACK, TCPOPT_TS_FOUND), False, rm.DEFER_TS))
    cases.append((rm.Stream.fresh(99, 4096, 1), (100, 0, 0, 10, ACK, TCPOPT_TS_UNPINNED), True, rm.DEFER_TS))
    cases.append((four_fragments(), (5000, 0, 0, 100, ACK, 0), True, rm.DEFER_FRAG_FULL))       # the fifth fragment
    # RBPut's insert behind a NULL prev: the loop breaks at the first fragment (the segment ends in front of it)
    # while GetMinSeq does not put the segment first: the two orders at a distance of 2^31
    st = rm.Stream.fresh(99, 1 << 30)
    st.frags, st.nfrag_field, st.rcv_wnd = [[(100 + 50 + 0x7FFFFFFF) & rm.M32, 10]], 1, 1 << 30
    cases.append((st, (101, 0, 0, 50, ACK, 0), True, rm.DEFER_BAD_STATE))
    with pytest.raises(rm.NullPrev):
        rm.step(rm.Stream.from_record(rg.record_of(st)), (101, 0, 0, 50, ACK, 0), deferral=False)
    for st, p, has_opt, want in cases:
        before = raw_state(st)
        assert rm.step(st, p, has_opt) == rm.place(verdict=want), rm.RCV_VERDICTS[want]
        assert raw_state(st) == before, rm.RCV_VERDICTS[want]
    # the fifth fragment's neighbours: a segment that merges is stored while the list is full
    st = four_fragments()
    assert rm.step(st, (1100, 0, 0, 900, ACK, 0))[4] == rm.PUT_STORED and len(st.frags) == 3


def test_a_batch_defers_behind_and_keeps_the_state():
    """The first deferred packet stops its stream: the later ones are
    DEFER_BEHIND, seg_stop names the position, the record holds what the
    packets in front left."""
    res, opt = np.zeros(6, RESULT_DTYPE), np.zeros(6, TCPOPT_DTYPE)
    res["seq"], res["payload_len"] = [1000, 1100, 1200, 1300, 7, 1400], 100
    res["tcp_flags"] = [ACK, ACK, ACK | 0x01, ACK, ACK, ACK]
    sid = np.array([3, 3, 3, 3, rm.FLOW_MISS, 3], np.uint32)
    state = np.zeros(6, RCV_STATE_DTYPE)
    state[3] = rg.record_of(rm.Stream.fresh(999, 8192))
    state[5] = rg.record_of(rm.Stream.fresh(5, 4096))
    idx, seg_sid, seg_start = gm.group(sid, 5)
    place, new, stop = rm.walk(res, opt, 5, idx, seg_sid, seg_start, state)
    assert place["verdict"].tolist() == [rm.PUT_STORED, rm.PUT_STORED, rm.DEFER_FLAGS, rm.DEFER_BEHIND, rm.NONE,
                                         rm.DEFER_BEHIND]
    assert stop.tolist() == [2, 5] and seg_sid.tolist() == [3, rm.FLOW_MISS]
    assert new[3]["rcv_nxt"] == 1200 and new[3]["nfrag"] == 1
    assert new[5].tobytes() == state[5].tobytes() and place[4].tobytes() == bytes(16)
    assert place[3].tobytes() == bytes(14) + bytes([rm.DEFER_BEHIND, 0])


# ---- the header ------------------------------------------------------------------------------------
def test_header_layouts_offsets_and_citations():
    hdr = open(os.path.join(ROOT, "include", "mtcp_gpu_rcvwalk.h")).read()
    assert re.search(r"#define MTCP_GPU_HAS_RCVWALK\s+1\b", hdr)
    assert "MTCP_GPU_ABI_VERSION" in hdr and "extern \"C\"" in hdr
    for name, dt in (("mtcp_gpu_rcv_state", RCV_STATE_DTYPE), ("mtcp_gpu_rcv_place", RCV_PLACE_DTYPE)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
        fields = re.findall(r"(\w+)(?:\[\w+\])?;\s*/\*\s*(\d+) ", body)
        assert [(f, int(o)) for f, o in fields] == [(f, dt.fields[f][1]) for f in dt.names], name
    assert RCV_STATE_DTYPE.itemsize == 64 and RCV_PLACE_DTYPE.itemsize == 16
    for k, v in enumerate(rm.RCV_VERDICTS):
        assert re.search(r"MTCP_GPU_RCV_%s\s*=\s*%d\b" % (v, k), hdr), v
    for k, v in (("COPY", RCV_COPY), ("ACK_NOW", RCV_ACK_NOW), ("ACK_AGGREGATE", RCV_ACK_AGGREGATE),
                 ("READ_EVENT", RCV_READ_EVENT), ("TS_NEWER", RCV_TS_NEWER)):
        assert re.search(r"#define MTCP_GPU_RCV_%s\s+0x%02xu" % (k, v), hdr), k
    # the head comment and every entry point cite the three ranges
    cites = ("tcp_in.c:101-179", "tcp_in.c:537-610", "tcp_ring_buffer.c:280-382")
    pieces = [hdr[:hdr.index("#ifndef")]]
    for fn in ("mtcp_gpu_rcvwalk_work_bytes", "mtcp_gpu_rcvwalk_short_len", "mtcp_gpu_rcvwalk_dev", "mtcp_gpu_rcvwalk"):
        at = re.search(r"\b%s\(" % fn, re.sub(r"/\*.*?\*/", lambda m: " " * len(m.group(0)), hdr, flags=re.S)).start()
        pieces.append(hdr[hdr.rindex("/*", 0, at):at])
    for text in pieces:
        flat = " ".join(text.replace("*", " ").split())
        for c in cites:
            assert c in flat, (c, text[:60])


def test_work_bytes_is_monotonic_and_zero_only_above_the_limits():
    from mtcp_amd import gpu
    wb = gpu.Context.rcvwalk_work_bytes
    ns = [0, 1, 2, 63, 64, 65, 4095, 4096, 4097, 1 << 20, (1 << 26) - 1, 1 << 26]
    ids = [0, 1, 255, 65535, 1 << 20, gm.MAX_ID - 1, gm.MAX_ID]
    grid = [[wb(n, i) for i in ids] for n in ns]
    assert all(v > 0 and v % 16 == 0 for row in grid for v in row)
    assert all(grid[a][c] <= grid[a + 1][c] for a in range(len(ns) - 1) for c in range(len(ids)))
    assert all(grid[a][c] <= grid[a][c + 1] for a in range(len(ns)) for c in range(len(ids) - 1))
    assert wb((1 << 26) + 1, 5) == 0 and wb(5, gm.MAX_ID + 1) == 0 and wb(5, gm.FLOW_NONE) == 0
    assert gpu.Context.rcvwalk_short_len() >= 1


# ---- the family the GPU tests share ----------------------------------------------------------------
@pytest.fixture(scope="module")
def family():
    rng = np.random.default_rng(2024)
    b = rg.batch(rng, rg.family_lens(rng, 500), extra=150, special=rg.family_special)
    b["group"] = gm.group(b["sid"], b["max_id"])
    b["want"] = rm.walk(b["res"], b["opt"], b["max_id"], *b["group"], b["state"])
    return b


def test_family_reaches_every_walked_verdict_and_defers_little(family):
    place = family["want"][0]
    n = len(place)
    counts = np.bincount(place["verdict"], minlength=16)
    for v in rm.WALKED:
        assert counts[v] * 200 >= n, (rm.RCV_VERDICTS[v], int(counts[v]), n)
    assert counts[list(rm.DEFERS)].sum() * 10 <= n, counts.tolist()
    assert counts[rm.NONE] == 150
    assert (place["flags"] & RCV_TS_NEWER).any() and (place["flags"] & RCV_READ_EVENT).any()
    assert family["want"][1]["nfrag"].max() == 4           # ordinary reordering fills the four slots


# ---- the kernels' step function, compiled for the host -----------------------------------------------
def host_loop(b, group=None, with_opt=True):
    lib = os.path.join(ROOT, "tools", "librcvwalk_pattern.so")
    P = ctypes.CDLL(lib)
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    P.rcvwalk_host_loop.argtypes = [vp, vp, u32, u32, vp, vp, vp, u32, vp, vp, vp]
    P.rcvwalk_host_loop.restype = None
    idx, seg_sid, seg_start = group or b["group"]
    n, m = len(b["res"]), len(seg_sid)
    res, state = np.ascontiguousarray(b["res"]), b["state"].copy()
    opt = np.ascontiguousarray(b["opt"]) if with_opt and b["opt"] is not None else None
    place, stop = np.full(16 * n, 0xA5, np.uint8).view(RCV_PLACE_DTYPE).copy(), np.zeros(m, np.uint32)
    P.rcvwalk_host_loop(res.ctypes.data, None if opt is None else opt.ctypes.data, n, b["max_id"], idx.ctypes.data,
                        seg_sid.ctypes.data, seg_start.ctypes.data, m, state.ctypes.data, place.ctypes.data,
                        stop.ctypes.data)
    return place, state, stop


def same(got, want, what=""):
    for g, w, name in zip(got, want, ("place", "state", "seg_stop")):
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, f"{what}: {name} differs at {bad[:5].tolist()}: {g[bad[0]]} want {w[bad[0]]}"


def test_host_compiled_step_function_matches_the_model(family):
    same(host_loop(family), family["want"], "the family")
    want = rm.walk(family["res"], None, family["max_id"], *family["group"], family["state"])
    same(host_loop(family, with_opt=False), want, "no option records")
    rng = np.random.default_rng(7)
    b = rg.batch(rng, [12] * 300, wrap=True)
    b["group"] = gm.group(b["sid"], b["max_id"])
    same(host_loop(b), rm.walk(b["res"], b["opt"], b["max_id"], *b["group"], b["state"]), "wrapping streams")


def test_host_compiled_step_function_on_random_state_bytes():
    b = rg.garbage_batch(np.random.default_rng(8), 4000, 6)
    b["group"] = gm.group(b["sid"], b["max_id"])
    want = rm.walk(b["res"], b["opt"], b["max_id"], *b["group"], b["state"])
    counts = np.bincount(want[0]["verdict"], minlength=16)
    assert counts[rm.DEFER_BAD_STATE] > 1000 and counts[rm.PUT_STORED] > 200 and counts[rm.PAWS_OLD] > 500 and \
        counts[rm.DEFER_FRAG_FULL] > 10 and counts[rm.PUT_DROPPED] > 10 and counts[rm.PUT_NO_ROOM] > 10, counts.tolist()
    same(host_loop(b), want, "random state bytes")
