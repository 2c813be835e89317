"""The frame builder's model (tests/txbuild_model.py) pinned on the CPU:
against the frames the reference's own SendTCPPacketStandalone chain wrote
(tests/golden/txbuild_frames.*.bin), against the project's oracle (the rx
chain and the tx fill) and, for SendTCPPacket's SYN options, against the
restatement of ParseTCPOptions that the reference pins
(tests/tcpopt_model.py)."""
import os

import numpy as np
import pytest

import oracle
from mtcp_amd import TX_LINK_DTYPE, TX_SEG_DTYPE
from tests import tcpopt_model, txbuild_model as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE_TX = os.path.join(ROOT, "oracle", "_ref", "dropin_tx")
SLOT = 2048


@pytest.fixture(scope="module")
def frames():
    return m.load_fixture()


@pytest.fixture(scope="module")
def fixture_segs(frames):
    return m.segs_from_frames(frames)


mixed_segments = m.mixed_segments


def test_layouts_match_the_package():
    assert m.SEG_DTYPE == TX_SEG_DTYPE and m.LINK_DTYPE == TX_LINK_DTYPE
    hdr = open(os.path.join(ROOT, "include", "mtcp_gpu_txbuild.h")).read()
    assert "#define MTCP_GPU_HAS_TXBUILD        1" in hdr
    for name, (_, off) in ((n, TX_SEG_DTYPE.fields[n]) for n in ("payload_len", "flags", "link")):
        assert f"/* {off} " in hdr, name


def test_fixture_is_the_references_run(frames):
    """4 054 frames, none left out; where oracle/_ref/dropin_tx exists a fresh
    run reproduces the committed bytes."""
    sizes = [os.path.getsize(p) for p in m.FIXTURE_PARTS]
    assert len(frames) == m.FIXTURE_FRAMES and sum(sizes) == m.FIXTURE_BYTES and max(sizes) < m.PART_LIMIT
    lens = np.array([len(f) for f in frames])
    flags = np.array([f[47] for f in frames])
    assert len(np.unique(flags)) == 8
    plen = lens - 54 - np.where(flags & m.SYN, 20, 12)
    assert plen.min() == 0 and plen.max() == 1460 and (plen & 1).sum() == 1970 and (plen == 0).sum() == 97
    if os.path.exists(EXE_TX):
        from tests import make_txbuild_golden as g
        fresh = g.reference_stream()
        have = np.concatenate([np.fromfile(p, dtype=np.uint8) for p in m.FIXTURE_PARTS])
        assert np.array_equal(fresh, have)
        assert [len(p) for p in g.split(fresh)] == sizes


def test_model_rebuilds_every_reference_frame(frames, fixture_segs):
    """segs_from_frames then build_frames: the whole image of 2 048 B slots
    pre-filled with 0xA5 equals the reference's frames in it; the fields the
    builders never read carry garbage."""
    seg, payload, links = fixture_segs
    seg = m.garbage_unread_fields(seg)
    assert (seg["ack"][(seg["flags"] & m.ACK) == 0] == 0xDEADBEEF).all() and (seg["mss"] != 0).all()
    desc = m.slots([len(f) for f in frames], SLOT)
    blank = np.full(SLOT * len(frames), 0xA5, dtype=np.uint8)
    want = blank.copy()
    for i, f in enumerate(frames):
        want[i * SLOT:i * SLOT + len(f)] = f
    image, status = m.build_frames(seg, payload, links, desc, blank)
    assert not status.any()
    assert np.array_equal(image, want)
    # SYN frames carry doff 10 with 8 zero option bytes, all others doff 8
    for f in frames[:600]:
        syn = f[47] & m.SYN
        assert f[46] >> 4 == (10 if syn else 8)
        assert not syn or not f[66:74].any()


def test_model_frames_pass_the_oracles_rx_chain():
    seg, payload, links, desc, nbytes = mixed_segments()
    image, status = m.build_frames(seg, payload, links, desc, np.zeros(nbytes, np.uint8), max_mss=8960)
    assert not status.any()
    r = oracle.rx_chunk(image, desc, 0)
    assert (r["verdict"] == 0).all() and not r["ip_csum"].any() and not r["tcp_csum"].any()
    for f in ("saddr", "daddr", "sport", "dport", "seq", "window", "payload_len"):
        assert np.array_equal(r[f], seg[f]), f
    ack = (seg["flags"] & m.ACK) != 0
    assert np.array_equal(r["ack_seq"], np.where(ack, seg["ack"], 0))
    assert np.array_equal(r["tcp_flags"], seg["flags"])
    assert np.array_equal(r["ip_len"], 40 + np.where(seg["flags"] & m.SYN, 20, 12) + seg["payload_len"])
    ids = np.array([(int(image[int(d["offset"]) + 18]) << 8) | int(image[int(d["offset"]) + 19]) for d in desc])
    assert np.array_equal(ids, seg["ip_id"]) and ids.any()
    # the payload's bytes, at frame byte 54 + optlen
    for s, d in zip(seg, desc):
        at = int(d["offset"]) + 54 + m.optlen_of(int(s["flags"]))
        assert np.array_equal(image[at:at + int(s["payload_len"])],
                              payload[int(s["payload_off"]):int(s["payload_off"]) + int(s["payload_len"])])


def test_no_csum_image_filled_by_the_oracle_is_the_plain_image():
    seg, payload, links, desc, nbytes = mixed_segments(seed=12)
    blank = np.full(nbytes, 0xA5, np.uint8)
    plain, _ = m.build_frames(seg, payload, links, desc, blank, max_mss=8960)
    bare, status = m.build_frames(seg, payload, links, desc, blank, max_mss=8960, flags=m.NO_CSUM)
    assert not status.any() and not np.array_equal(bare, plain)
    for d in desc:
        o = int(d["offset"])
        assert not bare[o + 24:o + 26].any() and not bare[o + 50:o + 52].any()
    assert oracle.tx_fill(bare, desc, 0) == len(desc)
    assert np.array_equal(bare, plain)


def test_form1_syn_options_read_back_by_parse_tcp_options():
    """What ties form 1 to reference code: ParseTCPOptions, restated in
    tests/tcpopt_model.py and pinned there by the reference's own outputs,
    reads back mss, wscale and the timestamps GenerateTCPOptions' layout
    carries (no committed recipe calls SendTCPPacket itself)."""
    seg, payload, links, desc, nbytes = mixed_segments(seed=13)
    image, _ = m.build_frames(seg, payload, links, desc, np.zeros(nbytes, np.uint8), max_mss=8960)
    seen = 0
    for s, d in zip(seg, desc):
        o = int(d["offset"]) + 54
        optlen = m.optlen_of(int(s["flags"]))
        block = np.concatenate([image[o:o + optlen], np.zeros(16, np.uint8)])
        ts = tcpopt_model.walk_ts(block, optlen)
        assert (ts["ret"], ts["ts_val"], ts["ts_ref"]) == (1, s["ts_val"], s["ts_ecr"])
        if s["form"] == 1 and s["flags"] & m.SYN:
            w = tcpopt_model.walk_syn(block, optlen)
            assert (w["mss"], w["wscale"], w["ts_recent"], w["saw_timestamp"]) == \
                (s["mss"], s["wscale"], s["ts_val"], 1)
            assert w["seen"] == tcpopt_model.MSS | tcpopt_model.WSCALE and not w["nonterm"]
            assert bytes(block[:4]) == bytes([2, 4, int(s["mss"]) >> 8, int(s["mss"]) & 0xFF])
            assert bytes(block[16:20]) == bytes([1, 3, 3, int(s["wscale"])])
            seen += 1
        elif s["flags"] & m.SYN:
            assert not block[12:20].any()              # tcp_out.c:160: the memset's zeros
    assert seen >= 10


def test_status_order_and_untouched_slots():
    seg, payload, links, desc, nbytes = mixed_segments(seed=14)
    seg, desc = seg[:8].copy(), desc[:8].copy()
    seg["flags"][0] |= 0x20                       # BAD_SEG
    desc["len"][0] += 1                           # ... wins over BAD_DESC
    seg["form"][1] = 2
    seg["link"][2] = 3
    desc["offset"][3] += 1                        # BAD_DESC: odd
    seg["payload_off"][3] = len(payload)          # ... wins over BAD_PAYLOAD
    seg["payload_off"][4] = len(payload) - int(seg["payload_len"][4]) + 1
    seg["payload_len"][5] = 1460 + m.optlen_of(int(seg["flags"][5])) + 1
    desc["len"][5] = m.frame_len(int(seg["flags"][5]), int(seg["payload_len"][5]))
    blank = np.full(nbytes, 0xA5, np.uint8)
    image, status = m.build_frames(seg, payload, links, desc, blank)
    assert status[:6].tolist() == [m.BAD_SEG, m.BAD_SEG, m.BAD_SEG, m.BAD_DESC, m.BAD_PAYLOAD, m.BAD_SEG]
    for i in range(6):
        assert (image[i * 9216:(i + 1) * 9216] == 0xA5).all()


@pytest.mark.parametrize("flags", [m.ACK | m.PSH, m.SYN, m.SYN | m.ACK, m.RST])
def test_vectorised_model_equals_the_per_segment_model(flags):
    """build_uniform (what tools/txbuild_bench.py checks a million frames
    with) against build_frame, strided and scattered source offsets."""
    rng = np.random.default_rng(flags)
    for plen in (0, 1, 7, 1448, 1449):
        for scattered in (False, True):
            n = 40
            seg = np.zeros(n, m.SEG_DTYPE)
            for f in ("saddr", "daddr", "seq", "ack", "ts_val", "ts_ecr"):
                seg[f] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
            for f in ("sport", "dport", "window", "ip_id", "mss"):
                seg[f] = rng.integers(0, 1 << 16, n)
            seg["wscale"], seg["link"], seg["form"] = rng.integers(0, 15, n), rng.integers(0, 2, n), rng.integers(0, 2, n)
            seg["flags"], seg["payload_len"] = flags, plen
            seg["payload_off"] = np.arange(n) * (plen + 16) + (rng.integers(0, 16, n) if scattered else 3)
            payload = rng.integers(0, 256, int(seg["payload_off"].max()) + plen, dtype=np.uint8)
            links = np.zeros(2, m.LINK_DTYPE)
            links["dst"], links["src"] = rng.integers(0, 256, (2, 6)), rng.integers(0, 256, (2, 6))
            F = m.build_uniform(seg, payload, links)
            for i in range(n):
                assert np.array_equal(F[i], m.build_frame(seg[i], payload, links[int(seg[i]["link"])])), (plen, i)
