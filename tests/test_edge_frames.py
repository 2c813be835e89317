"""The edge batches of tests/edge_frames.py discriminate (CPU): they are
deterministic, every byte around a frame would show in a checksum if a kernel
read it, the frames cover the cells of the kernels' chunk grid they claim to,
the oracle gives each family the verdicts it was built for, each family's
average slot dispatches the kernel tests/test_gpu_edges.py names for it, and
the oracle's answers on them are the reference's own (where oracle/_ref was
built).  Without this the GPU sweep would prove little."""
import ctypes

import numpy as np
import pytest

import oracle
from tests import edge_frames as ef

V_OK, V_IP_SHORT, V_ICMP, V_TCP_LEN_BAD, V_TRUNCATED, V_BAD_DESC = 0, 3, 6, 8, 10, 11


def _shift(name):
    return int(name[1:]) if name[0] == "D" else 0


def _frames(name):
    """Byte start and length of every frame placed in the family's buffer."""
    out = ef.get(name)
    buf, desc = out[:2]
    if name[0] == "D":
        desc = desc[:out[2]]
    return buf, desc["offset"].astype(np.int64) << _shift(name), desc["len"].astype(np.int64)


@pytest.mark.parametrize("name", ef.FAMILIES)
def test_builds_are_deterministic(name):
    a, b = ef.build(name), ef.build(name)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert a[0].tobytes() == ef.get(name)[0].tobytes()


@pytest.mark.parametrize("name", ef.FAMILIES)
def test_garbage_rule(name):
    buf, starts, lens = _frames(name)
    covered = np.zeros(len(buf) + 1, np.int32)
    np.add.at(covered, starts, 1)
    np.add.at(covered, starts + lens, -1)
    depth = np.cumsum(covered)[:-1]
    assert depth.max() == 1, "frames overlap"
    outside = buf[depth == 0]
    assert outside.min() >= 1 and outside.max() <= 254
    assert ef.window_violations(buf, starts, lens) == []
    if name[0] != "D":
        # a garbage byte on either side of every frame, a full window before the first and after the last
        assert starts[0] >= 256 and len(buf) - (starts[-1] + lens[-1]) >= 256
        assert (starts[1:] > (starts + lens)[:-1]).all()
        assert (starts & 1 == 0).all()


def test_window_rule_would_notice():
    """The window check itself: a planted run summing to 0xFFFF is reported."""
    buf = np.full(1024, 7, np.uint8)
    buf[398:400] = (0xFF - 7, 0xFF - 7)                  # words 0x0707 + 0xF8F8 just before the frame
    assert (0, 0) in ef.window_violations(buf, [400], [100])
    buf[398:400] = 7
    assert ef.window_violations(buf, [400], [100]) == []
    buf[500] = 0
    buf[501] = 0                                        # a zero word just past its end
    assert (0, 1) in ef.window_violations(buf, [400], [100])


def test_sweep_covers_every_granule_boundary():
    cells = set()
    for name in ("S", "M", "J"):
        nch, sh = ef.nch_of(ef.get(name)[1])
        cells |= set(zip(nch.tolist(), sh.tolist()))
    for g in ef.GRANULES:
        for k in (1, 2):
            for nch in (k * g - 1, k * g, k * g + 1):
                if nch < 5:
                    continue
                for sh in ef.PHASES:
                    assert (nch, sh) in cells, (g, k, nch, sh)
    # the starts spread over the 128 B line: every 16 B position of it
    for name in ("S", "M", "J", "H", "P"):
        p = ef.get(name)[1]["offset"].astype(np.int64)
        assert set(((p & 127) >> 4).tolist()) == set(range(8)), name


def test_header_family_covers_the_chunk_grid():
    _, desc = ef.get("H")
    specs = ef.h_specs()
    sh = (desc["offset"].astype(np.int64) & 15).tolist()
    assert [s[1] for s in specs] == sh
    seen = {(s[2], s[3], s[1]) for s in specs}
    assert seen == {(i, d, p) for i in range(5, 16) for d in range(5, 16) for p in ef.PHASES}
    # T = 14 + 4 * ihl and the starts are even: sh + T takes every even value mod 16
    assert {(s[1] + 14 + 4 * s[2]) & 15 for s in specs} == set(range(0, 16, 2))
    assert len(specs) == 11 * 11 * 8 * 9


def test_padding_family_covers_both_sides_of_the_fast_path():
    """rx_wave.hpp's one-trip fast path: ((e_rel + 15) >> 4) == nch, e_rel =
    sh + 14 + ip_len, te = e_rel & 15 — every te with the segment ending in the
    last chunk and with padding pushing the frame's end past it."""
    _, desc = ef.get("P")
    specs = ef.p_specs()
    nch, sh = ef.nch_of(desc)
    sides = {True: set(), False: set()}
    for (spec, pad), n, s in zip(specs, nch.tolist(), sh.tolist()):
        if pad < 0 or spec[4] < 40:                     # only a TCP_OK frame's segment is summed
            continue
        e_rel = s + 14 + spec[4]
        sides[((e_rel + 15) >> 4) == n].add(e_rel & 15)
    assert sides[True] == set(range(16)) and sides[False] == set(range(16))
    ends = {(int(o) & 15) + int(L) for o, L in zip(desc["offset"], desc["len"]) if L == 2046}
    assert min(ends) < 2048 <= max(ends) and max(ends) - 2048 < 16 and 2048 - min(ends) < 16


def test_oracle_verdicts():
    for name in ("S", "M", "J", "Mt"):
        want = ef.oracle_rx(name)
        assert (want["verdict"] == V_OK).all(), name
        assert (want["tcp_csum"] == 0).all() and (want["ip_csum"] == 0).all()
    v = ef.oracle_rx("H")["verdict"]
    short = np.array([s[4] < 4 * (s[2] + s[3]) for s in ef.h_specs()])
    assert short.sum() == 11 * 11 * 8 and (v[short] == V_TCP_LEN_BAD).all() and (v[~short] == V_OK).all()
    v = ef.oracle_rx("P")["verdict"]
    more = np.array([pad < 0 for _, pad in ef.p_specs()])
    tot = np.array([s[4] for s, _ in ef.p_specs()])
    # (the padding of a 60..64 B frame can leave less than the headers: tot_len < 40 or < 20)
    assert (v[more] == V_TRUNCATED).all() and (v[~more & (tot >= 40)] == V_OK).all()
    assert (v[~more & (tot >= 20) & (tot < 40)] == V_TCP_LEN_BAD).all() and (v[tot < 20] == V_IP_SHORT).all()
    assert (v == V_OK).sum() == 8 * (41 + 41 + 7 + 8 + 9 + 10 + 11)
    want = ef.oracle_rx("I")
    more = np.array([m for _, m in ef.i_specs()])
    assert (want["verdict"] == V_ICMP).all()
    assert (want["tcp_csum"][more] == 0).all() and (want["payload_len"][more] == 0).all()
    dl = np.array([s[4] - 4 * s[2] for s, _ in ef.i_specs()])
    assert (want["payload_len"][~more] == dl[~more]).all()
    assert len(np.unique(want["tcp_csum"][~more])) > 1000      # ICMPChecksum of random content
    for name in ("Z", "Zf"):
        buf, desc = ef.get(name)
        want = ef.oracle_rx(name)
        assert (want["verdict"] == V_OK).all() and not want["ip_csum"].any() and not want["tcp_csum"].any()
        stored = 0x00 if name == "Z" else 0xFF
        for o in desc["offset"].astype(np.int64):
            assert (buf[[o + 24, o + 25, o + 50, o + 51]] == stored).all()
        filled = buf.copy()
        assert oracle.tx_fill(filled, desc, 0) == len(desc)
        for o in desc["offset"].astype(np.int64):           # the fill's canonical answer: 0x0000 in both
            assert not filled[[o + 24, o + 25, o + 50, o + 51]].any()
    assert np.array_equal(ef.get("Z")[1], ef.get("Zf")[1])


D_WANT = {"at 2^32": V_BAD_DESC, "at 2^32 + one slot": V_BAD_DESC, "offset 0xFFFFFFFF": V_BAD_DESC,
          "one byte past buf_len": V_BAD_DESC, "length 60 at buf_len": V_BAD_DESC,
          "length 13 at 0": V_TRUNCATED, "odd start": V_BAD_DESC}


@pytest.mark.parametrize("s", ef.SHIFTS)
def test_descriptor_family(s):
    buf, desc, nv, cases = ef.get(f"D{s}")
    v = ef.oracle_rx(f"D{s}")["verdict"]
    assert (v[:nv] == V_OK).all()
    pos = desc["offset"].astype(np.uint64) << np.uint64(s)
    assert int(pos[nv - 1]) + int(desc["len"][nv - 1]) == len(buf)
    assert set(cases) == set(ef.D_CASES) - ({"odd start"} if s else {"at 2^32", "at 2^32 + one slot"})
    starts = {int(p): int(L) for p, L in zip(pos[:nv], desc["len"][:nv])}
    for name, p, L, got in zip(cases, pos[nv:].tolist(), desc["len"][nv:].tolist(), v[nv:].tolist()):
        if name == "length 0 at buf_len":
            # TRUNCATED at buf_len itself; where 2^s does not divide buf_len the next position is out of range
            assert got == (V_TRUNCATED if p == len(buf) else V_BAD_DESC) and p >= len(buf), (name, got)
        else:
            assert got == D_WANT[name], (name, got)
        if name.startswith("at 2^32"):
            # truncated to 32 bits: exactly a valid frame (a kernel that truncates answers TCP_OK)
            assert p >= 1 << 32 and starts[p & 0xFFFFFFFF] == L
        elif name == "offset 0xFFFFFFFF":
            assert p & 0xFFFFFFFF >= len(buf) or p & 1
    assert len(buf) % 16 == 0                           # the device entry points' contract
    assert (len(buf) % (1 << s) == 0) == (s != 16)      # "at buf_len" is buf_len itself up to shift 6


def test_slot_conditions():
    """The average slot mtcp_gpu.hip's launch sees (the 16 B-padded buffer over
    n) puts each family on the schedule the GPU test asserts for it
    (dispatch.hpp: big_schedule, kWaveShortUpToSlot)."""
    def slot(name):
        buf, desc = ef.get(name)[:2]
        return ((len(buf) + 15) & ~15) // len(desc), len(desc)
    s, n = slot("S")
    assert s < 1024                                     # rx_kernel<sorted>
    s, n = slot("M")
    assert 1024 <= s <= 1536                            # rx_wave_kernel<2 loads>; tiled: unrolled
    s, n = slot("Mt")
    assert 1024 <= s <= 1536 and n > 65536              # rx_kernel<unrolled>
    s, n = slot("J")
    assert s > 2048                                     # <10 loads>, rx_kernel<unrolled,line-aligned>
    lens = ef.get("M")[1]["len"]
    assert (lens > 2048).sum() > 1000 and lens.max() >= 4130


def _ref_pin(name, every=1, phase=None):
    buf, desc = ef.get(name)
    want = ef.oracle_rx(name, 0)
    R = oracle.ref()
    ret, csum = ctypes.c_int(0), ctypes.c_uint16(0)
    compared = 0
    offs, lens = desc["offset"].astype(np.int64), desc["len"].astype(np.int64)
    for i in range(0, len(desc), every):
        o, L = int(offs[i]), int(lens[i])
        if phase is not None and (o & 15) != phase:
            continue
        v = int(want["verdict"][i])
        if v == V_TRUNCATED:
            continue                                    # the reference would read past the frame
        pkt = np.zeros(L + 64, np.uint8)                # the reference may zero tcph->check: a copy
        pkt[:L] = buf[o:o + L]
        br = R.ref_rx_packet(pkt.ctypes.data, L, ctypes.byref(ret), ctypes.byref(csum))
        assert br == v, (name, i, L, br, v)
        if v in (0, 9):
            assert csum.value == int(want["tcp_csum"][i]), (name, i, csum.value, int(want["tcp_csum"][i]))
        compared += 1
    return compared


@pytest.mark.skipif(not oracle.ref_available(), reason="oracle/_ref not built (needs the reference's sources)")
def test_oracle_equals_reference_on_edge_frames():
    """Every frame of H, P, Z, Zf, and S at one phase: ProcessPacket's branch
    and TCPCalcChecksum's value are the oracle's (the exceptions are those of
    tests/test_oracle_fuzz_ref.py).  Zf pins the answer for a stored 0xFFFF
    check — TCP_OK, checksum 0 — on the reference's own code."""
    assert _ref_pin("H") == 11 * 11 * 8 * 9
    assert _ref_pin("P") == len(ef.P_LENGTHS) * 8 * 41
    assert _ref_pin("Z") == 192 and _ref_pin("Zf") == 192
    assert _ref_pin("S", phase=6) == 547
