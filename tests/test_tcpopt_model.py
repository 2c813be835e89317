"""SURVEY §8 f5 on the CPU: the Python restatement of ParseTCPTimestamp /
ParseTCPOptions (tests/tcpopt_model.py) against the reference itself and
against the golden fixture the reference wrote (tests/golden/tcpopt_cases.bin),
the fixture's coverage, and the Python view of the new ABI."""
import numpy as np
import pytest

import oracle
from tests import tcpopt_model as m


@pytest.fixture(scope="module")
def cases():
    c = m.load_fixture()
    assert len(c) == m.NCASES
    return c


@pytest.fixture(scope="module")
def walks(cases):
    """(ts walk, syn walk) of the restatement for every fixture case."""
    return [(m.walk_ts(c["bytes"], int(c["len"])), m.walk_syn(c["bytes"], int(c["len"]))) for c in cases]


def test_restatement_equals_live_reference():
    if not oracle.ref_available():
        pytest.skip("oracle/_ref was not built here (needs the reference tree)")
    ref = m.RefWalks()
    called = 0
    for length, b in m.gen_blocks(100_000, seed=77):
        t, s = m.walk_ts(b, length), m.walk_syn(b, length)
        if not t["nonterm"]:                     # the reference would never return from the others
            got = ref.ts_walk(b, length)
            assert got == {k: t[k] for k in m.TS_KEYS}, (length, bytes(b).hex())
            called += 1
        if not s["nonterm"]:
            got = ref.syn_walk(b, length)
            assert got == {k: s[k] for k in m.SYN_KEYS}, (length, bytes(b).hex())
            called += 1
    assert called > 180_000


def test_restatement_equals_fixture(cases, walks):
    for c, (t, s) in zip(cases, walks):
        assert int(c["nonterm"]) == (1 if t["nonterm"] else 0) | (2 if s["nonterm"] else 0)
        if not t["nonterm"]:
            assert (int(c["ts_ret"]), int(c["ts_val"]), int(c["ts_ref"])) == (t["ret"], t["ts_val"], t["ts_ref"])
        else:
            assert (int(c["ts_ret"]), int(c["ts_val"]), int(c["ts_ref"])) == (0, 0, 0)
        for k in m.SYN_KEYS:
            assert int(c[k]) == (0 if s["nonterm"] else s[k]), k
        # the fixture-based expectation is the restatement-based one
        for flags in (0x10, 0x02, 0x12, 0x04, 0x06):
            for avail in (int(c["len"]), int(c["len"]) + 9):
                assert m.record_of_case(c, flags, avail) == m.expected_record(c["bytes"], int(c["len"]), flags, avail)


def test_fixture_coverage(cases, walks):
    n = len(cases)
    assert cases.nbytes < (1 << 20)
    assert set(np.unique(cases["len"])) == set(range(0, 44, 4))
    assert (cases["len"] == 12).mean() > 0.3                      # weighted to 12
    for bit in (1, 2):                                            # endless walks: at most 10 % each
        assert ((cases["nonterm"] & bit) != 0).mean() <= 0.10
    share = {
        "ts_found": (cases["ts_ret"] != 0).mean(),
        "mss": ((cases["seen"] & m.MSS) != 0).mean(),
        "wscale": ((cases["seen"] & m.WSCALE) != 0).mean(),
        "sack_permit": (cases["sack_permit"] != 0).mean(),
        "saw_timestamp": (cases["saw_timestamp"] != 0).mean(),
    }
    for k, v in share.items():
        assert v >= 0.03, (k, v)
    past = sum(1 for c, (t, s) in zip(cases, walks) if c["len"] and max(t["hi"], s["hi"]) >= c["len"])
    assert past / n >= 0.02
    assert max(max(t["hi"], s["hi"]) - int(c["len"]) for c, (t, s) in zip(cases, walks) if c["len"]) == 8


def test_quirks_of_the_reference_walks():
    # a skipped option of length 0: the reference never returns (1e 00 01 01)
    b = np.zeros(m.BLOCK, np.uint8)
    b[:4] = (0x1E, 0, 1, 1)
    assert m.walk_ts(b, 4)["nonterm"] and m.walk_syn(b, 4)["nonterm"]
    b[:4] = (2, 0, 0x05, 0xB4)                   # kind 2 is handled in ParseTCPOptions only
    assert m.walk_ts(b, 4)["nonterm"] and not m.walk_syn(b, 4)["nonterm"]
    assert m.walk_syn(b, 4)["mss"] == 1460
    b[:4] = (0x1E, 1, 0, 0)                      # length 1: the length byte is read again as a NOP
    assert not m.walk_ts(b, 4)["nonterm"]
    # a timestamp whose length byte is 0 at the block's last byte: read to len + 8
    b[:] = 0
    b[:4] = (1, 1, 1, 8)
    t = m.walk_ts(b, 4)
    assert t["ret"] == 1 and t["hi"] == 12
    rec = m.expected_record(b, 4, 0x10, 12)
    assert rec["flags"] == m.TS_UNPINNED
    assert m.expected_record(b, 4, 0x10, 13)["flags"] == m.TS_FOUND


def test_python_view_of_the_option_abi():
    import mtcp_amd
    from mtcp_amd import _lib, gpu
    dt = mtcp_amd.TCPOPT_DTYPE
    assert dt == m.TCPOPT_DTYPE
    assert dt.itemsize == 16 and dt.fields["flags"][1] == 15
    assert dt.fields["ts_recent"][1] == 8 and dt.fields["mss"][1] == 12 and dt.fields["wscale"][1] == 14
    lib = _lib.lib()
    for name in ("mtcp_gpu_rx_tcpopt_chunk_dev", "mtcp_gpu_rx_tcpopt_ptrs_dev", "mtcp_gpu_rx_chunk_opts"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    for meth in ("rx_tcpopt_chunk_dev", "rx_tcpopt_ptrs_dev", "rx_chunk_opts"):
        assert callable(getattr(gpu.Context, meth))
