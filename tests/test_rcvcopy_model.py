"""The receive copy's model (tests/rcvcopy_model.py) against the reference's own
RBPut (tests/golden/rcvcopy_cases.bin, written by tests/c/ref_rcvcopy_gen.c),
this row's scheme against the literal sequence, the header
(include/mtcp_gpu_rcvcopy.h), the workspace size, and the kernels' step
functions and width rule compiled for the host (tools/librcvcopy_pattern.so).
All on the CPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from mtcp_amd._types import RCV_BUF_DTYPE, RCV_COPY, RCVCOPY_STATS, RCVCOPY_WAVE_LEN
from tests import group_model as gm
from tests import rcvcopy_gen as rg
from tests import rcvcopy_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return cm.load_golden()


def replay(golden, fn):
    """Every case of the fixture batch by batch: fn(case number, family, ring,
    packets as (put_off, payload), the fixture's state behind the batch)."""
    for c, (fam, size, batches) in enumerate(golden):
        rb = cm.Ring(np.full(size, cm.FILL, np.uint8))
        head_seq, serial = 0, 0
        for removed, pk, want, frags, data in batches:
            cm.remove(rb, removed)
            head_seq += removed
            pkts = []
            for off, ln, ret in pk:
                if ret > 0:
                    assert ret == ln and 0 <= off - head_seq and off - head_seq + ln <= size
                    pkts.append((off - head_seq, cm.payload_bytes(c, serial, ln)))
                serial += 1
            assert head_seq == want[3]
            fn(c, fam, rb, pkts, want, data)


# ---- the literal model against the reference ---------------------------------------------------------
def test_literal_model_equals_the_references_chunk_and_offsets(golden):
    seen = {"batches": 0, "moves": 0}

    def check(c, fam, rb, pkts, want, data):
        for off, b in pkts:
            seen["moves"] += cm.put(rb, off, b)
        assert rb.offsets() == want[:3], (c, fam)
        assert rb.data.tobytes() == data.tobytes(), (c, fam)
        seen["batches"] += 1
    replay(golden, check)
    assert seen["batches"] > 200 and seen["moves"] >= 20


def test_fixture_holds_every_family(golden):
    fams = {f for f, _, _ in golden}
    assert fams == {0, 1, 2, 3, 4} and {s for _, s, _ in golden} == {256, 512, 1024, 2048}
    got = {"ordered": 0, "exact": 0, "delayed": 0, "heads": set()}

    def look(c, fam, rb, pkts, want, data):
        head = rb.head
        cls, M, trig = cm.plan(rb.size, head, [(o, len(b)) for o, b in pkts])
        got["ordered"] += cls.count(cm.ORDERED) if fam == 2 else 0
        got["delayed"] += cls.count(cm.ORDERED) == 0 and any(pkts[k][0] > pkts[k + 1][0] for k in range(len(pkts) - 1))
        got["exact"] += fam == 3 and head == 0 and M == rb.size
        if fam == 4 and trig and head:
            got["heads"].add(head if head != rb.size - 1 else -1)
        for off, b in pkts:
            cm.put(rb, off, b)
    replay(golden, look)
    assert got["ordered"] >= 20 and got["exact"] >= 4 and got["heads"] >= {1, 15, 16, 17, -1}, got
    assert os.path.getsize(cm.GOLDEN) < (1 << 20)


# ---- the scheme against the literal sequence -----------------------------------------------------------
def hold_guarantees(lit, sch, compacted, last_before, pkts, what):
    assert sch.offsets() == lit.offsets(), what                                        # 1
    if not compacted:
        assert sch.data.tobytes() == lit.data.tobytes(), what                          # 3
        return
    m = cm.live_mask(lit.size, lit.head, last_before, [(o, len(b)) for o, b in pkts])
    assert (sch.data[m] == lit.data[m]).all(), what                                    # 2 (4: the rest is free)


def test_scheme_meets_the_guarantees_on_the_fixture(golden):
    rng = np.random.default_rng(5)
    twin = {}

    def check(c, fam, rb, pkts, want, data):
        sch = twin.setdefault(c, cm.Ring(np.full(rb.size, cm.FILL, np.uint8)))
        sch.head, sch.tail, sch.last = rb.offsets()    # as the caller refreshes the record after RBRemove
        sch.data[:] = rb.data                          # (and the model restarts from the reference's bytes)
        last_before = rb.last
        for off, b in pkts:
            cm.put(rb, off, b)
        cls, compacted = cm.scheme(sch, pkts, rng)
        hold_guarantees(rb, sch, compacted, last_before, pkts, (c, fam))
    replay(golden, check)


def random_stream(rng):
    size = int(rng.choice([64, 100, 256, 777]))
    head = int(rng.integers(0, size + 1)) if rng.random() < 0.8 else 0
    last = int(rng.integers(0, size - head + 1))
    data = rng.integers(0, 256, size, dtype=np.uint8)
    pkts = []
    for _ in range(int(rng.integers(0, 12))):
        ln = int(rng.integers(1, 60))
        if ln > size:
            continue
        off = int(rng.integers(0, size - ln + 1)) if rng.random() < 0.85 else size - ln
        pkts.append((off, rng.integers(0, 256, ln, dtype=np.uint8)))
    return data, head, last, pkts


def test_scheme_meets_the_guarantees_on_seeded_random_streams():
    rng = np.random.default_rng(12)
    compactions = ordered = 0
    for k in range(4000):
        data, head, last, pkts = random_stream(rng)
        lit, sch = cm.Ring(data.copy(), head, head + last, last), cm.Ring(data.copy(), head, head + last, last)
        for off, b in pkts:
            cm.put(lit, off, b)
        cls, compacted = cm.scheme(sch, pkts, rng)
        compactions += compacted
        ordered += cls.count(cm.ORDERED)
        hold_guarantees(lit, sch, compacted, last, pkts, k)
    assert compactions > 500 and ordered > 3000


# ---- the header --------------------------------------------------------------------------------------
def test_header_layouts_offsets_and_citations():
    hdr = open(os.path.join(ROOT, "include", "mtcp_gpu_rcvcopy.h")).read()
    assert re.search(r"#define MTCP_GPU_HAS_RCVCOPY\s+1\b", hdr)
    assert re.search(r"#define MTCP_GPU_RCVCOPY_WAVE_LEN\s+%d\b" % RCVCOPY_WAVE_LEN, hdr)
    assert "MTCP_GPU_ABI_VERSION" in hdr and "extern \"C\"" in hdr and "#define MTCP_GPU_ABI_VERSION" not in hdr
    body = re.search(r"typedef struct mtcp_gpu_rcv_buf \{(.*?)\} mtcp_gpu_rcv_buf;", hdr, re.S).group(1)
    fields = re.findall(r"(\w+)(?:\[\w+\])?;\s*/\*\s*(\d+) ", body)
    assert [(f, int(o)) for f, o in fields] == [(f, RCV_BUF_DTYPE.fields[f][1]) for f in RCV_BUF_DTYPE.names]
    assert RCV_BUF_DTYPE.itemsize == 32
    for k, v in enumerate(RCVCOPY_STATS):
        assert re.search(r"MTCP_GPU_RCVCOPY_%s\s*=\s*%d\b" % (v, k), hdr), v
    assert (cm.NONE, cm.FRONT, cm.ORDERED, cm.BAD_BUF, cm.BAD_SRC, cm.BAD_RANGE) == tuple(range(6))
    pieces = [hdr[:hdr.index("#ifndef")]]
    for fn in ("mtcp_gpu_rcvcopy_work_bytes", "mtcp_gpu_rcvcopy_dev"):
        at = re.search(r"\b%s\(" % fn, re.sub(r"/\*.*?\*/", lambda m: " " * len(m.group(0)), hdr, flags=re.S)).start()
        pieces.append(hdr[hdr.rindex("/*", 0, at):at])
    for text in pieces:
        assert "tcp_ring_buffer.c:304-319" in " ".join(text.replace("*", " ").split()), text[:60]
    assert "no host-memory form" in " ".join(pieces[0].replace("*", " ").split())
    walk = open(os.path.join(ROOT, "include", "mtcp_gpu_rcvwalk.h")).read()
    assert re.search(r"#define MTCP_GPU_RCV_COPY\s+0x%02xu" % RCV_COPY, walk)


def test_work_bytes_is_monotonic_and_zero_only_above_the_limits():
    from mtcp_amd import gpu
    wb = gpu.Context.rcvcopy_work_bytes
    ns = [0, 1, 2, 63, 64, 65, 4095, 4096, 4097, 1 << 20, (1 << 26) - 1, 1 << 26]
    ids = [0, 1, 255, 65535, 1 << 20, gm.MAX_ID - 1, gm.MAX_ID]
    grid = [[wb(n, i) for i in ids] for n in ns]
    assert all(v > 0 and v % 16 == 0 for row in grid for v in row)
    assert all(grid[a][c] <= grid[a + 1][c] for a in range(len(ns) - 1) for c in range(len(ids)))
    assert all(grid[a][c] <= grid[a][c + 1] for a in range(len(ns)) for c in range(len(ids) - 1))
    assert wb((1 << 26) + 1, 5) == 0 and wb(5, gm.MAX_ID + 1) == 0 and wb(5, gm.FLOW_NONE) == 0


# ---- the kernels' step functions and the width rule, compiled for the host -----------------------------
@pytest.fixture(scope="module")
def P():
    lib = ctypes.CDLL(os.path.join(ROOT, "tools", "librcvcopy_pattern.so"))
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    lib.rcvcopy_host_plan.argtypes = [vp, vp, vp, u32, u64, u32, u32, vp, vp, vp, u32, vp, vp, u64, vp, vp]
    lib.rcvcopy_host_plan.restype = None
    lib.rcvcopy_group_of.argtypes = [u64, u32]
    lib.rcvcopy_group_of.restype = ctypes.c_int
    return lib


def test_width_rule(P):
    """Eight lanes up to an average slot of 512 B, half a wave above; n = 0 is
    the narrow one."""
    g = P.rcvcopy_group_of
    assert [g(n * s, n) for n, s in ((1, 64), (4096, 256), (7, 512))] == [8, 8, 8]
    assert [g(n * s, n) for n, s in ((1, 513), (4096, 2048), (3, 9216))] == [32, 32, 32]
    assert g(513 * 4096 - 1, 4096) == 8 and g(513 * 4096, 4096) == 32 and g(0, 0) == 8 and g(1 << 40, 1) == 32
    src = open(os.path.join(ROOT, "mtcp_amd", "csrc", "mtcp_gpu.hip")).read()
    assert set(re.findall(r"rcvcopy_front_kernel<(\d+)>", src)) == {"8", "32"}


def host_plan(P, b):
    idx, seg_sid, seg_start = b["group"]
    n, m = len(b["res"]), len(seg_sid)
    rbuf, cstat, moved = b["rbuf"].copy(), np.full(n, 0xA5, np.uint8), np.zeros(max(m, 1), np.uint8)
    arrs = [np.ascontiguousarray(a) for a in (b["res"], b["place"], b["desc"], idx, seg_sid, seg_start, b["seg_stop"])]
    P.rcvcopy_host_plan(arrs[0].ctypes.data, arrs[1].ctypes.data, arrs[2].ctypes.data, b["off_shift"], len(b["buf"]),
                        n, b["max_id"], arrs[3].ctypes.data, arrs[4].ctypes.data, arrs[5].ctypes.data, m,
                        arrs[6].ctypes.data, rbuf.ctypes.data, len(b["arena"]), cstat.ctypes.data, moved.ctypes.data)
    return rbuf, cstat, int(moved.sum())


def model_of(b):
    return cm.copy(b["buf"], b["desc"], b["off_shift"], b["res"], b["place"], b["max_id"], *b["group"], b["seg_stop"],
                   b["rbuf"], b["arena"])


@pytest.mark.parametrize("garbage", [False, True])
def test_host_compiled_plan_matches_the_model(P, garbage):
    rng = np.random.default_rng(31 + garbage)
    counts = np.zeros(6, np.int64)
    for _ in range(6):
        b = rg.random_batch(rng, 150, garbage)
        _, w_rbuf, w_cstat, _, info = model_of(b)
        rbuf, cstat, moved = host_plan(P, b)
        bad = np.nonzero(cstat != w_cstat)[0]
        assert len(bad) == 0, (bad[:5], cstat[bad[:5]], w_cstat[bad[:5]])
        assert rbuf.tobytes() == w_rbuf.tobytes()
        assert moved == info["compacted"]
        counts += info["classes"]
    if garbage:                                        # few records of random bytes hold a packet of random bytes
        assert counts[cm.BAD_BUF] > 1000 and counts[cm.BAD_RANGE] > 100 and counts[cm.FRONT] > 10, counts.tolist()
    else:
        assert (counts > 20).all(), counts.tolist()
