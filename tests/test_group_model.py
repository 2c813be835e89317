"""The group model (tests/group_model.py) against a plain loop, the header's
constants and the host-only sizing calls (no GPU)."""
import os
import re

import numpy as np

from tests import flowtab_model as fm
from tests import group_model as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def plain(sid, max_id):
    """Append i to the list of its class, then emit the classes in order."""
    lists = {}
    for i, s in enumerate(int(x) for x in sid):
        c = (0, s) if s <= max_id else (1, gm.FLOW_MISS) if s == gm.FLOW_MISS else (2, gm.FLOW_NONE)
        lists.setdefault(c, []).append(i)
    idx, seg_sid, seg_start = [], [], []
    for c in sorted(lists):
        seg_sid.append(c[1])
        seg_start.append(len(idx))
        idx += lists[c]
    return idx, seg_sid, seg_start + [len(idx)]


def random_input(rng):
    """n and max_id from a few regimes, values drawn so that classes are empty,
    full, MISS, NONE and above max_id."""
    n = int(rng.choice([1, 2, 7, 64, 300]))
    max_id = int(rng.choice([0, 1, 2, 5, 255, 256, 70000, gm.MAX_ID]))
    pool = np.array([0, min(1, max_id), max_id, min(max_id + 1, 0xFFFFFFFF), min(max_id + 7, 0xFFFFFFFF),
                     gm.FLOW_MISS, gm.FLOW_NONE, gm.MAX_ID + 1], dtype=np.uint64)
    sid = np.where(rng.random(n) < 0.5, rng.integers(0, min(max_id, 40) + 3, n, dtype=np.uint64),
                   pool[rng.integers(0, len(pool), n)])
    keep = rng.random(len(pool)) < 0.7                        # some of the special values never occur
    sid = np.where(np.isin(sid, pool[~keep]), 0, sid)
    return sid.astype(np.uint32), max_id


def test_model_equals_a_plain_loop_on_1000_random_inputs():
    rng = np.random.default_rng(2026)
    seen_none_above, seen_max0, seen_missing = 0, 0, 0
    for _ in range(1000):
        sid, max_id = random_input(rng)
        idx, seg_sid, seg_start = gm.group(sid, max_id)
        assert idx.dtype == seg_sid.dtype == seg_start.dtype == np.uint32
        want = plain(sid, max_id)
        assert (idx.tolist(), seg_sid.tolist(), seg_start.tolist()) == want, (sid, max_id)
        assert len(seg_start) == len(seg_sid) + 1 and seg_start[-1] == len(sid)
        above = (sid > max_id) & (sid != gm.FLOW_MISS) & (sid != gm.FLOW_NONE)
        seen_none_above += bool(above.any())
        seen_max0 += max_id == 0
        seen_missing += len(seg_sid) < min(len(sid), max_id + 3)
    assert seen_none_above > 100 and seen_max0 > 50 and seen_missing > 100


def test_header_constants():
    hdr = open(os.path.join(ROOT, "include", "mtcp_gpu_group.h")).read()
    assert re.search(r"#define\s+MTCP_GPU_HAS_GROUP\s+1\b", hdr)
    m = re.search(r"#define\s+MTCP_GPU_GROUP_MAX_PKTS\s+\(1u << (\d+)\)", hdr)
    assert m and 1 << int(m.group(1)) == gm.GROUP_MAX_PKTS
    assert (gm.FLOW_MISS, gm.FLOW_NONE, gm.MAX_ID) == (fm.FLOW_MISS, fm.FLOW_NONE, fm.MAX_ID)
    for cite in ("core.c:768-777", "tcp_in.c:1181-1186"):
        assert hdr.count(cite) >= 5, cite                     # the head comment and every entry point


def test_tile_and_work_bytes():
    from mtcp_amd import gpu
    T = gpu.Context.group_tile()
    assert T > 0
    wb = gpu.Context.group_work_bytes
    # 0 exactly for the out-of-range arguments
    assert wb(gm.GROUP_MAX_PKTS + 1, 0) == 0 and wb(0xFFFFFFFF, 0) == 0
    assert wb(1, gm.MAX_ID + 1) == 0 and wb(1, 0xFFFFFFFF) == 0
    ns = [0, 1, T - 1, T, T + 1, 2 * T, 2 * T + 5, 17 * T + 5, 1 << 20, gm.GROUP_MAX_PKTS]
    ids = sorted({0, gm.MAX_ID} | {v for k in range(1, 33) for v in (2 ** k - 2, 2 ** k - 1, 2 ** k)
                                   if v <= gm.MAX_ID})
    table = np.array([[wb(n, i) for i in ids] for n in ns], dtype=np.uint64)
    assert (table[1:] > 0).all()                              # (0 is allowed at n <= T; it is not used)
    assert (np.diff(table.astype(np.int64), axis=0) >= 0).all(), "not non-decreasing in n"
    assert (np.diff(table.astype(np.int64), axis=1) >= 0).all(), "not non-decreasing in max_id"
    assert (table % 16 == 0).all()
