"""The steer model (tests/steer_model.py) against a plain loop, its
destination rule case by case, and the header's constants (no GPU)."""
import os
import re

import numpy as np
import pytest

from mtcp_amd import RESULT16_DTYPE, RESULT_DTYPE
from mtcp_amd import _types
from tests import steer_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROP_VERDICTS = {4, 9, 10, 11, 12, 13, 14, 15}


def random_records(dtype, n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, n * dtype.itemsize, dtype=np.uint8).view(dtype)


@pytest.mark.parametrize("dtype", [RESULT_DTYPE, RESULT16_DTYPE], ids=["40B", "16B"])
@pytest.mark.parametrize("flags", [0, sm.STEER_DROP_BAD])
@pytest.mark.parametrize("Q", [1, 3, 16, 128])
def test_model_equals_a_plain_loop(Q, flags, dtype):
    res = random_records(dtype, 3000, 17 * Q + flags)
    res["verdict"] &= 15
    lists = [[] for _ in range(Q + 1)]
    for i in range(len(res)):
        v, q = int(res["verdict"][i]), int(res["rss_queue"][i])
        d = q
        if q >= Q or (flags & sm.STEER_DROP_BAD and v in DROP_VERDICTS):
            d = Q
        lists[d].append(i)
    idx, start = sm.steer(res, Q, flags)
    assert idx.dtype == np.uint32 and start.dtype == np.uint32
    assert len(start) == Q + 2 and start[0] == 0 and start[Q + 1] == len(res)
    for l in range(Q + 1):
        assert idx[start[l]:start[l + 1]].tolist() == lists[l], l
    assert any(lists[Q]) and any(lists[0])


@pytest.mark.parametrize("dtype", [RESULT_DTYPE, RESULT16_DTYPE], ids=["40B", "16B"])
@pytest.mark.parametrize("Q", [1, 3, 16, 128])
def test_destination_rule_case_by_case(Q, dtype):
    for verdict in range(16):
        for queue in (0, Q - 1, Q, 255):
            r = np.zeros(1, dtype)
            r["verdict"], r["rss_queue"] = verdict, queue
            plain = Q if queue >= Q else queue
            assert sm.dest(r, Q, 0)[0] == plain, (verdict, queue)
            drop = Q if (queue >= Q or verdict in DROP_VERDICTS) else queue
            assert sm.dest(r, Q, sm.STEER_DROP_BAD)[0] == drop, (verdict, queue)


def test_verdict_above_15_is_dropped_and_high_queue_is_rest():
    r = np.zeros(2, RESULT_DTYPE)
    r["verdict"] = [200, 0]
    r["rss_queue"] = [0, 128]
    assert sm.dest(r, 128, sm.STEER_DROP_BAD).tolist() == [128, 128]
    assert sm.dest(r, 128, 0).tolist() == [0, 128]


def test_header_constants():
    hdr = open(os.path.join(ROOT, "include", "mtcp_gpu_steer.h")).read()

    def macro(name):
        m = re.search(r"#define\s+%s\s+(\(1u << (\d+)\)|0x[0-9a-fA-F]+u?|\d+u?)" % name, hdr)
        assert m, name
        return 1 << int(m.group(2)) if m.group(2) else int(m.group(1).rstrip("u"), 0)

    assert macro("MTCP_GPU_HAS_STEER") == 1
    assert macro("MTCP_GPU_STEER_MAX_QUEUES") == sm.STEER_MAX_QUEUES == _types.STEER_MAX_QUEUES == 128
    assert macro("MTCP_GPU_STEER_MAX_PKTS") == sm.STEER_MAX_PKTS == _types.STEER_MAX_PKTS
    assert macro("MTCP_GPU_STEER_DROP_BAD") == sm.STEER_DROP_BAD == _types.STEER_DROP_BAD
    import mtcp_amd
    assert mtcp_amd.STEER_DROP_BAD == 1
    # the verdict values the rule names
    main = open(os.path.join(ROOT, "include", "mtcp_gpu.h")).read()
    for name, v in (("IP_CSUM_BAD", sm.V_IP_CSUM_BAD), ("TCP_CSUM_BAD", sm.V_TCP_CSUM_BAD),
                    ("TRUNCATED", sm.V_TRUNCATED), ("BAD_DESC", sm.V_BAD_DESC)):
        assert re.search(r"MTCP_GPU_V_%s\s*=\s*%d\b" % (name, v), main), name
