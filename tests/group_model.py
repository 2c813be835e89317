"""Numpy model of the group step (include/mtcp_gpu_group.h): a stable
partition of a batch by stream id, and its segment table.

The class of a stream id as mtcp_gpu_flowtab_lookup writes it: the stream for a
value up to max_id, MISS for FLOW_MISS, NONE for everything else (FLOW_NONE
and any value above max_id).  Classes come out by ascending stream id, then
MISS, then NONE; indices within a class ascend."""
import numpy as np

FLOW_MISS = 0xFFFFFFFE
FLOW_NONE = 0xFFFFFFFF
MAX_ID = 0xFFFFFFEF
GROUP_MAX_PKTS = 1 << 26


def key(sid: np.ndarray, max_id: int) -> np.ndarray:
    """The sort key of every record: sid, max_id + 1 (MISS) or max_id + 2 (NONE)."""
    s = np.asarray(sid, dtype=np.uint32).astype(np.int64)
    return np.where(s <= max_id, s, np.where(s == FLOW_MISS, max_id + 1, max_id + 2))


def group(sid: np.ndarray, max_id: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(idx[n], seg_sid[m], seg_start[m + 1]) as mtcp_gpu_group writes them."""
    k = key(sid, max_id)
    idx = np.argsort(k, kind="stable").astype(np.uint32)
    ks = k[idx]
    head = np.ones(len(ks), dtype=bool)
    head[1:] = ks[1:] != ks[:-1]
    pos = np.nonzero(head)[0]
    seg = ks[pos]
    seg_sid = np.where(seg <= max_id, seg, np.where(seg == max_id + 1, FLOW_MISS, FLOW_NONE)).astype(np.uint32)
    seg_start = np.append(pos, len(ks)).astype(np.uint32)
    return idx, seg_sid, seg_start
