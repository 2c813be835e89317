"""Numpy model of the steer step (include/mtcp_gpu_steer.h): a stable
partition of rx records by destination list.

Q queues and one rest list (list Q).  A record goes to the rest list when its
rss_queue is Q or more, or, with STEER_DROP_BAD, when its verdict is one for
which an io_module's get_rptr answers NULL (IP_CSUM_BAD, TCP_CSUM_BAD,
TRUNCATED, BAD_DESC) or a value above BAD_DESC; otherwise to the list of its
rss_queue.  Works on RESULT_DTYPE and RESULT16_DTYPE records alike (only
`verdict` and `rss_queue` are read)."""
import numpy as np

STEER_MAX_QUEUES = 128
STEER_MAX_PKTS = 1 << 26
STEER_DROP_BAD = 0x1

V_IP_CSUM_BAD, V_TCP_CSUM_BAD, V_TRUNCATED, V_BAD_DESC = 4, 9, 10, 11


def dest(res: np.ndarray, Q: int, flags: int = 0) -> np.ndarray:
    """The list (0..Q) of every record."""
    verdict = res["verdict"].astype(np.int64)
    queue = res["rss_queue"].astype(np.int64)
    rest = queue >= Q
    if flags & STEER_DROP_BAD:
        rest |= (verdict == V_IP_CSUM_BAD) | (verdict == V_TCP_CSUM_BAD) | (verdict >= V_TRUNCATED)
    return np.where(rest, Q, queue)


def steer(res: np.ndarray, Q: int, flags: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """(idx[n], start[Q + 2]) as mtcp_gpu_steer writes them."""
    d = dest(res, Q, flags)
    idx = np.argsort(d, kind="stable").astype(np.uint32)
    counts = np.bincount(d, minlength=Q + 1)
    start = np.zeros(Q + 2, dtype=np.uint32)
    start[1:] = np.cumsum(counts)
    return idx, start
