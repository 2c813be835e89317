"""A literal restatement of the reference's flow table (mtcp/src/fhash.c) as
the yardstick of the device flow table (include/mtcp_gpu_flowtab.h).

No open addressing and no code shared with the library: NUM_BINS_FLOWS
(fhash.h:7) Python lists stand for the TAILQ bins, HashFlow
(tcp_stream.c:56-90) comes from the oracle (tests/golden/flow_cases.bin pins
it), and EqualFlow (tcp_stream.c:92-102) is the comparison of the 12 key
bytes.

  insert   StreamHTInsert, fhash.c:68-87: TAILQ_INSERT_TAIL into the key's bin
  remove   StreamHTRemove, fhash.c:89-101: the item leaves its bin.  The
           reference removes by pointer; here the item with that key and id
  search   StreamHTSearch, fhash.c:103-121: walk the bin HashFlow names, the
           FIRST item with an equal key
  lowest   the device table's contract: the LOWEST id among the items with an
           equal key

The two agree on every table that holds no key twice, which is every table
the reference builds (tests/test_flowtab_model.py).
"""
import numpy as np

import oracle

NUM_BINS_FLOWS = 131072           # fhash.h:7
FLOW_NONE = 0xFFFFFFFF
FLOW_MISS = 0xFFFFFFFE
MAX_ID = 0xFFFFFFEF
V_TCP_OK = 0

ENTRY_DTYPE = np.dtype([("saddr", "<u4"), ("daddr", "<u4"), ("sport", "<u2"), ("dport", "<u2"), ("id", "<u4")])


def entry_key(e) -> bytes:
    """The 12 key bytes of one entry record."""
    return bytes(np.asarray(e).reshape(1).view(np.uint8)[:12])


def record_keys(res: np.ndarray) -> np.ndarray:
    """The stream key of every rx record, n x 12 bytes (tcp_in.c:1180-1186:
    saddr = iph->daddr, daddr = iph->saddr, sport = tcph->dest, dport =
    tcph->source)."""
    k = np.zeros(len(res), dtype=ENTRY_DTYPE)
    k["saddr"], k["daddr"], k["sport"], k["dport"] = res["daddr"], res["saddr"], res["dport"], res["sport"]
    return k.view(np.uint8).reshape(len(res), 16)[:, :12]


def entries(keys: np.ndarray, ids) -> np.ndarray:
    """Entry records from n x 12 key bytes and n ids."""
    e = np.zeros(len(keys), dtype=ENTRY_DTYPE)
    e.view(np.uint8).reshape(len(keys), 16)[:, :12] = keys
    e["id"] = ids
    return e


class FlowTable:
    def __init__(self):
        self.bins = [[] for _ in range(NUM_BINS_FLOWS)]
        self.count = 0
        self.remove_missed = 0
        self.used = set()                                         # bins that ever held an item

    def clear(self) -> None:
        """An empty table again (building the 131 072 lists anew costs 0.1 s)."""
        for b in self.used:
            self.bins[b].clear()
        self.used.clear()
        self.count = self.remove_missed = 0

    def insert(self, key: bytes, sid: int) -> None:
        b = oracle.hash_flow(key)
        self.bins[b].append((key, sid))                           # TAILQ_INSERT_TAIL
        self.used.add(b)
        self.count += 1

    def remove(self, key: bytes, sid: int) -> bool:
        b = self.bins[oracle.hash_flow(key)]
        for i, item in enumerate(b):
            if item == (key, sid):
                del b[i]                                          # TAILQ_REMOVE
                self.count -= 1
                return True
        self.remove_missed += 1
        return False

    def search(self, key: bytes) -> int:
        """StreamHTSearch: the first item with an equal key, or FLOW_MISS."""
        for k, sid in self.bins[oracle.hash_flow(key)]:
            if k == key:                                          # EqualFlow
                return sid
        return FLOW_MISS

    def lowest(self, key: bytes) -> int:
        """The device table's contract: the lowest id under an equal key."""
        ids = [sid for k, sid in self.bins[oracle.hash_flow(key)] if k == key]
        return min(ids) if ids else FLOW_MISS

    # -- batches ---------------------------------------------------------------
    def update(self, dele=(), ins=()) -> None:
        """One mtcp_gpu_flowtab_update: every remove, then every insert."""
        for e in dele:
            self.remove(entry_key(e), int(e["id"]))
        for e in ins:
            self.insert(entry_key(e), int(e["id"]))

    def lookup(self, res: np.ndarray, rule: str = "lowest") -> np.ndarray:
        """One answer per rx record: FLOW_NONE unless the verdict is TCP_OK.
        Every distinct key is searched once."""
        find = self.lowest if rule == "lowest" else self.search
        out = np.full(len(res), FLOW_NONE, dtype=np.uint32)
        ok = np.nonzero(res["verdict"] == V_TCP_OK)[0]
        if len(ok) == 0:
            return out
        keys = record_keys(res[ok])
        uniq, inv = np.unique(keys, axis=0, return_inverse=True)
        ans = np.array([find(bytes(k)) for k in uniq], dtype=np.uint32)
        out[ok] = ans[inv.reshape(-1)]
        return out

    def has_duplicate_keys(self) -> bool:
        return any(len({k for k, _ in self.bins[b]}) != len(self.bins[b]) for b in self.used)
