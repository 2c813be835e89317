"""CPU checks of the device flow table's yardstick (tests/flowtab_model.py,
the restatement of mtcp/src/fhash.c) and of mtcp_gpu_flowtab_home, which is
host code and needs no GPU.

The model's bins are the golden HashFlow values; its first-match search
(StreamHTSearch) and the device table's lowest-id contract agree on every
table without duplicate keys and differ exactly where duplicate keys were
inserted with descending ids."""
import os

import numpy as np

import oracle
from tests import flowtab_model as fm

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def home(key: bytes, cap_log2: int) -> int:
    from mtcp_amd import gpu
    return gpu.FlowTable.home(key, cap_log2)


def test_every_golden_key_lands_in_its_golden_bin(golden):
    t = fm.FlowTable()
    c = golden.flow_cases
    for i, k in enumerate(c["key"]):
        t.insert(bytes(k), i)
    for i, (k, h) in enumerate(zip(c["key"], c["hash"])):
        assert (bytes(k), i) in t.bins[int(h)], i
    assert t.count == len(c) == sum(len(b) for b in t.bins)


def test_golden_rx_keys_every_second_distinct_key_hits(golden):
    """The keys the reference handed to StreamHTSearch for the golden rx
    frames (rx_flowkey.bin) and the bins it computed (rx_flowbins.bin): a
    table built from every second distinct key hits exactly those, in the
    golden bin."""
    keys = np.fromfile(os.path.join(GOLD, "rx_flowkey.bin"), dtype=np.uint8).reshape(-1, 12)
    tcp = (golden.meta["ref_ub"] == 0) & (golden.expect["verdict"] == 0)
    assert tcp.sum() > 100
    assert np.array_equal(fm.record_keys(golden.expect)[tcp], keys[tcp])       # the records carry the same key
    distinct = sorted({bytes(k) for k in keys[tcp]})
    held = {k: i for i, k in enumerate(distinct[::2])}
    assert len(held) > 10 and len(held) < len(distinct)
    t = fm.FlowTable()
    for k, i in held.items():
        t.insert(k, i)
    for f in np.nonzero(tcp)[0]:
        k = bytes(keys[f])
        assert (k, held[k]) in t.bins[int(golden.flow_bins[f])] if k in held else True
        assert t.search(k) == t.lowest(k) == held.get(k, fm.FLOW_MISS)
    got = t.lookup(golden.expect)
    want = np.array([held.get(bytes(k), fm.FLOW_MISS) for k in keys], dtype=np.uint32)
    assert np.array_equal(got[tcp], want[tcp])
    assert (got[golden.expect["verdict"] != 0] == fm.FLOW_NONE).all()


def test_first_match_equals_lowest_id_without_duplicate_keys():
    """1 000 random insert / remove sequences that never hold a key twice,
    with keys crowded into few bins' worth of values and ids in random order."""
    rng = np.random.default_rng(9)
    t = fm.FlowTable()
    for seq in range(1000):
        t.clear()
        pool = [bytes(rng.integers(0, 4, 12, dtype=np.uint8)) for _ in range(12)]
        held = {}
        for step in range(30):
            k = pool[int(rng.integers(len(pool)))]
            if k in held and rng.random() < 0.6:
                assert t.remove(k, held.pop(k))
            elif k not in held:
                held[k] = int(rng.integers(0, fm.MAX_ID + 1))
                t.insert(k, held[k])
        assert not t.has_duplicate_keys() and t.count == len(held)
        for k in pool:
            assert t.search(k) == t.lowest(k) == held.get(k, fm.FLOW_MISS), (seq, k)


def test_duplicate_keys_differ_exactly_where_ids_descend():
    rng = np.random.default_rng(10)
    differ = same = 0
    t = fm.FlowTable()
    for seq in range(300):
        t.clear()
        k = bytes(rng.integers(0, 256, 12, dtype=np.uint8))
        ids = [int(x) for x in rng.choice(1000, size=int(rng.integers(2, 5)), replace=False)]
        for i in ids:
            t.insert(k, i)
        assert t.has_duplicate_keys()
        assert t.search(k) == ids[0] and t.lowest(k) == min(ids)
        # first-inserted is the lowest unless a later insert carried a lower id
        assert (t.search(k) != t.lowest(k)) == (min(ids) != ids[0])
        differ += t.search(k) != t.lowest(k)
        same += t.search(k) == t.lowest(k)
        # a remove of the first item moves the first match on; the lowest id follows the multiset
        t.remove(k, ids[0])
        assert t.search(k) == ids[1] and t.lowest(k) == min(ids[1:])
    assert differ > 50 and same > 50


def test_remove_takes_key_and_id():
    t = fm.FlowTable()
    k = bytes(range(12))
    t.insert(k, 5)
    assert not t.remove(k, 6) and t.remove_missed == 1 and t.search(k) == 5
    assert t.remove(k, 5) and t.search(k) == fm.FLOW_MISS and t.count == 0
    assert not t.remove(k, 5) and t.remove_missed == 2


# ---- mtcp_gpu_flowtab_home: host code of the library, no GPU -----------------------
def test_home_stays_below_cap(golden):
    rng = np.random.default_rng(11)
    keys = [bytes(k) for k in golden.flow_cases["key"][:200]]
    keys += [bytes(rng.integers(0, 256, 12, dtype=np.uint8)) for _ in range(200)]
    for cap_log2 in range(4, 27):
        homes = [home(k, cap_log2) for k in keys]
        assert max(homes) < (1 << cap_log2)
        if cap_log2 <= 6:
            assert len(set(homes)) == 1 << cap_log2           # every slot is some key's home
    for bad in (0, 3, 27, 32):
        assert home(keys[0], bad) == 0xFFFFFFFF
    from mtcp_amd._lib import lib
    assert lib().mtcp_gpu_flowtab_home(None, 10) == 0xFFFFFFFF


def test_home_low_bits_are_the_golden_bin(golden):
    """home = HashFlow's unmasked Jenkins value & (cap - 1): from 2^17 slots on
    its low 17 bits are the pinned bin, below that it is the bin's low bits,
    and a larger table's home extends a smaller one's."""
    c = golden.flow_cases
    for k, h in zip(c["key"], c["hash"]):
        k, h = bytes(k), int(h)
        assert oracle.hash_flow(k) == h
        for cap_log2 in (17, 18, 21, 26):
            assert home(k, cap_log2) & (fm.NUM_BINS_FLOWS - 1) == h
        for cap_log2 in (4, 10, 16):
            assert home(k, cap_log2) == h & ((1 << cap_log2) - 1)
        assert home(k, 26) & ((1 << 21) - 1) == home(k, 21)
    top = {home(bytes(k), 26) >> 17 for k in c["key"]}
    assert len(top) > min(len(c), 512) // 4                  # the bits above the bin vary too
