"""tests/datagen_model.py against the reference: tests/golden/datagen_cases.bin
holds, per case, 1-8 streams before, their send buffers' bytes, cur_ts, a slot
budget, ret, the frames the reference's own WriteTCPDataList,
FlushTCPSendingBuffer, SendTCPPacket, IPOutput and EthernetOutput wrote, and the
streams after (tests/c/ref_datagen_gen.c).  The model must give the same streams,
the same ret and, through tests/txseg_model.py and tests/txbuild_model.py, the
same frames byte for byte; its bursts through the library's host plan
(mtcp_gpu_tx_segment_plan) must give the fixture's counts; the last-flag-wins
fold is held to a plain loop.  No GPU."""
import numpy as np

from mtcp_amd._lib import lib
from tests import ackgen_model as am
from tests import datagen_model as dm
from tests import txbuild_model as xm
from tests import txseg_model as sm

CASES = dm.load_fixture()
LINKS = am.fixture_links()


def test_fixture_has_every_family():
    fam = np.bincount([c["family"] for c in CASES], minlength=len(dm.FAMILIES))
    assert len(fam) == len(dm.FAMILIES) and (fam > 0).all(), dict(zip(dm.FAMILIES, fam))
    S = [s for c in CASES for s in c["streams"]]
    assert {13, 14, 64, 536, 1460} <= {s["before"]["mss"] for s in S}
    assert {-1, -2, -3, 0, 1, dm.NOT_SERVED} <= {s["ret"] for s in S}
    assert any(s["wack_enqueued"] for s in S) and any(s["rto_added"] for s in S)
    assert any(s["ret"] == -3 and s["frames"] for s in S) and any(s["ret"] == -3 and not s["frames"] for s in S)
    assert any(s["ret"] == -2 and s["frames"] for s in S) and any(s["ret"] == -2 and not s["frames"] for s in S)
    assert any(s["after"]["ip_id"] < s["before"]["ip_id"] for s in S)                    # ip_id wrapped
    assert any(s["after"]["snd_nxt"] < s["before"]["snd_nxt"] for s in S)                # seq wrapped
    assert any(s["after"]["need_wnd_adv"] > s["before"]["need_wnd_adv"] for s in S)
    assert {0, 1} == {s["before"]["on_rto"] for s in S} and all(s["before"]["arena_off"] & 1 for s in S)
    assert {2, 3, 4, 5, 6, 7, 8} == {len(c["streams"]) for c in CASES if c["family"] == 11}
    d = [(c["cur_ts"] - c["streams"][0]["before"]["ts_lastack_sent"]) & dm.M32 for c in CASES if c["family"] == 2]
    assert {499, 500, 501, 4294968, 4295468, 4295469} <= set(d)


def test_model_equals_the_reference():
    for i, c in enumerate(CASES):
        b = dm.case_batch(c)
        seg, desc, dres, total, snd, tx, dtx, _ = dm.run_batch(b)
        image = np.zeros(max(b["buf_len"], 1), np.uint8)
        image, status = xm.build_frames(seg, b["payload"], LINKS, desc, image)
        k = 0
        for j, s in enumerate(c["streams"]):
            tag = (i, j, dm.FAMILIES[c["family"]])
            assert dm.after_of(j, snd, tx, dtx, s["before"]) == s["after"], tag
            st = int(dres[j]["status"])
            ret = dm.NOT_SERVED if st == dm.IDLE else int(dres[j]["n_seg"]) if st == dm.SENT else dm.RET[st]
            assert ret == s["ret"], (tag, dm.FAMILIES[c["family"]], st, ret, s["ret"])
            assert int(dres[j]["n_seg"]) == len(s["frames"]) and int(dres[j]["first_seg"]) == k, tag
            assert bool(dres[j]["flags"] & dm.RTO_ADD) == bool(s["rto_added"]), tag
            assert bool(dres[j]["flags"] & dm.WACK_ENQUEUED) == bool(s["wack_enqueued"]), tag
            for f in s["frames"]:
                assert status[k] == 0 and int(desc[k]["len"]) == len(f), (tag, k)
                at = int(desc[k]["offset"])
                assert image[at:at + len(f)].tobytes() == f.tobytes(), (tag, k)
                k += 1
        assert int(total[0]) == k


def test_bursts_through_the_host_plan_give_the_fixture_counts():
    L = lib()
    for i, c in enumerate(CASES):
        b = dm.case_batch(c)
        bursts = dm.run_batch(b)[7]
        res, total = np.zeros(len(bursts), dtype=sm.RESULT_DTYPE), np.zeros(2, dtype=np.uint64)
        assert L.mtcp_gpu_tx_segment_plan(bursts.ctypes.data, len(bursts), len(b["payload"]), 3, 0, b["buf_len"], 0,
                                          dm.SLOT, b["seg_cap"], 0, res.ctypes.data, total.ctypes.data) == 0
        assert [int(r["n_seg"]) for r in res] == [len(s["frames"]) for s in c["streams"]], i
        assert [int(r["bytes"]) for r in res] == [(s["after"]["snd_nxt"] - s["before"]["snd_nxt"]) & dm.M32
                                                  for s in c["streams"]], i
        assert int(total[0]) == sum(len(s["frames"]) for s in c["streams"])


def fold_masks(on: int, words) -> int:
    """The wave's form: 64 flag words a step, the highest set position of the
    two ballots decides, the add where both have it."""
    for base in range(0, len(words), 64):
        add = rm = 0
        for k, w in enumerate(words[base:base + 64]):
            add |= bool(int(w) & dm.ACK_FAST_RTX) << k
            rm |= bool(int(w) & dm.ACK_SEND_LIST_REMOVE) << k
        if add | rm:
            on = 1 if add.bit_length() >= rm.bit_length() else 0
    return on


def test_fold_equals_a_plain_loop():
    rng = np.random.default_rng(5)
    for trial in range(3000):
        n = int(rng.integers(0, 200))
        words = rng.integers(0, 1 << 16, n)
        if trial % 3:                                                         # sparse flags: most words carry neither
            words &= np.where(rng.random(n) < 0.05, 0xFFFF, 0xFFFF & ~(dm.ACK_FAST_RTX | dm.ACK_SEND_LIST_REMOVE))
        on = trial & 1
        want = on
        for w in words:
            want = 0 if int(w) & dm.ACK_SEND_LIST_REMOVE else want
            want = 1 if int(w) & dm.ACK_FAST_RTX else want
        assert dm.fold(on, words) == want == fold_masks(on, list(words))
