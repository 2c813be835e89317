"""The receive copy on the GPU (include/mtcp_gpu_rcvcopy.h,
mtcp_amd/csrc/rcvcopy_kernels.hpp): every arena byte the contract pins, every
d_rbuf record and every d_cstat byte of every case is compared with
tests/rcvcopy_model.py; none is sampled.

The arena's buffers are separated by 64 B guard bands which the model never
writes, the workspace is exactly sized, d_cstat and d_rbuf have guards behind
them.  Every source alignment x destination alignment x length 1-48 and the
lengths around a group pass for both widths, FRONT and ORDERED; the
reference-written fixture through rx, lookup, group and walk; overlaps; list
lengths around the wave and the wave-plan threshold; compaction at every
head_offset of the fixture; bad records and sources, random bytes in the
records; determinism, the error returns and a captured graph."""
import ctypes
import os

import numpy as np
import pytest

import oracle
from mtcp_amd._types import RCV_BUF_DTYPE, RCV_COPY, RCV_PLACE_DTYPE, RCV_STATE_DTYPE, RCVCOPY_WAVE_LEN
from tests import flowtab_model as fm
from tests import group_model as gm
from tests import rcvcopy_gen as rg
from tests import rcvcopy_model as cm
from tests import tcpopt_model as tm

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
EINVAL = -22
GUARD = 4096
SENT = 0xA5
SENT32 = 0xA5A5A5A5
INIT_SEQ = 0xFFFFF000                                  # tests/c/ref_rcvcopy_gen.c


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")
    from mtcp_amd import gpu as g
    return g


@pytest.fixture(scope="module")
def ctx(gpu):
    with gpu.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def width_of():
    lib = ctypes.CDLL(os.path.join(ROOT, "tools", "librcvcopy_pattern.so"))
    lib.rcvcopy_group_of.argtypes = [ctypes.c_uint64, ctypes.c_uint32]
    lib.rcvcopy_group_of.restype = ctypes.c_int
    return lib.rcvcopy_group_of


def to_dev(a: np.ndarray):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)


class Guarded:
    """`nbytes` of device memory holding `fill` and a guard region of SENT behind it."""

    def __init__(self, nbytes, fill=SENT):
        self.nbytes = nbytes
        self.all = torch.full((nbytes + GUARD,), SENT, dtype=torch.uint8, device=DEV)
        self.t = self.all[:nbytes]
        if isinstance(fill, np.ndarray):
            self.t.copy_(to_dev(fill))
        elif fill != SENT:
            self.t.fill_(fill)

    def guard_intact(self):
        return bool((self.all[self.nbytes:] == SENT).all().item())

    def numpy(self, dtype=np.uint8):
        return self.t.cpu().numpy().view(dtype)


class Call:
    """The device arrays of one call on batch b, the outputs guarded."""

    def __init__(self, gpu, b, work_fill=SENT, walked=None):
        self.b, self.n, self.max_id = b, len(b["res"]), b["max_id"]
        n = self.n
        self.buf, self.desc = to_dev(b["buf"]), to_dev(b["desc"])
        if walked is None:
            idx, seg_sid, seg_start = b["group"]
            self.m = len(seg_sid)
            pad = lambda a, k: np.concatenate([a, np.full(k - len(a), SENT32, np.uint32)])
            self.res, self.place = to_dev(b["res"]), to_dev(b["place"])
            self.idx, self.seg_sid = to_dev(idx), to_dev(pad(seg_sid, n))
            self.seg_start, self.nseg = to_dev(pad(seg_start, n + 1)), to_dev(np.array([self.m], np.uint32))
            self.seg_stop = to_dev(pad(b["seg_stop"], n))
        else:
            self.res, self.place, self.idx, self.seg_sid, self.seg_start, self.nseg, self.seg_stop = walked
        self.rbuf = Guarded(32 * (self.max_id + 1), b["rbuf"])
        self.arena = Guarded(len(b["arena"]), b["arena"])
        self.cstat = Guarded(n)
        self.wb = gpu.Context.rcvcopy_work_bytes(n, self.max_id)
        assert self.wb > 0
        self.work = Guarded(self.wb, work_fill)

    def args(self):
        return (self.buf, self.desc, self.b["off_shift"], self.res, self.place, self.n, self.max_id, self.idx,
                self.seg_sid, self.seg_start, self.nseg, self.seg_stop, self.rbuf.t, self.arena.t, self.cstat.t,
                self.work.t)

    def run(self, ctx, stream=None):
        ctx.rcvcopy_dev(*self.args(), stream=stream)

    def reset(self):
        self.rbuf.t.copy_(to_dev(self.b["rbuf"]))
        self.arena.t.copy_(to_dev(self.b["arena"]))
        self.cstat.t.fill_(SENT)

    def raw(self):
        return self.arena.numpy().copy(), self.rbuf.numpy(RCV_BUF_DTYPE).copy(), self.cstat.numpy().copy()

    def check(self, want, what=""):
        for name in ("rbuf", "arena", "cstat", "work"):
            assert getattr(self, name).guard_intact(), f"{what}: bytes behind {name} were written"
        arena, rbuf, cstat = self.raw()
        w_arena, w_rbuf, w_cstat, mask, _ = want
        bad = np.nonzero(cstat != w_cstat)[0]
        assert len(bad) == 0, f"{what}: {len(bad)} of {len(cstat)} status bytes differ, first at {bad[0]}: " \
                              f"{cstat[bad[0]]} want {w_cstat[bad[0]]}"
        bad = np.nonzero(rbuf != w_rbuf)[0]
        assert len(bad) == 0, f"{what}: {len(bad)} records differ, first stream {bad[0]}: {rbuf[bad[0]]} want {w_rbuf[bad[0]]}"
        assert rbuf.tobytes() == w_rbuf.tobytes(), f"{what}: rbuf"
        bad = np.nonzero((arena != w_arena) & mask)[0]
        assert len(bad) == 0, f"{what}: {len(bad)} arena bytes differ, first at {bad[0]}: {arena[bad[0]]} want " \
                              f"{w_arena[bad[0]]} (stream chunks at {self.b['rbuf']['data_off'][:8].tolist()}...)"
        # the bytes of a compacted chunk that are not pinned are free, but nothing outside a chunk moved:
        assert (arena[~chunk_mask(self.b, w_rbuf)] == self.b["arena"][~chunk_mask(self.b, w_rbuf)]).all(), \
            f"{what}: a byte outside every non-BAD chunk changed"


def chunk_mask(b, rbuf):
    m = np.zeros(len(b["arena"]), bool)
    for r in rbuf:
        if not cm.record_bad(r, len(b["arena"])):
            m[int(r["data_off"]):int(r["data_off"]) + int(r["size"])] = True
    return m


def expect(b):
    if "want" not in b:
        b["want"] = cm.copy(b["buf"], b["desc"], b["off_shift"], b["res"], b["place"], b["max_id"], *b["group"],
                            b["seg_stop"], b["rbuf"], b["arena"])
    return b["want"]


def run(gpu, ctx, b, what="", work_fill=SENT):
    want = expect(b)
    c = Call(gpu, b, work_fill)
    c.run(ctx)
    torch.cuda.synchronize()
    c.check(want, what)
    return c


# ---- alignment -------------------------------------------------------------------------------------
def aligned_streams(lengths, order):
    """One stream per (source alignment, destination alignment): its packets
    have the lengths given, each at the next put_off whose address is the
    destination alignment (data_off is 16 B aligned).  order: "front" (list
    order ascending, all FRONT) or "ordered" (descending: all ORDERED but the
    first)."""
    streams = []
    for sa in range(16):
        for da in range(16):
            pk, at = [], 0
            for ln in lengths:
                at += (da - at) & 15
                pk.append((at, ln, sa))
                at += ln
            streams.append({"size": at + 16, "head": 0, "last": 0, "align": 0,
                            "pkts": pk if order == "front" else pk[::-1]})
    return streams


@pytest.mark.parametrize("width", [8, 32])
@pytest.mark.parametrize("order", ["front", "ordered"])
def test_every_alignment_and_short_length(gpu, ctx, width_of, width, order):
    """16 source alignments x 16 destination alignments x lengths 1-48."""
    rng = np.random.default_rng(width + len(order))
    b = rg.build(rng, aligned_streams(range(1, 49), order), width)
    assert width_of(len(b["buf"]), len(b["res"])) == width
    c = run(gpu, ctx, b, f"{order}, width {width}")
    counts = np.bincount(c.raw()[2], minlength=6)
    assert counts[cm.FRONT] == (256 * 48 if order == "front" else 256)
    assert counts[cm.ORDERED] == (0 if order == "front" else 256 * 47)


@pytest.mark.parametrize("width", [8, 32])
def test_lengths_around_a_group_pass_and_full_segments(gpu, ctx, width_of, width):
    """One pass of the group is 16 x width bytes: that length and its
    neighbours, and 1 448, 1 460 and 8 948, at every pair of alignments."""
    rng = np.random.default_rng(width)
    lengths = [16 * width - 1, 16 * width, 16 * width + 1, 1448, 1460, 8948]
    b = rg.build(rng, aligned_streams(lengths, "front"), width)
    assert width_of(len(b["buf"]), len(b["res"])) == width
    run(gpu, ctx, b, f"width {width}")
    # and through the ORDERED pass (a whole wave per packet), a quarter of the pairs
    streams = aligned_streams(lengths, "ordered")[::4]
    run(gpu, ctx, rg.build(rng, streams, width), f"ORDERED, width {width}")


# ---- overlap ---------------------------------------------------------------------------------------
def overlap_stream(rng, size, npk, head=0, last=0):
    pk = []
    for _ in range(npk):
        ln = int(rng.integers(1, min(200, size - head) + 1))
        pk.append((int(rng.integers(0, size - head - ln + 1)), ln, None))
    return {"size": size, "head": head, "last": last, "pkts": pk}


def test_overlapping_payloads_with_differing_bytes(gpu, ctx):
    """Front, middle, tail and superset overlaps in one list; random lists;
    a list whose packets are all ORDERED but the first."""
    rng = np.random.default_rng(3)
    base = [(100, 60, None), (300, 80, None), (500, 50, None), (700, 90, None)]
    again = [(90, 40, None), (320, 30, None), (530, 60, None), (690, 110, None)]     # front, middle, tail, superset
    streams = [{"size": 1024, "head": 0, "last": 0, "pkts": base + again},
               {"size": 1024, "head": 100, "last": 50, "pkts": again + base},
               {"size": 2048, "head": 0, "last": 0, "pkts": [(1900 - 37 * k, 60, None) for k in range(40)]}]
    streams += [overlap_stream(rng, int(rng.choice([256, 512, 2048])), int(rng.integers(2, 30))) for _ in range(60)]
    b = rg.build(rng, streams)
    c = run(gpu, ctx, b, "overlaps")
    cstat = c.raw()[2]
    assert (cstat[b["sid"] == 0] == [1, 1, 1, 1, 2, 2, 2, 2]).all()
    assert (cstat[b["sid"] == 2] == [1] + [2] * 39).all()
    assert (cstat == cm.ORDERED).sum() > 300


# ---- list lengths -----------------------------------------------------------------------------------
def test_list_lengths_around_the_wave_and_the_wave_plan(gpu, ctx):
    """Lists of 1, 63, 64, 65 packets and at the wave-plan threshold +- 1 and
    beyond, each on one stream among short ones; in order with one in eight
    retransmitted, so both classes occur in the lane's and in the wave's plan."""
    T = RCVCOPY_WAVE_LEN
    rng = np.random.default_rng(4)
    streams = []
    for k in [1, 63, 64, 65, T - 1, T, T + 1, 2 * T, 2 * T + 1, 700]:
        pk, at = [], 0
        for _ in range(k):
            ln = int(rng.integers(1, 30))
            if pk and rng.random() < 0.125:
                at = max(0, at - int(rng.integers(1, 40)))
            pk.append((at, ln, None))
            at += ln
        streams.append({"size": 16384 + 1024, "head": 7, "last": 0, "pkts": pk})
        streams += [overlap_stream(rng, 256, int(rng.integers(1, 6))) for _ in range(9)]
    b = rg.build(rng, streams)
    assert 1000 < len(b["res"]) < 5000
    c = run(gpu, ctx, b, "list lengths")
    counts = np.bincount(c.raw()[2], minlength=6)
    assert counts[cm.FRONT] > 1000 and counts[cm.ORDERED] > 100


# ---- compaction -------------------------------------------------------------------------------------
def test_compaction_at_every_head_offset(gpu, ctx):
    rng = np.random.default_rng(5)
    streams = []
    for size in (256, 1024, 4000):
        for head in (1, 15, 16, 17, 31, 33, size // 2, size - 1):
            last = int(rng.integers(0, size - head + 1))
            end = size - head                          # head_offset + end >= size: :304 fires
            streams.append({"size": size, "head": head, "last": last,
                            "pkts": [(end - 40, 40, None)] if head < size - 40 else [(0, 1, None)]})
            streams.append({"size": size, "head": head, "last": min(last, 60),      # a hole, then only the last packet compacts
                            "pkts": [(70, 20, None), (100, 30, None), (90, 25, None), (size - head - 5 if head < size - 140 else 130, 5, None)]
                            if size - head > 140 else [(0, size - head, None)]})
        streams.append({"size": size, "head": 0, "last": 100, "pkts": [(50, 100, None), (size - 30, 30, None)]})   # exact fit at 0: no move
        streams.append({"size": size, "head": 20, "last": 100, "pkts": [(50, 100, None)]})                        # no trigger
    b = rg.build(rng, streams)
    want = expect(b)
    assert want[4]["compacted"] >= 40
    c = run(gpu, ctx, b, "compaction")
    rbuf = c.raw()[1]
    assert (rbuf["head_offset"][[len(streams) - 2, len(streams) - 1]] == [0, 20]).all()


def test_large_window_moves_by_one_byte(gpu, ctx):
    """A window of several passes of the wave moved down by 1, 15 and 16 bytes:
    a later pass must not read what an earlier one wrote."""
    rng = np.random.default_rng(6)
    streams = [{"size": 8192, "head": h, "last": 8192 - h - 10, "align": a, "pkts": [(8192 - h - 10, 10, None)]}
               for h in (1, 15, 16, 17, 1023, 1024, 1025) for a in (0, 5)]
    b = rg.build(rng, streams)
    assert expect(b)[4]["compacted"] == len(streams)
    run(gpu, ctx, b, "large windows")


# ---- bad input --------------------------------------------------------------------------------------
def test_every_bad_record_range_and_source(gpu, ctx):
    rng = np.random.default_rng(7)
    streams = [{"size": 512, "head": 10, "last": 20, "pkts": [(40, 30, None), (100, 20, None)]} for _ in range(14)]
    b = rg.build(rng, streams)
    r, abytes = b["rbuf"], len(b["arena"])
    r["rsvd"][0, 0], r["rsvd"][1, 1] = 1, 0x80000000
    r["size"][2], r["size"][3] = 0, (1 << 30) + 1
    r["data_off"][4] = abytes - 511                     # data_off + size > arena_bytes
    r["data_off"][5] = 0xFFFFFFFFFFFFFF00
    r["head_offset"][6] = 31                            # head_offset > tail_offset
    r["tail_offset"][7], r["last_len"][7] = 513, 503    # tail_offset > size
    r["last_len"][8] = 21                               # last_len != tail_offset - head_offset
    p9, p10, p11, p12 = (int(np.nonzero(b["sid"] == s)[0][0]) for s in (9, 10, 11, 12))
    b["place"]["put_off"][p9] = 512 - 29                # BAD_RANGE by one byte
    b["res"]["payload_len"][p10] += 1                   # BAD_SRC: payload_len != put_len
    b["desc"]["len"][p11] = 14 + 4 * (5 + (int(b["res"]["ihl_doff"][p11]) >> 4)) + 29   # BAD_SRC: the payload leaves the frame
    b["desc"]["offset"][p12] = len(b["buf"]) - 8        # BAD_SRC: the descriptor leaves the chunk
    c = run(gpu, ctx, b, "bad input")
    cstat = c.raw()[2]
    for s in range(9):
        assert (cstat[b["sid"] == s] == cm.BAD_BUF).all(), s
    assert [cstat[p] for p in (p9, p10, p11, p12)] == [cm.BAD_RANGE, cm.BAD_SRC, cm.BAD_SRC, cm.BAD_SRC]
    assert (cstat[b["sid"] == 13] == cm.FRONT).all()
    assert c.raw()[1][:9].tobytes() == b["rbuf"][:9].tobytes()


@pytest.mark.parametrize("garbage", [False, True])
def test_random_records(gpu, ctx, garbage):
    """Every status byte in one batch with deferrals inside the lists; then
    random bytes in d_rbuf and d_place with valid group arrays.  The stores are
    bounded by construction: the guards, the bytes outside the chunks and the
    records of BAD and absent streams are checked with the model."""
    rng = np.random.default_rng(8 + garbage)
    b = rg.random_batch(rng, 400, garbage)
    want = expect(b)
    c = run(gpu, ctx, b, f"random records, garbage = {garbage}")
    bad = np.array([bool(cm.record_bad(r, len(b["arena"]))) for r in b["rbuf"]])
    assert bad.sum() > (100 if garbage else 20)
    assert c.raw()[1][bad].tobytes() == b["rbuf"][bad].tobytes()
    assert want[4]["classes"][cm.FRONT] > 10 and want[4]["classes"][cm.BAD_BUF] > 50


# ---- the fixture through the real chain --------------------------------------------------------------
def fixture_batches():
    """Batch k of every case of the fixture as one GPU batch: the case is
    stream k's, its packets frames with the fixture's payload bytes; the
    receive state and the buffer record are what the fixture says the reference
    held in front of the batch (RBRemove applied)."""
    golden = cm.load_golden()
    ncase = len(golden)
    sizes = [size for _, size, _ in golden]
    rng = np.random.default_rng(9)
    arena, offs = rg.arena_for(rng, sizes)
    for d0, size in zip(offs, sizes):
        arena[d0:d0 + size] = cm.FILL
    tuples = [rng.integers(1, 255, 12, dtype=np.uint8).tobytes() for _ in range(ncase)]
    rings = [cm.Ring(arena[d0:d0 + size]) for d0, size in zip(offs, sizes)]           # the literal model, in place
    head_seq, serial, frags = [0] * ncase, [0] * ncase, [[] for _ in range(ncase)]
    merged = [0] * ncase
    out = []
    for k in range(max(len(bt) for _, _, bt in golden)):
        state, rbuf = np.zeros(ncase, RCV_STATE_DTYPE), np.zeros(ncase, RCV_BUF_DTYPE)
        frames, owner, fixture_after = [], [], {}
        for c, (fam, size, batches) in enumerate(golden):
            if k < len(batches):
                removed, pk, after, fr_after, data = batches[k]
                cm.remove(rings[c], removed)
                head_seq[c] += removed
                merged[c] -= removed
                fr = [(s, ln) for s, ln in frags[c]]
                if removed:
                    fr = fr[1:] if removed == fr[0][1] else [(fr[0][0] + removed, fr[0][1] - removed)] + fr[1:]
                frags[c] = fr
            st = state[c]
            st["head_seq"], st["merged_len"], st["size"] = (INIT_SEQ + head_seq[c]) & 0xFFFFFFFF, merged[c], size
            st["rcv_nxt"], st["rcv_wnd"] = (INIT_SEQ + head_seq[c] + merged[c]) & 0xFFFFFFFF, size - merged[c]
            st["tcp_state"], st["nfrag"] = 4, min(len(frags[c]), 4)
            for i, (s, ln) in enumerate(frags[c][:4]):
                st["frag"][i] = ((INIT_SEQ + s) & 0xFFFFFFFF, ln)
            state[c] = st
            rbuf[c] = (offs[c], size, rings[c].head, rings[c].tail, rings[c].last, (0, 0))
            if k >= len(batches) or len(frags[c]) > 4:
                continue                               # more fragments than the state holds: the case ends here
            for off, ln, ret in pk:
                body = cm.payload_bytes(c, serial[c], ln).tobytes()
                serial[c] += 1
                doff = 5 + (off + c) % 4
                f = tm.frame_raw(5, doff, 0x10, bytes(4 * (doff - 5)) + body, seed=len(frames))
                f[26:34], f[34:38] = tuples[c][:8], tuples[c][8:12]
                f[38:42] = ((INIT_SEQ + off) & 0xFFFFFFFF).to_bytes(4, "big")
                frames.append(f)
                owner.append(c)
            fixture_after[c] = (after, fr_after, data)
            frags[c], merged[c] = [(s, ln) for s, ln in fr_after], after[4]
        # the streams interleave, every list keeps its order: packet i of each case, case by case
        seen, rank = {}, []
        for c in owner:
            rank.append(seen.get(c, 0))
            seen[c] = rank[-1] + 1
        order = sorted(range(len(frames)), key=lambda i: (rank[i], owner[i]))
        frames_k, owner_k = [frames[i] for i in order], [owner[i] for i in order]
        buf, desc = tm.pack_chunk(frames_k, slot=64)
        tm.fill_checksums(buf, desc)
        out.append({"buf": buf, "desc": desc.astype(oracle.DESC_DTYPE), "owner": np.array(owner_k), "state": state,
                    "rbuf": rbuf, "arena": arena.copy(), "after": fixture_after, "tuples": tuples, "offs": offs,
                    "sizes": sizes})
        # the reference's own bytes carry on: the next batch starts from the fixture's chunk
        for c, (after, fr_after, data) in fixture_after.items():
            rings[c].data[:] = data
            rings[c].head, rings[c].tail, rings[c].last = after[:3]
    return out


def test_fixture_through_rx_lookup_group_walk_and_copy(gpu):
    """d_place comes from the walk itself.  Where the walk stored every packet
    RBPut stored, the chunk and the offsets are the reference's own."""
    matched = total = 0
    golden = cm.load_golden()
    with gpu.Context(0) as cx, gpu.FlowTable(cx, 10) as tab:
        st = torch.cuda.Stream(device=DEV)
        first = True
        for k, fb in enumerate(fixture_batches()):
            n, ncase = len(fb["desc"]), len(fb["state"])
            if n == 0:
                continue
            max_id = ncase - 1
            res = oracle.rx_chunk(fb["buf"], fb["desc"], 0, None)
            assert (res["verdict"] == 0).all()
            d_buf, d_desc = to_dev(fb["buf"]), to_dev(fb["desc"])
            d_res = torch.zeros(n * 40, dtype=torch.uint8, device=DEV)
            sid, g = Guarded(4 * n), (Guarded(4 * n), Guarded(4 * n), Guarded(4 * n + 4), Guarded(4))
            gwork = Guarded(gpu.Context.group_work_bytes(n, max_id))
            wwork = Guarded(gpu.Context.rcvwalk_work_bytes(n, max_id))
            d_state, d_place, d_stop = to_dev(fb["state"]), Guarded(16 * n), Guarded(4 * n)
            cx.rx_chunk_dev(d_buf, d_desc, n, 0, d_res, stream=st)
            if first:
                keys = {}
                for i in range(n):
                    keys.setdefault(int(fb["owner"][i]), i)
                # every case's tuple, from a record of its own (the later batches hold the same streams or fewer)
                ids = sorted(keys)
                assert len(ids) == ncase
                ent = fm.entries(fm.record_keys(res[[keys[c] for c in ids]]), np.array(ids, np.uint32))
                tab.update_dev(None, 0, to_dev(ent), len(ent), stream=st)
                first = False
            tab.lookup_dev(d_res, n, sid.t, None, stream=st)
            cx.group_dev(sid.t, n, max_id, *(x.t for x in g), gwork.t, stream=st)
            cx.rcvwalk_dev(d_res, None, n, max_id, *(x.t for x in g), d_state, d_place.t, d_stop.t, wwork.t, stream=st)
            b = {"buf": fb["buf"], "desc": fb["desc"], "off_shift": 0, "res": res, "max_id": max_id,
                 "rbuf": fb["rbuf"], "arena": fb["arena"]}
            c = Call(gpu, b, walked=(d_res, d_place.t, g[0].t, g[1].t, g[2].t, g[3].t, d_stop.t))
            c.run(cx, stream=st)
            st.synchronize()
            assert np.array_equal(sid.numpy(np.uint32), fb["owner"].astype(np.uint32))
            assert d_res.cpu().numpy().tobytes() == res.tobytes()
            m = int(g[3].numpy(np.uint32)[0])
            b["place"] = d_place.numpy(RCV_PLACE_DTYPE).copy()
            b["group"] = (g[0].numpy(np.uint32).copy(), g[1].numpy(np.uint32)[:m].copy(), g[2].numpy(np.uint32)[:m + 1].copy())
            b["seg_stop"] = d_stop.numpy(np.uint32)[:m].copy()
            want = expect(b)
            c.check(want, f"fixture batch {k}")
            arena, rbuf, cstat = c.raw()
            for case, (after, fr_after, data) in fb["after"].items():
                total += 1
                mine = fb["owner"] == case
                stored = (b["place"]["flags"][mine] & RCV_COPY) != 0
                golden_pk = [ret > 0 for _, _, ret in golden[case][2][k][1]]
                if stored.tolist() != golden_pk:
                    continue                           # the walk refused what RBPut alone took (an old retransmission)
                matched += 1
                assert tuple(int(rbuf[f][case]) for f in ("head_offset", "tail_offset", "last_len")) == after[:3]
                d0, size = fb["offs"][case], fb["sizes"][case]
                pin = want[3][d0:d0 + size]
                assert (arena[d0:d0 + size][pin] == data[pin]).all(), (k, case)
    assert total > 150 and matched > 0.6 * total, (matched, total)


# ---- determinism, errors, capture ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed():
    rng = np.random.default_rng(10)
    streams = [overlap_stream(rng, int(rng.choice([256, 1024])), int(rng.integers(1, 20)),
                              head=int(rng.integers(0, 100)), last=int(rng.integers(0, 100))) for _ in range(100)]
    b = rg.build(rng, streams)
    expect(b)
    assert b["want"][4]["compacted"] > 5 and b["want"][4]["classes"][cm.ORDERED] > 100
    return b


def test_same_batch_twice_gives_equal_bytes(gpu, ctx, mixed):
    """Into two arenas, with different workspace contents: every byte equal,
    the unpinned ones of the compacted chunks included."""
    a = run(gpu, ctx, mixed, "first", work_fill=0x00).raw()
    b = run(gpu, ctx, mixed, "second", work_fill=0xFF).raw()
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_error_returns(gpu, mixed):
    from mtcp_amd._lib import MtcpGpuError
    b = mixed
    c = Call(gpu, b)
    names = ["buf", "desc", "off_shift", "res", "place", "n", "max_id", "idx", "seg_sid", "seg_start", "nseg", "seg_stop",
             "rbuf", "arena", "cstat", "work"]
    align = {"buf": 16, "desc": 8, "res": 8, "place": 16, "idx": 4, "seg_sid": 4, "seg_start": 4, "nseg": 4,
             "seg_stop": 4, "rbuf": 32, "arena": 16, "work": 16}

    def fails(cx, **kw):
        a = dict(zip(names, c.args()))
        a.update(kw)
        with pytest.raises(MtcpGpuError) as e:
            cx.rcvcopy_dev(*(a[k] for k in names))
        assert e.value.code == EINVAL, kw.keys()

    with gpu.Context(0) as cx:
        before = c.raw()
        for name, al in align.items():
            t = dict(zip(names, c.args()))[name]
            big = torch.zeros(t.numel() + 64, dtype=torch.uint8, device=DEV)
            base = (-big.data_ptr()) % 64
            fails(cx, **{name: big[base + al // 2:base + al // 2 + t.numel()]})       # misaligned by half its alignment
        fails(cx, work=c.work.t[:c.wb - 16])
        fails(cx, off_shift=17)
        fails(cx, buf=c.buf[:len(b["buf"]) - 8])                                     # buf_len not a multiple of 16
        fails(cx, n=(1 << 26) + 1)
        fails(cx, max_id=gm.MAX_ID + 1)
        lib, vp = __import__("mtcp_amd._lib", fromlist=["lib"]).lib(), ctypes.c_void_p
        ptrs = [t.data_ptr() for t in (c.buf, c.desc, c.res, c.place, c.idx, c.seg_sid, c.seg_start, c.nseg, c.seg_stop,
                                       c.rbuf.t, c.arena.t, c.cstat.t, c.work.t)]

        def raw_call(h, p, n=c.n):
            return lib.mtcp_gpu_rcvcopy_dev(h, p[0], len(b["buf"]), p[1], 0, p[2], p[3], n, c.max_id, p[4], p[5], p[6], p[7],
                                            p[8], p[9], p[10], len(b["arena"]), p[11], p[12], c.wb, None)
        assert raw_call(None, ptrs) == EINVAL
        for k in range(len(ptrs)):
            assert raw_call(cx._h, ptrs[:k] + [None] + ptrs[k + 1:]) == EINVAL, k
        assert raw_call(cx._h, [None] * len(ptrs), n=0) == 0                          # n == 0: OK without a launch
        torch.cuda.synchronize()
        after = c.raw()
        for x, y in zip(before, after):
            assert x.tobytes() == y.tobytes()
    with gpu.Context(0, compact=True) as cx:
        fails(cx)


def test_captured_walk_and_copy_replayed(gpu):
    """rcvwalk_dev and rcvcopy_dev captured once (a linear chain) and replayed
    from reset state: the same bytes."""
    fb = fixture_batches()[0]
    n, ncase = len(fb["desc"]), len(fb["state"])
    max_id = ncase - 1
    res = oracle.rx_chunk(fb["buf"], fb["desc"], 0, None)
    d_res, d_sid = to_dev(res), to_dev(fb["owner"].astype(np.uint32))
    g = (Guarded(4 * n), Guarded(4 * n), Guarded(4 * n + 4), Guarded(4))
    gwork = Guarded(gpu.Context.group_work_bytes(n, max_id))
    wwork = Guarded(gpu.Context.rcvwalk_work_bytes(n, max_id))
    d_state, d_place, d_stop = to_dev(fb["state"]), Guarded(16 * n), Guarded(4 * n)
    b = {"buf": fb["buf"], "desc": fb["desc"], "off_shift": 0, "res": res, "max_id": max_id, "rbuf": fb["rbuf"],
         "arena": fb["arena"]}
    c = Call(gpu, b, walked=(d_res, d_place.t, g[0].t, g[1].t, g[2].t, g[3].t, d_stop.t))
    st = torch.cuda.Stream(device=DEV)
    with gpu.Context(0) as cx:
        def launch():
            cx.group_dev(d_sid, n, max_id, *(x.t for x in g), gwork.t, stream=st)
            cx.rcvwalk_dev(d_res, None, n, max_id, *(x.t for x in g), d_state, d_place.t, d_stop.t, wwork.t, stream=st)
            c.run(cx, stream=st)

        launch()                                            # kernels loaded before the capture
        st.synchronize()
        m = int(g[3].numpy(np.uint32)[0])
        b["place"] = d_place.numpy(RCV_PLACE_DTYPE).copy()
        b["group"] = (g[0].numpy(np.uint32).copy(), g[1].numpy(np.uint32)[:m].copy(), g[2].numpy(np.uint32)[:m + 1].copy())
        b["seg_stop"] = d_stop.numpy(np.uint32)[:m].copy()
        want = expect(b)
        assert want[4]["classes"][cm.FRONT] > 100
        c.check(want, "before the capture")
        first = c.raw()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            launch()
        c.reset()
        d_state.copy_(to_dev(fb["state"]))
        d_place.t.fill_(SENT)
        c.work.t.fill_(0)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        c.check(want, "the replay")
        for x, y in zip(first, c.raw()):
            assert x.tobytes() == y.tobytes()
        del graph
