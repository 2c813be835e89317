"""Batches for the tests of the application write (tests/test_sndwrite_model.py,
tests/test_gpu_sndwrite.py): send buffers laid out in a payload arena and
source ranges laid out in a source region, each with 64 B guard bands around
it, and the requests on them.  Expected values come from tests/sndwrite_model.py."""
import numpy as np

from mtcp_amd._types import ACK_STATE_DTYPE, DATAGEN_STATE_DTYPE, SNDWRITE_REQ_DTYPE
from tests import sndwrite_model as sm

GUARD = 64
ARENA_FILL, SRC_FILL = 0x5A, 0xA5


class Batch:
    """snd, dtx: the record arrays; payload: the arena; chunks: (sb_off, size)
    per stream; src, wreq: set by requests()."""

    def __init__(self, snd, dtx, payload, chunks):
        self.snd, self.dtx, self.payload, self.chunks = snd, dtx, payload, chunks
        self.max_id = len(snd) - 1
        self.src = np.zeros(16, dtype=np.uint8)
        self.wreq = np.zeros(0, dtype=SNDWRITE_REQ_DTYPE)
        self.ranges = []

    def requests(self, sids, lens, src_align=None, rng=None, fill=None):
        """One request per entry: len bytes of fresh source bytes each, at
        alignment src_align[i] (mod 16) behind a guard band.  fill(i, n): the
        bytes of request i (default: random)."""
        rng = rng or np.random.default_rng(len(sids))
        n = len(sids)
        self.wreq = np.zeros(n, dtype=SNDWRITE_REQ_DTYPE)
        at, parts, self.ranges = 0, [], []
        for i in range(n):
            a = int(src_align[i]) & 15 if src_align is not None else int(rng.integers(16))
            start = ((at + GUARD + 15) & ~15) + a
            ln = int(lens[i])
            body = rng.integers(0, 256, ln, dtype=np.uint8) if fill is None else fill(i, ln)
            parts.append((start, body))
            self.wreq[i] = (sids[i], ln, start, 0, (0, 0, 0))
            self.ranges.append((start, ln))
            at = start + ln
        self.src = np.full((at + GUARD + 15) & ~15, SRC_FILL, dtype=np.uint8)
        for start, body in parts:
            self.src[start:start + len(body)] = body
        return self

    def copies(self):
        return self.snd.copy(), self.dtx.copy(), self.payload.copy()

    def expect(self):
        """(snd, dtx, payload, wres, seg_sid, seg_start, seg_stop, nseg, total) by the model."""
        snd, dtx, payload = self.copies()
        return (snd, dtx, payload, *sm.write(self.wreq, self.max_id, snd, dtx, self.src, payload))


def lay_out(bufs, chunk_align=None, rng=None, snd_wnd=None, on_send_list=None, tcp_states=None, stale_base=None):
    """The SendBufs of `bufs` as streams 0 .. len - 1: chunk i at alignment
    chunk_align[i] (mod 16) of the arena, guard bands around it."""
    rng = rng or np.random.default_rng(len(bufs))
    n = len(bufs)
    snd, dtx = np.zeros(n, dtype=ACK_STATE_DTYPE), np.zeros(n, dtype=DATAGEN_STATE_DTYPE)
    at, chunks = 0, []
    for i, b in enumerate(bufs):
        a = int(chunk_align[i]) & 15 if chunk_align is not None else int(rng.integers(16))
        off = ((at + GUARD + 15) & ~15) + a
        chunks.append((off, b.size))
        at = off + b.size
        s, d = sm.records_of(b, off, None if snd_wnd is None else snd_wnd[i],
                             0 if on_send_list is None else on_send_list[i],
                             sm.ST_ESTABLISHED if tcp_states is None else tcp_states[i],
                             None if stale_base is None else stale_base[i])
        snd[i], dtx[i] = s[0], d[0]
    payload = np.full((at + GUARD + 15) & ~15, ARENA_FILL, dtype=np.uint8)
    for (off, size), b in zip(chunks, bufs):
        payload[off:off + size] = b.data
    return Batch(snd, dtx, payload, chunks)


def buffer(rng, size, length, head_off=0, init_seq=None):
    """A SendBuf of `size` holding `length` bytes at head_off, reached through SBPut and SBRemove."""
    assert head_off + length <= size and (length or not head_off)     # an empty buffer has head_off 0
    b = sm.SendBuf(size, int(rng.integers(1 << 32)) if init_seq is None else init_seq)
    if head_off + length:
        sm.SBPut(b, rng.integers(0, 256, head_off + length, dtype=np.uint8), head_off + length)
    if head_off:
        sm.SBRemove(b, head_off)
    return b


def random_batch(rng, n_streams, n_req, sizes=(48, 64, 200, 256, 1024, 5000), dup=0.2):
    """Streams in random states after random puts and removes, requests with
    duplicates, ids above max_id, zero lengths, closed windows, other states."""
    bufs = []
    for _ in range(n_streams):
        b = sm.SendBuf(int(rng.choice(sizes)), int(rng.integers(1 << 32)))
        for _ in range(int(rng.integers(6))):
            if rng.integers(3):
                ln = 1 + int(rng.integers(b.size))
                sm.SBPut(b, rng.integers(0, 256, ln, dtype=np.uint8), ln)
            else:
                sm.SBRemove(b, 1 + int(rng.integers(b.size)))
        bufs.append(b)
    wnd = [b.size - b.len if rng.integers(8) else int(rng.choice([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF])) for b in bufs]
    states = [4 if rng.integers(10) else int(rng.integers(11)) for _ in bufs]
    batch = lay_out(bufs, rng=rng, snd_wnd=wnd, on_send_list=rng.integers(0, 2, n_streams).tolist(), tcp_states=states)
    for i in range(n_streams):
        if not rng.integers(12):
            batch.snd["has_sndbuf"][i] = 0
        k = int(rng.integers(40))                    # records no write may touch
        if k == 0:
            batch.snd["eff_mss"][i] = 0
        elif k == 1:
            batch.dtx["rsvd"][i, 1] = 1
        elif k == 2:
            batch.dtx["sb_off"][i] = len(batch.payload) - bufs[i].size + 1
        elif k == 3 and bufs[i].len:
            batch.dtx["sb_base_seq"][i] = (int(batch.dtx["sb_base_seq"][i]) - bufs[i].size) & sm.M32
    sids, lens = [], []
    for _ in range(n_req):
        sid = int(rng.integers(n_streams))
        if sids and rng.random() < dup:
            sid = sids[int(rng.integers(len(sids)))]
        if not rng.integers(15):
            sid = n_streams + int(rng.integers(3))
        sids.append(sid)
        lens.append(0 if not rng.integers(12) else 1 + int(rng.integers(int(rng.choice([16, 300, 6000])))))
    batch.requests(sids, lens, rng=rng)
    for i in range(n_req):
        k = int(rng.integers(40))
        if k == 0:
            batch.wreq["flags"][i] = 1 << int(rng.integers(32))
        elif k == 1:
            batch.wreq["rsvd"][i, int(rng.integers(3))] = 1 + int(rng.integers(1 << 20))
        elif k == 2:
            batch.wreq["src_off"][i] = len(batch.src) - int(batch.wreq["len"][i]) + 1
        elif k == 3:
            batch.wreq["len"][i] = 0x80000000
    return batch


def random_records(rng, n_streams, n_req, slot=512, src_bytes=2048):
    """Random bytes in every record array.  So that the outputs are defined (the
    header asks for disjoint chunks of the WRITTEN requests) a stream's sb_off
    either lies with its clamped sb_size inside the stream's own slot of the
    arena, or has its top bit set and so lies outside any arena."""
    snd = np.frombuffer(rng.integers(0, 256, n_streams * 128, dtype=np.uint8).tobytes(), dtype=ACK_STATE_DTYPE).copy()
    dtx = np.frombuffer(rng.integers(0, 256, n_streams * 16, dtype=np.uint8).tobytes(), dtype=DATAGEN_STATE_DTYPE).copy()
    for i in range(n_streams):
        if rng.integers(5):                          # mostly records that pass the BAD rules
            snd["rsvd"][i], snd["wscale_peer"][i] = 0, int(rng.integers(32))
            snd["eff_mss"][i] = 1 + int(rng.integers(1500))
            snd["tcp_state"][i] = 4 if rng.integers(6) else int(rng.integers(11))
            snd["has_sndbuf"][i] = int(rng.choice([0, 1, 1, 1, 1, 7]))
            dtx["rsvd"][i], dtx["on_send_list"][i], dtx["on_control_list"][i] = 0, rng.integers(2), rng.integers(2)
            snd["snd_wnd"][i] = int(rng.choice([0, 1, 5, 100, 1 << 20, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]))
        if rng.integers(6):
            size = int(rng.integers(slot - 15 + 1))
            snd["sb_size"][i] = size
            snd["sb_len"][i] = int(rng.integers(size + 1)) if rng.integers(8) else size + int(rng.integers(3))
            dtx["sb_off"][i] = i * slot + int(rng.integers(16))
            if rng.integers(6) and size:
                head = int(rng.integers(size - min(int(snd["sb_len"][i]), size) + 1))
                dtx["sb_base_seq"][i] = (int(snd["sb_head_seq"][i]) - head) & sm.M32
        else:
            dtx["sb_off"][i] |= np.uint64(1 << 63)
    payload = rng.integers(0, 256, n_streams * slot, dtype=np.uint8)
    batch = Batch(snd, dtx, payload, [(i * slot, slot) for i in range(n_streams)])
    batch.src = rng.integers(0, 256, src_bytes, dtype=np.uint8)
    wreq = np.frombuffer(rng.integers(0, 256, n_req * 32, dtype=np.uint8).tobytes(), dtype=SNDWRITE_REQ_DTYPE).copy()
    for i in range(n_req):
        if rng.integers(8):
            wreq["sid"][i] = int(rng.integers(n_streams + 1))
        if rng.integers(8):
            wreq["flags"][i], wreq["rsvd"][i] = 0, 0
        if rng.integers(8):
            wreq["len"][i] = int(rng.choice([0, 1, 15, 16, 17, 100, 700, src_bytes]))
            wreq["src_off"][i] = int(rng.integers(src_bytes - min(int(wreq["len"][i]), src_bytes) + 2))
    batch.wreq = wreq
    return batch
