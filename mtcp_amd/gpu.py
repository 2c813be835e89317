"""Python view of the C ABI (include/mtcp_gpu.h) for tests and bench.py.

Device memory and streams come from PyTorch-ROCm (plumbing only); every
computation runs in libmtcp_gpu.so's gfx950 kernels.  Mirrors the
reference's operator boundary: `dev_ioctl` answers like
io_module_func.dev_ioctl (mtcp/src/include/io_module.h:67, :80-87), rx calls
return one verdict per packet in place of ProcessPacket's return value
(mtcp/src/eth_in.c:9-56).
"""
from __future__ import annotations

import contextlib
import ctypes
import os

import numpy as np

from ._lib import check, lib
from ._types import (ADDR_ENTRY_DTYPE, DESC_DTYPE, FLOW_ENTRY_DTYPE, FLOWTAB_COUNTERS_DTYPE, MAX_PORT, MIN_PORT, RESULT16_DTYPE, RESULT_DTYPE,
                     ACKGEN_RES_DTYPE, ACKGEN_STATE_DTYPE, DATAGEN_RES_DTYPE, DATAGEN_STATE_DTYPE, RCVREAD_REQ_DTYPE, RCVREAD_RES_DTYPE, SNDWRITE_REQ_DTYPE, SNDWRITE_RES_DTYPE, RTO_REC_DTYPE, ACK_REC_DTYPE, ACK_STATE_DTYPE, RCV_PLACE_DTYPE, RCV_STATE_DTYPE, TCPOPT_DTYPE, TX_BURST_DTYPE, TX_BURST_RESULT_DTYPE, TX_LINK_DTYPE, TX_SEG_DTYPE)

F_RSS = 0x1
F_RSS_ENDIAN = 0x2
F_COMPACT = 0x4

PKT_TX_IP_CSUM = 0x01
PKT_TX_TCP_CSUM = 0x02
PKT_RX_TCP_LROSEG = 0x03
PKT_TX_TCPIP_CSUM = 0x04
PKT_RX_IP_CSUM = 0x05
PKT_RX_TCP_CSUM = 0x06
PKT_TX_TCPIP_CSUM_PEEK = 0x07


def _stream_handle(stream) -> int | None:
    if stream is None:
        return None
    if isinstance(stream, int):
        return stream
    return stream.cuda_stream   # torch.cuda.Stream


def _dptr(t) -> int:
    if not t.is_cuda:
        raise ValueError("device-resident entry points take GPU tensors")
    return t.data_ptr()


class Context:
    """One mtcp_gpu_ctx (one per mTCP thread; not re-entrant).

    The `*_dev` methods take GPU tensors and a `stream`: a torch.cuda.Stream
    or a raw hipStream_t handle; None (the default) orders the call after
    the work PyTorch has queued on its current stream, as a torch op would."""

    def __init__(self, device: int = 0, rss: bool = False, rss_key: bytes | None = None,
                 rss_queues: int = 1, rss_endian: bool = True, compact: bool = False):
        L = lib()
        self._h = ctypes.c_void_p()
        flags = (F_RSS if rss else 0) | (F_RSS_ENDIAN if (rss and rss_endian) else 0)
        flags |= F_COMPACT if compact else 0
        key = None
        if rss_key is not None:
            if len(rss_key) != 40:
                raise ValueError("RSS key must be 40 bytes (util/rss.c:84-90)")
            self._key = (ctypes.c_uint8 * 40).from_buffer_copy(rss_key)
            key = ctypes.cast(self._key, ctypes.c_void_p)
        check(L.mtcp_gpu_open(ctypes.byref(self._h), device, key, rss_queues, flags),
              "mtcp_gpu_open")
        self.device = device
        self.compact = compact
        # Q of the steer calls (mtcp_gpu_steer.h): 1 without RSS
        self.num_queues = rss_queues if rss else 1
        # the rx records this context writes (numpy dtype of one record)
        self.result_dtype = RESULT16_DTYPE if compact else RESULT_DTYPE

    @property
    def record_size(self) -> int:
        return lib().mtcp_gpu_record_size(self._h)

    @property
    def last_kernel(self) -> str:
        """The kernel the last rx / tx launch dispatched (mtcp_gpu_last_kernel)."""
        return lib().mtcp_gpu_last_kernel(self._h).decode()

    # -- lifetime ----------------------------------------------------------
    def close(self) -> None:
        if self._h:
            lib().mtcp_gpu_close(self._h)
            self._h = ctypes.c_void_p()

    @property
    def wait_limit(self) -> int:
        """The bound of every wait of this context's synchronous calls, in us
        (0: none; mtcp_gpu_set_wait_limit)."""
        return lib().mtcp_gpu_wait_limit(self._h)

    @wait_limit.setter
    def wait_limit(self, timeout_us: int) -> None:
        check(lib().mtcp_gpu_set_wait_limit(self._h, timeout_us), "mtcp_gpu_set_wait_limit")

    def reserve(self, max_bytes: int, max_pkts: int) -> None:
        """Allocate the host calls' device staging and load the kernels now
        (mtcp_gpu_reserve), instead of on the first host-buffer call."""
        check(lib().mtcp_gpu_reserve(self._h, max_bytes, max_pkts), "mtcp_gpu_reserve")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stream(self) -> int:
        return lib().mtcp_gpu_stream(self._h) or 0

    def sync(self) -> None:
        check(lib().mtcp_gpu_sync(self._h), "mtcp_gpu_sync")

    def dev_ioctl(self, cmd: int, nif: int = 0) -> int:
        return lib().mtcp_gpu_dev_ioctl(self._h, nif, cmd, None)

    # -- device-resident ---------------------------------------------------
    @contextlib.contextmanager
    def _ordered(self, stream):
        """The stream handle for one device call.  None: PyTorch's current
        stream OF THIS CONTEXT'S DEVICE (whatever device is current); when
        that is the legacy default stream, which the C-ABI cannot name (NULL
        there means the context's own non-blocking stream), the call is
        ordered by synchronizing that device's default stream before and the
        context's stream after."""
        if stream is not None:
            yield _stream_handle(stream)
            return
        import torch
        cur = torch.cuda.current_stream(self.device)
        if cur.cuda_stream:
            yield cur.cuda_stream
            return
        cur.synchronize()
        yield None
        torch.cuda.ExternalStream(lib().mtcp_gpu_stream(self._h), device=self.device).synchronize()

    def rx_chunk_dev(self, buf, desc, n: int, off_shift: int, out, stream=None, hint=None) -> None:
        """hint: (min_len, max_len) of the batch's frames -> mtcp_gpu_rx_chunk_hint_dev."""
        with self._ordered(stream) as st:
            if hint is None:
                check(lib().mtcp_gpu_rx_chunk_dev(self._h, _dptr(buf), buf.numel() * buf.element_size(),
                                                  _dptr(desc), n, off_shift, _dptr(out),
                                                  st), "mtcp_gpu_rx_chunk_dev")
            else:
                h = (ctypes.c_uint16 * 2)(*hint)
                check(lib().mtcp_gpu_rx_chunk_hint_dev(self._h, _dptr(buf), buf.numel() * buf.element_size(),
                                                       _dptr(desc), n, off_shift, _dptr(out), None,
                                                       ctypes.cast(h, ctypes.c_void_p), st),
                      "mtcp_gpu_rx_chunk_hint_dev")

    def rx_ptrs_dev(self, ptrs, lens, n: int, out, stream=None) -> None:
        with self._ordered(stream) as st:
            check(lib().mtcp_gpu_rx_ptrs_dev(self._h, _dptr(ptrs), _dptr(lens), n, _dptr(out),
                                             st), "mtcp_gpu_rx_ptrs_dev")

    def rx_chunk_flow_dev(self, buf, desc, n: int, off_shift: int, out, bins, stream=None) -> None:
        with self._ordered(stream) as st:
            check(lib().mtcp_gpu_rx_chunk_flow_dev(self._h, _dptr(buf), buf.numel() * buf.element_size(),
                                                   _dptr(desc), n, off_shift, _dptr(out), _dptr(bins),
                                                   st), "mtcp_gpu_rx_chunk_flow_dev")

    def rx_ptrs_flow_dev(self, ptrs, lens, n: int, out, bins, stream=None) -> None:
        with self._ordered(stream) as st:
            check(lib().mtcp_gpu_rx_ptrs_flow_dev(self._h, _dptr(ptrs), _dptr(lens), n, _dptr(out),
                                                  _dptr(bins), st),
                  "mtcp_gpu_rx_ptrs_flow_dev")

    def tx_fill_ptrs_dev(self, ptrs, lens, n: int, stream=None) -> None:
        with self._ordered(stream) as st:
            check(lib().mtcp_gpu_tx_fill_ptrs_dev(self._h, _dptr(ptrs), _dptr(lens), n,
                                                  st), "mtcp_gpu_tx_fill_ptrs_dev")

    def tx_fill_dev(self, buf, desc, n: int, off_shift: int, stream=None) -> None:
        with self._ordered(stream) as st:
            check(lib().mtcp_gpu_tx_fill_dev(self._h, _dptr(buf), buf.numel() * buf.element_size(),
                                             _dptr(desc), n, off_shift, st),
                  "mtcp_gpu_tx_fill_dev")

    # -- host memory ---------------------------------------------------------
    def rx_chunk(self, buf: np.ndarray, desc: np.ndarray, off_shift: int = 0,
                 out: np.ndarray | None = None) -> np.ndarray:
        desc = np.ascontiguousarray(desc, dtype=DESC_DTYPE)
        if out is None:
            out = np.zeros(len(desc), dtype=self.result_dtype)
        if out.dtype.itemsize != self.result_dtype.itemsize:
            raise ValueError("out must hold this context's records (compact: 16 B)")
        check(lib().mtcp_gpu_rx_chunk(self._h, buf.ctypes.data, buf.nbytes, desc.ctypes.data,
                                      len(desc), off_shift, out.ctypes.data), "mtcp_gpu_rx_chunk")
        return out

    def rx_ptrs(self, frames: list) -> np.ndarray:
        n = len(frames)
        arrs = [np.ascontiguousarray(np.frombuffer(bytes(f), dtype=np.uint8)) for f in frames]
        ptrs = (ctypes.c_void_p * n)(*[a.ctypes.data for a in arrs])
        lens = np.array([a.nbytes for a in arrs], dtype=np.uint16)
        out = np.zeros(n, dtype=self.result_dtype)
        check(lib().mtcp_gpu_rx_ptrs(self._h, ctypes.cast(ptrs, ctypes.c_void_p),
                                     lens.ctypes.data, n, out.ctypes.data), "mtcp_gpu_rx_ptrs")
        return out

    def tx_fill(self, buf: np.ndarray, desc: np.ndarray, off_shift: int = 0) -> int:
        desc = np.ascontiguousarray(desc, dtype=DESC_DTYPE)
        cnt = ctypes.c_uint32(0)
        check(lib().mtcp_gpu_tx_fill(self._h, buf.ctypes.data, buf.nbytes, desc.ctypes.data,
                                     len(desc), off_shift, ctypes.byref(cnt)), "mtcp_gpu_tx_fill")
        return cnt.value

    def tx_fill_ptrs(self, buf: np.ndarray, offsets, lens, timeout_us: int | None = None) -> int:
        """mtcp_gpu_tx_fill_ptrs over frames of the host array `buf` at byte
        `offsets` (a DPDK-style pointer burst into one host buffer); fills
        `buf` in place and returns the number of frames filled.  With
        timeout_us: mtcp_gpu_tx_fill_ptrs_for (MtcpGpuError ETIMEDOUT past
        the limit, the context abandoned; 0: the context's wait limit)."""
        offsets = np.asarray(offsets, dtype=np.int64)
        n = len(offsets)
        ptrs = (ctypes.c_void_p * max(n, 1))(*[buf.ctypes.data + int(o) for o in offsets])
        lens = np.ascontiguousarray(lens, dtype=np.uint16)
        cnt = ctypes.c_uint32(0)
        if timeout_us is None:
            check(lib().mtcp_gpu_tx_fill_ptrs(self._h, ctypes.cast(ptrs, ctypes.c_void_p), lens.ctypes.data,
                                              n, ctypes.byref(cnt)), "mtcp_gpu_tx_fill_ptrs")
        else:
            check(lib().mtcp_gpu_tx_fill_ptrs_for(self._h, ctypes.cast(ptrs, ctypes.c_void_p),
                                                  lens.ctypes.data, n, ctypes.byref(cnt), timeout_us),
                  "mtcp_gpu_tx_fill_ptrs_for")
        return cnt.value

    # -- flow-table hash (HashFlow, mtcp/src/tcp_stream.c:56-90) -------------
    def flow_hash_dev(self, res, n: int, bins, stream=None) -> None:
        with self._ordered(stream) as st:
            check(lib().mtcp_gpu_flow_hash_dev(self._h, _dptr(res), n, _dptr(bins),
                                               st), "mtcp_gpu_flow_hash_dev")

    def flow_hash(self, res: np.ndarray) -> np.ndarray:
        res = np.ascontiguousarray(res, dtype=RESULT_DTYPE)
        bins = np.zeros(len(res), dtype=np.uint32)
        check(lib().mtcp_gpu_flow_hash(self._h, res.ctypes.data, len(res), bins.ctypes.data),
              "mtcp_gpu_flow_hash")
        return bins

    # -- TCP option records (ParseTCPTimestamp / ParseTCPOptions, tcp_util.c:14-92) --
    def rx_tcpopt_chunk_dev(self, buf, desc, n: int, off_shift: int, res, opt, stream=None) -> None:
        """res: the records this context's rx call wrote for these frames;
        opt: n x 16 B (TCPOPT_DTYPE)."""
        with self._ordered(stream) as st:
            check(lib().mtcp_gpu_rx_tcpopt_chunk_dev(self._h, _dptr(buf), buf.numel() * buf.element_size(),
                                                     _dptr(desc), n, off_shift, _dptr(res), _dptr(opt),
                                                     st), "mtcp_gpu_rx_tcpopt_chunk_dev")

    def rx_tcpopt_ptrs_dev(self, ptrs, lens, n: int, res, opt, stream=None) -> None:
        with self._ordered(stream) as st:
            check(lib().mtcp_gpu_rx_tcpopt_ptrs_dev(self._h, _dptr(ptrs), _dptr(lens), n, _dptr(res),
                                                    _dptr(opt), st), "mtcp_gpu_rx_tcpopt_ptrs_dev")

    def rx_chunk_opts(self, buf: np.ndarray, desc: np.ndarray,
                      off_shift: int = 0) -> tuple[np.ndarray, np.ndarray]:
        """mtcp_gpu_rx_chunk_opts: rx_chunk's records and the option records."""
        desc = np.ascontiguousarray(desc, dtype=DESC_DTYPE)
        out = np.zeros(len(desc), dtype=self.result_dtype)
        opts = np.zeros(len(desc), dtype=TCPOPT_DTYPE)
        check(lib().mtcp_gpu_rx_chunk_opts(self._h, buf.ctypes.data, buf.nbytes, desc.ctypes.data,
                                           len(desc), off_shift, out.ctypes.data, opts.ctypes.data),
              "mtcp_gpu_rx_chunk_opts")
        return out, opts

    # -- steering by RSS queue (dpdk_module.c:101-121, :401-402; mtcp_gpu_steer.h) --
    @staticmethod
    def steer_tile() -> int:
        return lib().mtcp_gpu_steer_tile()

    def steer_work_bytes(self, n: int) -> int:
        return lib().mtcp_gpu_steer_work_bytes(self._h, n)

    def steer_dev(self, res, n: int, idx, start, work, flags: int = 0, desc=None, desc_out=None,
                  stream=None) -> None:
        """res: this context's rx records; idx: n x u32; start: (Q + 2) x u32;
        work: at least steer_work_bytes(n) bytes, 16 B aligned; desc / desc_out:
        both or neither."""
        with self._ordered(stream) as st:
            check(lib().mtcp_gpu_steer_dev(self._h, _dptr(res), n, flags, _dptr(idx), _dptr(start),
                                           None if desc is None else _dptr(desc),
                                           None if desc_out is None else _dptr(desc_out), _dptr(work),
                                           work.numel() * work.element_size(), st), "mtcp_gpu_steer_dev")

    def steer(self, res: np.ndarray, flags: int = 0) -> tuple[np.ndarray, np.ndarray]:
        """mtcp_gpu_steer: (idx, start) of this context's records in host memory."""
        res = np.ascontiguousarray(res, dtype=self.result_dtype)
        idx = np.zeros(len(res), dtype=np.uint32)
        start = np.zeros(self.num_queues + 2, dtype=np.uint32)
        check(lib().mtcp_gpu_steer(self._h, res.ctypes.data, len(res), flags, idx.ctypes.data,
                                   start.ctypes.data), "mtcp_gpu_steer")
        return idx, start

    # -- grouping by stream (core.c:768-777, tcp_in.c:1181-1186; mtcp_gpu_group.h) --
    @staticmethod
    def group_tile() -> int:
        return lib().mtcp_gpu_group_tile()

    @staticmethod
    def group_work_bytes(n: int, max_id: int) -> int:
        """mtcp_gpu_group_work_bytes (host only, needs no GPU)."""
        return lib().mtcp_gpu_group_work_bytes(n, max_id)

    def group_dev(self, sid, n: int, max_id: int, idx, seg_sid, seg_start, nseg, work, stream=None) -> None:
        """sid: n x u32 as FlowTable.lookup_dev writes them; idx, seg_sid: n x u32;
        seg_start: (n + 1) x u32; nseg: 1 x u32; work: at least
        group_work_bytes(n, max_id) bytes, 16 B aligned."""
        with self._ordered(stream) as st:
            check(lib().mtcp_gpu_group_dev(self._h, _dptr(sid), n, max_id, _dptr(idx), _dptr(seg_sid),
                                           _dptr(seg_start), _dptr(nseg), _dptr(work),
                                           work.numel() * work.element_size(), st), "mtcp_gpu_group_dev")

    def group(self, sid: np.ndarray, max_id: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """mtcp_gpu_group: (idx, seg_sid, seg_start) of stream ids in host memory,
        the table cut to its m and m + 1 entries."""
        sid = np.ascontiguousarray(sid, dtype=np.uint32)
        n = len(sid)
        idx, seg_sid = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        seg_start, nseg = np.zeros(n + 1, dtype=np.uint32), np.zeros(1, dtype=np.uint32)
        check(lib().mtcp_gpu_group(self._h, sid.ctypes.data, n, max_id, idx.ctypes.data, seg_sid.ctypes.data,
                                   seg_start.ctypes.data, nseg.ctypes.data), "mtcp_gpu_group")
        m = int(nseg[0])
        return idx, seg_sid[:m], seg_start[:m + 1]

    # -- the per-stream receive walk (tcp_in.c:101-179, :537-610, tcp_ring_buffer.c:280-382; mtcp_gpu_rcvwalk.h) --
    @staticmethod
    def rcvwalk_work_bytes(n: int, max_id: int) -> int:
        """mtcp_gpu_rcvwalk_work_bytes (host only, needs no GPU)."""
        return lib().mtcp_gpu_rcvwalk_work_bytes(n, max_id)

    @staticmethod
    def rcvwalk_short_len() -> int:
        return lib().mtcp_gpu_rcvwalk_short_len()

    def rcvwalk_dev(self, res, opt, n: int, max_id: int, idx, seg_sid, seg_start, nseg, state, place, seg_stop,
                    work, stream=None) -> None:
        """res: n x 40 B records; opt: n x 16 B option records or None; idx,
        seg_sid, seg_start, nseg: as group_dev wrote them; state: (max_id + 1) x
        64 B (RCV_STATE_DTYPE), updated; place: n x 16 B (RCV_PLACE_DTYPE);
        seg_stop: n x u32; work: at least rcvwalk_work_bytes(n, max_id) bytes."""
        with self._ordered(stream) as st:
            check(lib().mtcp_gpu_rcvwalk_dev(self._h, _dptr(res), None if opt is None else _dptr(opt), n, max_id,
                                             _dptr(idx), _dptr(seg_sid), _dptr(seg_start), _dptr(nseg), _dptr(state),
                                             _dptr(place), _dptr(seg_stop), _dptr(work),
                                             work.numel() * work.element_size(), st), "mtcp_gpu_rcvwalk_dev")

    def rcvwalk(self, res: np.ndarray, opt, max_id: int, idx: np.ndarray, seg_sid: np.ndarray,
                seg_start: np.ndarray, state: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
        """mtcp_gpu_rcvwalk over the arrays group() returned: `state`
        ((max_id + 1) x RCV_STATE_DTYPE) is updated in place; returns (place,
        seg_stop), seg_stop cut to the table's m entries."""
        res = np.ascontiguousarray(res, dtype=RESULT_DTYPE)
        if opt is not None:
            opt = np.ascontiguousarray(opt, dtype=TCPOPT_DTYPE)
        n, m = len(res), len(seg_sid)
        if state.dtype != RCV_STATE_DTYPE or not state.flags.c_contiguous or len(state) != max_id + 1:
            raise ValueError("state: (max_id + 1) contiguous RCV_STATE_DTYPE records")
        idx, seg_sid = np.ascontiguousarray(idx, dtype=np.uint32), np.ascontiguousarray(seg_sid, dtype=np.uint32)
        seg_start, nseg = np.ascontiguousarray(seg_start, dtype=np.uint32), np.array([m], dtype=np.uint32)
        place, seg_stop = np.zeros(n, dtype=RCV_PLACE_DTYPE), np.zeros(max(m, 1), dtype=np.uint32)
        check(lib().mtcp_gpu_rcvwalk(self._h, res.ctypes.data, None if opt is None else opt.ctypes.data, n, max_id,
                                     idx.ctypes.data, seg_sid.ctypes.data, seg_start.ctypes.data, nseg.ctypes.data,
                                     state.ctypes.data, place.ctypes.data, seg_stop.ctypes.data), "mtcp_gpu_rcvwalk")
        return place, seg_stop[:m]

    # -- the per-stream ProcessACK walk (tcp_in.c:302-531; mtcp_gpu_ackwalk.h) --
    @staticmethod
    def ackwalk_work_bytes(n: int, max_id: int) -> int:
        """mtcp_gpu_ackwalk_work_bytes (host only, needs no GPU)."""
        return lib().mtcp_gpu_ackwalk_work_bytes(n, max_id)

    @staticmethod
    def ackwalk_short_len() -> int:
        return lib().mtcp_gpu_ackwalk_short_len()

    def ackwalk_dev(self, res, opt, place, n: int, max_id: int, idx, seg_sid, seg_start, nseg, cur_ts: int, snd, ack,
                    ack_stop, work, stream=None) -> None:
        """res: n x 40 B records; opt: n x 16 B option records or None; place:
        n x 16 B as rcvwalk_dev wrote them; idx, seg_sid, seg_start, nseg: as
        group_dev wrote them; snd: (max_id + 1) x 128 B (ACK_STATE_DTYPE),
        updated; ack: n x 16 B (ACK_REC_DTYPE); ack_stop: n x u32; work: at
        least ackwalk_work_bytes(n, max_id) bytes."""
        with self._ordered(stream) as st:
            check(lib().mtcp_gpu_ackwalk_dev(self._h, _dptr(res), None if opt is None else _dptr(opt), _dptr(place), n,
                                             max_id, _dptr(idx), _dptr(seg_sid), _dptr(seg_start), _dptr(nseg),
                                             cur_ts & 0xFFFFFFFF, _dptr(snd), _dptr(ack), _dptr(ack_stop), _dptr(work),
                                             work.numel() * work.element_size(), st), "mtcp_gpu_ackwalk_dev")

    def ackwalk(self, res: np.ndarray, opt, place: np.ndarray, max_id: int, idx: np.ndarray, seg_sid: np.ndarray,
                seg_start: np.ndarray, cur_ts: int, snd: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
        """mtcp_gpu_ackwalk over the arrays group() and rcvwalk() returned:
        `snd` ((max_id + 1) x ACK_STATE_DTYPE) is updated in place; returns
        (ack, ack_stop), ack_stop cut to the table's m entries."""
        res = np.ascontiguousarray(res, dtype=RESULT_DTYPE)
        if opt is not None:
            opt = np.ascontiguousarray(opt, dtype=TCPOPT_DTYPE)
        place = np.ascontiguousarray(place, dtype=RCV_PLACE_DTYPE)
        n, m = len(res), len(seg_sid)
        if snd.dtype != ACK_STATE_DTYPE or not snd.flags.c_contiguous or len(snd) != max_id + 1:
            raise ValueError("snd: (max_id + 1) contiguous ACK_STATE_DTYPE records")
        if len(place) != n:
            raise ValueError("place: one record per packet")
        idx, seg_sid = np.ascontiguousarray(idx, dtype=np.uint32), np.ascontiguousarray(seg_sid, dtype=np.uint32)
        seg_start, nseg = np.ascontiguousarray(seg_start, dtype=np.uint32), np.array([m], dtype=np.uint32)
        ack, ack_stop = np.zeros(n, dtype=ACK_REC_DTYPE), np.zeros(max(m, 1), dtype=np.uint32)
        check(lib().mtcp_gpu_ackwalk(self._h, res.ctypes.data, None if opt is None else opt.ctypes.data,
                                     place.ctypes.data, n, max_id, idx.ctypes.data, seg_sid.ctypes.data,
                                     seg_start.ctypes.data, nseg.ctypes.data, cur_ts & 0xFFFFFFFF, snd.ctypes.data,
                                     ack.ctypes.data, ack_stop.ctypes.data), "mtcp_gpu_ackwalk")
        return ack, ack_stop[:m]

    # -- pure-ACK tx segments from a walked batch (tcp_out.c:911-935, :697-761, :220-354; mtcp_gpu_ackgen.h) --
    @staticmethod
    def ackgen_work_bytes(n: int, max_id: int) -> int:
        """mtcp_gpu_ackgen_work_bytes (host only, needs no GPU)."""
        return lib().mtcp_gpu_ackgen_work_bytes(n, max_id)

    @staticmethod
    def ackgen_lane_len() -> int:
        return lib().mtcp_gpu_ackgen_lane_len()

    def ackgen_dev(self, place, n: int, max_id: int, idx, seg_sid, seg_start, nseg, seg_stop, ack_stop, state, snd,
                   cur_ts: int, tx, n_links: int, buf_off: int, buf_len: int, off_shift: int, slot_bytes: int, seg,
                   desc, seg_cap: int, ares, total, work, stream=None) -> None:
        """place, seg_stop: as rcvwalk_dev wrote them; ack_stop: as ackwalk_dev
        wrote it, or None; idx, seg_sid, seg_start, nseg: as group_dev wrote
        them; state, snd: the walks' (max_id + 1) records; tx: (max_id + 1) x
        32 B (ACKGEN_STATE_DTYPE), updated; seg: seg_cap x 48 B; desc: seg_cap
        x 8 B; ares: n x 16 B (ACKGEN_RES_DTYPE); total: 2 x u64; work: at
        least ackgen_work_bytes(n, max_id) bytes."""
        with self._ordered(stream) as st:
            check(lib().mtcp_gpu_ackgen_dev(self._h, _dptr(place), n, max_id, _dptr(idx), _dptr(seg_sid),
                                            _dptr(seg_start), _dptr(nseg), _dptr(seg_stop),
                                            None if ack_stop is None else _dptr(ack_stop), _dptr(state), _dptr(snd),
                                            cur_ts & 0xFFFFFFFF, _dptr(tx), n_links, buf_off, buf_len, off_shift,
                                            slot_bytes, _dptr(seg), _dptr(desc), seg_cap, _dptr(ares), _dptr(total),
                                            _dptr(work), work.numel() * work.element_size(), st),
                  "mtcp_gpu_ackgen_dev")

    def ack_send_dev(self, place, n: int, max_id: int, idx, seg_sid, seg_start, nseg, seg_stop, ack_stop, state, snd,
                     cur_ts: int, tx, links, buf, buf_off: int, off_shift: int, slot_bytes: int, seg, desc,
                     seg_cap: int, ares, total, status, work, flags: int = 0, buf_len: int | None = None,
                     stream=None) -> None:
        """ackgen_dev, then tx_build_dev over all seg_cap records, on one stream.
        buf_len: the bytes of buf the call may use (None: all of it)."""
        room = buf.numel() * buf.element_size()
        if buf_len is not None and not 0 <= buf_len <= room:
            raise ValueError("buf_len: at most the bytes of buf")
        with self._ordered(stream) as st:
            check(lib().mtcp_gpu_ack_send_dev(self._h, _dptr(place), n, max_id, _dptr(idx), _dptr(seg_sid),
                                              _dptr(seg_start), _dptr(nseg), _dptr(seg_stop),
                                              None if ack_stop is None else _dptr(ack_stop), _dptr(state), _dptr(snd),
                                              cur_ts & 0xFFFFFFFF, _dptr(tx), _dptr(links),
                                              links.numel() * links.element_size() // 12, _dptr(buf), buf_off,
                                              room if buf_len is None else buf_len, off_shift, slot_bytes, flags,
                                              _dptr(seg), _dptr(desc), seg_cap, _dptr(ares), _dptr(total),
                                              _dptr(status), _dptr(work), work.numel() * work.element_size(), st),
                  "mtcp_gpu_ack_send_dev")

    def ackgen(self, place: np.ndarray, max_id: int, idx: np.ndarray, seg_sid: np.ndarray, seg_start: np.ndarray,
               seg_stop: np.ndarray, ack_stop, state: np.ndarray, snd: np.ndarray, cur_ts: int, tx: np.ndarray,
               n_links: int, buf_len: int, seg_cap: int, buf_off: int = 0, off_shift: int = 0, slot_bytes: int = 0):
        """mtcp_gpu_ackgen over the arrays group(), rcvwalk() and ackwalk()
        returned: `tx` ((max_id + 1) x ACKGEN_STATE_DTYPE) is updated in place;
        returns (seg, desc, ares, total), ares cut to the table's m entries."""
        place = np.ascontiguousarray(place, dtype=RCV_PLACE_DTYPE)
        n, m = len(place), len(seg_sid)
        for a, dt, name in ((tx, ACKGEN_STATE_DTYPE, "tx"), (state, RCV_STATE_DTYPE, "state"), (snd, ACK_STATE_DTYPE, "snd")):
            if a.dtype != dt or not a.flags.c_contiguous or len(a) != max_id + 1:
                raise ValueError(f"{name}: (max_id + 1) contiguous records of its dtype")
        u32 = lambda a: np.ascontiguousarray(a, dtype=np.uint32)
        idx, seg_sid, seg_start, seg_stop = u32(idx), u32(seg_sid), u32(seg_start), u32(seg_stop)
        ack_stop = None if ack_stop is None else u32(ack_stop)
        nseg = np.array([m], dtype=np.uint32)
        seg, desc = np.zeros(seg_cap, dtype=TX_SEG_DTYPE), np.zeros(seg_cap, dtype=DESC_DTYPE)
        ares, total = np.zeros(max(m, 1), dtype=ACKGEN_RES_DTYPE), np.zeros(2, dtype=np.uint64)
        check(lib().mtcp_gpu_ackgen(self._h, place.ctypes.data, n, max_id, idx.ctypes.data, seg_sid.ctypes.data,
                                    seg_start.ctypes.data, nseg.ctypes.data, seg_stop.ctypes.data,
                                    None if ack_stop is None else ack_stop.ctypes.data, state.ctypes.data,
                                    snd.ctypes.data, cur_ts & 0xFFFFFFFF, tx.ctypes.data, n_links, buf_off, buf_len,
                                    off_shift, slot_bytes, seg.ctypes.data, desc.ctypes.data, seg_cap,
                                    ares.ctypes.data, total.ctypes.data), "mtcp_gpu_ackgen")
        return seg, desc, ares[:m], total

    # -- data tx segments from a walked batch (tcp_out.c:607-660, :357-449; mtcp_gpu_datagen.h) --
    @staticmethod
    def datagen_work_bytes(n: int, max_id: int) -> int:
        """mtcp_gpu_datagen_work_bytes (host only, needs no GPU)."""
        return lib().mtcp_gpu_datagen_work_bytes(n, max_id)

    @staticmethod
    def datagen_lane_len() -> int:
        return lib().mtcp_gpu_datagen_lane_len()

    def datagen_dev(self, ack, ack_stop, n: int, max_id: int, idx, seg_sid, seg_start, nseg, seg_stop, state, snd, tx,
                    dtx, cur_ts: int, payload_bytes: int, n_links: int, buf_off: int, buf_len: int, off_shift: int,
                    slot_bytes: int, seg, desc, seg_cap: int, dres, total, work, max_mss: int = 0, stream=None) -> None:
        """ack, ack_stop: as ackwalk_dev wrote them, or None for both; idx,
        seg_sid, seg_start, nseg: as group_dev wrote them; seg_stop: as
        rcvwalk_dev wrote it; state: the receive walk's (max_id + 1) records;
        snd ((max_id + 1) x 128 B), tx (x 32 B) and dtx (x 16 B,
        DATAGEN_STATE_DTYPE): updated; seg: seg_cap x 48 B; desc: seg_cap x 8 B;
        dres: n x 16 B (DATAGEN_RES_DTYPE); total: 2 x u64; work: at least
        datagen_work_bytes(n, max_id) bytes."""
        with self._ordered(stream) as st:
            check(lib().mtcp_gpu_datagen_dev(self._h, None if ack is None else _dptr(ack),
                                             None if ack_stop is None else _dptr(ack_stop), n, max_id, _dptr(idx),
                                             _dptr(seg_sid), _dptr(seg_start), _dptr(nseg), _dptr(seg_stop),
                                             _dptr(state), _dptr(snd), _dptr(tx), _dptr(dtx), cur_ts & 0xFFFFFFFF,
                                             payload_bytes, n_links, buf_off, buf_len, off_shift, slot_bytes, max_mss,
                                             _dptr(seg), _dptr(desc), seg_cap, _dptr(dres), _dptr(total), _dptr(work),
                                             work.numel() * work.element_size(), st), "mtcp_gpu_datagen_dev")

    def data_send_dev(self, ack, ack_stop, n: int, max_id: int, idx, seg_sid, seg_start, nseg, seg_stop, state, snd,
                      tx, dtx, cur_ts: int, payload, links, buf, buf_off: int, off_shift: int, slot_bytes: int, seg,
                      desc, seg_cap: int, dres, total, status, work, max_mss: int = 0, flags: int = 0,
                      buf_len: int | None = None, payload_bytes: int | None = None, stream=None) -> None:
        """datagen_dev, then tx_build_dev over all seg_cap records, on one
        stream.  payload: the arena the send buffers live in; buf_len: the
        bytes of buf the call may use (None: all of it)."""
        room = buf.numel() * buf.element_size()
        if buf_len is not None and not 0 <= buf_len <= room:
            raise ValueError("buf_len: at most the bytes of buf")
        pbytes = payload.numel() * payload.element_size()
        if payload_bytes is not None and not 0 <= payload_bytes <= pbytes:
            raise ValueError("payload_bytes: at most the bytes of payload")
        with self._ordered(stream) as st:
            check(lib().mtcp_gpu_data_send_dev(self._h, None if ack is None else _dptr(ack),
                                               None if ack_stop is None else _dptr(ack_stop), n, max_id, _dptr(idx),
                                               _dptr(seg_sid), _dptr(seg_start), _dptr(nseg), _dptr(seg_stop),
                                               _dptr(state), _dptr(snd), _dptr(tx), _dptr(dtx), cur_ts & 0xFFFFFFFF,
                                               _dptr(payload), pbytes if payload_bytes is None else payload_bytes,
                                               _dptr(links), links.numel() * links.element_size() // 12, _dptr(buf),
                                               buf_off, room if buf_len is None else buf_len, off_shift, slot_bytes,
                                               max_mss, flags, _dptr(seg), _dptr(desc), seg_cap, _dptr(dres),
                                               _dptr(total), _dptr(status), _dptr(work),
                                               work.numel() * work.element_size(), st), "mtcp_gpu_data_send_dev")

    def datagen(self, ack, ack_stop, max_id: int, idx: np.ndarray, seg_sid: np.ndarray, seg_start: np.ndarray,
                seg_stop: np.ndarray, state: np.ndarray, snd: np.ndarray, tx: np.ndarray, dtx: np.ndarray, cur_ts: int,
                payload_bytes: int, n_links: int, buf_len: int, seg_cap: int, buf_off: int = 0, off_shift: int = 0,
                slot_bytes: int = 0, max_mss: int = 0):
        """mtcp_gpu_datagen over the arrays group(), rcvwalk() and ackwalk()
        returned (ack and ack_stop may both be None): `snd`, `tx` and `dtx`
        ((max_id + 1) records each) are updated in place; returns (seg, desc,
        dres, total), dres cut to the table's m entries."""
        n, m = len(idx), len(seg_sid)
        for a, dt, name in ((tx, ACKGEN_STATE_DTYPE, "tx"), (state, RCV_STATE_DTYPE, "state"),
                            (snd, ACK_STATE_DTYPE, "snd"), (dtx, DATAGEN_STATE_DTYPE, "dtx")):
            if a.dtype != dt or not a.flags.c_contiguous or len(a) != max_id + 1:
                raise ValueError(f"{name}: (max_id + 1) contiguous records of its dtype")
        if (ack is None) != (ack_stop is None):
            raise ValueError("ack and ack_stop: both or neither")
        u32 = lambda a: np.ascontiguousarray(a, dtype=np.uint32)
        idx, seg_sid, seg_start, seg_stop = u32(idx), u32(seg_sid), u32(seg_start), u32(seg_stop)
        if ack is not None:
            ack, ack_stop = np.ascontiguousarray(ack, dtype=ACK_REC_DTYPE), u32(ack_stop)
            if len(ack) != n:
                raise ValueError("ack: one record per packet")
        nseg = np.array([m], dtype=np.uint32)
        seg, desc = np.zeros(seg_cap, dtype=TX_SEG_DTYPE), np.zeros(seg_cap, dtype=DESC_DTYPE)
        dres, total = np.zeros(max(m, 1), dtype=DATAGEN_RES_DTYPE), np.zeros(2, dtype=np.uint64)
        check(lib().mtcp_gpu_datagen(self._h, None if ack is None else ack.ctypes.data,
                                     None if ack_stop is None else ack_stop.ctypes.data, n, max_id, idx.ctypes.data,
                                     seg_sid.ctypes.data, seg_start.ctypes.data, nseg.ctypes.data,
                                     seg_stop.ctypes.data, state.ctypes.data, snd.ctypes.data, tx.ctypes.data,
                                     dtx.ctypes.data, cur_ts & 0xFFFFFFFF, payload_bytes, n_links, buf_off, buf_len,
                                     off_shift, slot_bytes, max_mss, seg.ctypes.data, desc.ctypes.data, seg_cap,
                                     dres.ctypes.data, total.ctypes.data), "mtcp_gpu_datagen")
        return seg, desc, dres[:m], total

    # -- the retransmission-timeout sweep (timer.c:363-419, :176-337; mtcp_gpu_rtosweep.h) --
    @staticmethod
    def rto_sweep_work_bytes(max_id: int, cap: int) -> int:
        """mtcp_gpu_rto_sweep_work_bytes (host only, needs no GPU)."""
        return lib().mtcp_gpu_rto_sweep_work_bytes(max_id, cap)

    @staticmethod
    def rto_sweep_tile() -> int:
        return lib().mtcp_gpu_rto_sweep_tile()

    def rto_sweep_dev(self, max_id: int, snd, dtx, cur_ts: int, cap: int, rto, seg_sid, seg_start, seg_stop, nseg,
                      total, work, stream=None) -> None:
        """snd ((max_id + 1) x 128 B) and dtx (x 16 B): updated; rto: cap x 16 B
        (RTO_REC_DTYPE); seg_sid: cap x u32; seg_start: (cap + 1) x u32;
        seg_stop: cap x u32; nseg: 1 x u32; total: 2 x u64 (due, handled);
        work: at least rto_sweep_work_bytes(max_id, cap) bytes."""
        with self._ordered(stream) as st:
            check(lib().mtcp_gpu_rto_sweep_dev(self._h, max_id, _dptr(snd), _dptr(dtx), cur_ts & 0xFFFFFFFF, cap,
                                               _dptr(rto), _dptr(seg_sid), _dptr(seg_start), _dptr(seg_stop),
                                               _dptr(nseg), _dptr(total), _dptr(work),
                                               work.numel() * work.element_size(), st), "mtcp_gpu_rto_sweep_dev")

    def rto_send_dev(self, max_id: int, snd, dtx, cur_ts: int, cap: int, rto, seg_sid, seg_start, seg_stop, nseg,
                     total, rwork, idx, state, tx, payload, links, buf, buf_off: int, off_shift: int,
                     slot_bytes: int, seg, desc, seg_cap: int, dres, dtotal, status, work, max_mss: int = 0,
                     flags: int = 0, buf_len: int | None = None, payload_bytes: int | None = None,
                     stream=None) -> None:
        """rto_sweep_dev, then data_send_dev over the table the sweep wrote
        (ack and ack_stop None, n = cap), on one stream.  idx: cap x u32, any
        values; rwork: the sweep's workspace; work: the data send's, at least
        datagen_work_bytes(cap, max_id) bytes; dtotal: the data send's totals."""
        room = buf.numel() * buf.element_size()
        if buf_len is not None and not 0 <= buf_len <= room:
            raise ValueError("buf_len: at most the bytes of buf")
        pbytes = payload.numel() * payload.element_size()
        if payload_bytes is not None and not 0 <= payload_bytes <= pbytes:
            raise ValueError("payload_bytes: at most the bytes of payload")
        with self._ordered(stream) as st:
            check(lib().mtcp_gpu_rto_send_dev(self._h, max_id, _dptr(snd), _dptr(dtx), cur_ts & 0xFFFFFFFF, cap,
                                              _dptr(rto), _dptr(seg_sid), _dptr(seg_start), _dptr(seg_stop),
                                              _dptr(nseg), _dptr(total), _dptr(rwork),
                                              rwork.numel() * rwork.element_size(), _dptr(idx), _dptr(state),
                                              _dptr(tx), _dptr(payload),
                                              pbytes if payload_bytes is None else payload_bytes, _dptr(links),
                                              links.numel() * links.element_size() // 12, _dptr(buf), buf_off,
                                              room if buf_len is None else buf_len, off_shift, slot_bytes, max_mss,
                                              flags, _dptr(seg), _dptr(desc), seg_cap, _dptr(dres), _dptr(dtotal),
                                              _dptr(status), _dptr(work), work.numel() * work.element_size(), st),
                  "mtcp_gpu_rto_send_dev")

    def rto_sweep(self, snd: np.ndarray, dtx: np.ndarray, cur_ts: int, cap: int):
        """mtcp_gpu_rto_sweep over `snd` and `dtx` ((max_id + 1) records each,
        updated in place); returns (rto, seg_sid, seg_start, seg_stop, total):
        rto and seg_sid cut to the handled streams, seg_start of cap + 1 and
        seg_stop of cap zeros, total = (due, handled)."""
        max_id = len(snd) - 1
        for a, dt, name in ((snd, ACK_STATE_DTYPE, "snd"), (dtx, DATAGEN_STATE_DTYPE, "dtx")):
            if a.dtype != dt or not a.flags.c_contiguous or len(a) != max_id + 1 or max_id < 0:
                raise ValueError(f"{name}: (max_id + 1) contiguous records of its dtype")
        n = max(cap, 1)
        rto, seg_sid = np.zeros(n, dtype=RTO_REC_DTYPE), np.zeros(n, dtype=np.uint32)
        seg_start, seg_stop = np.full(n + 1, 0xFFFFFFFF, dtype=np.uint32), np.full(n, 0xFFFFFFFF, dtype=np.uint32)
        nseg, total = np.zeros(1, dtype=np.uint32), np.zeros(2, dtype=np.uint64)
        check(lib().mtcp_gpu_rto_sweep(self._h, max_id, snd.ctypes.data, dtx.ctypes.data, cur_ts & 0xFFFFFFFF, cap,
                                       rto.ctypes.data, seg_sid.ctypes.data, seg_start.ctypes.data,
                                       seg_stop.ctypes.data, nseg.ctypes.data, total.ctypes.data),
              "mtcp_gpu_rto_sweep")
        m = int(nseg[0])
        return rto[:m], seg_sid[:m], seg_start, seg_stop, total

    # -- the payload copy behind the walk (tcp_ring_buffer.c:304-319; mtcp_gpu_rcvcopy.h) --
    @staticmethod
    def rcvcopy_work_bytes(n: int, max_id: int) -> int:
        """mtcp_gpu_rcvcopy_work_bytes (host only, needs no GPU)."""
        return lib().mtcp_gpu_rcvcopy_work_bytes(n, max_id)

    def rcvcopy_dev(self, buf, desc, off_shift: int, res, place, n: int, max_id: int, idx, seg_sid, seg_start, nseg,
                    seg_stop, rbuf, arena, cstat, work, stream=None) -> None:
        """buf, desc, off_shift: the chunk as rx_chunk_dev saw it; res: n x 40 B
        records; place, seg_stop: as rcvwalk_dev wrote them; idx, seg_sid,
        seg_start, nseg: as group_dev wrote them; rbuf: (max_id + 1) x 32 B
        (RCV_BUF_DTYPE), updated; arena: the receive buffers' bytes, written;
        cstat: n x u8; work: at least rcvcopy_work_bytes(n, max_id) bytes."""
        with self._ordered(stream) as st:
            check(lib().mtcp_gpu_rcvcopy_dev(self._h, _dptr(buf), buf.numel() * buf.element_size(), _dptr(desc),
                                             off_shift, _dptr(res), _dptr(place), n, max_id, _dptr(idx),
                                             _dptr(seg_sid), _dptr(seg_start), _dptr(nseg), _dptr(seg_stop),
                                             _dptr(rbuf), _dptr(arena), arena.numel() * arena.element_size(),
                                             _dptr(cstat), _dptr(work), work.numel() * work.element_size(), st),
                  "mtcp_gpu_rcvcopy_dev")

    # -- the application read out of the arena (api.c:1096-1149, tcp_ring_buffer.c:384-421; mtcp_gpu_rcvread.h) --
    @staticmethod
    def rcvread_work_bytes(n: int, max_id: int) -> int:
        """mtcp_gpu_rcvread_work_bytes (host only, needs no GPU)."""
        return lib().mtcp_gpu_rcvread_work_bytes(n, max_id)

    @staticmethod
    def rcvread_tile() -> int:
        return lib().mtcp_gpu_rcvread_tile()

    def rcvread_dev(self, req, n: int, max_id: int, state, rbuf, tx, snd, arena, dst, rres, total, work,
                    stream=None) -> None:
        """req: n x 32 B (RCVREAD_REQ_DTYPE); state: (max_id + 1) x 64 B and rbuf:
        x 32 B, updated; tx (x 32 B, byte 19 updated) and snd (x 128 B): both or
        neither None; arena: the receive buffers' bytes, read; dst: the
        destination region, written; rres: n x 16 B (RCVREAD_RES_DTYPE); total:
        2 x u64 (requests that copied, bytes); work: at least
        rcvread_work_bytes(n, max_id) bytes."""
        with self._ordered(stream) as st:
            check(lib().mtcp_gpu_rcvread_dev(self._h, _dptr(req), n, max_id, _dptr(state), _dptr(rbuf),
                                             None if tx is None else _dptr(tx), None if snd is None else _dptr(snd),
                                             _dptr(arena), arena.numel() * arena.element_size(), _dptr(dst),
                                             dst.numel() * dst.element_size(), _dptr(rres), _dptr(total), _dptr(work),
                                             work.numel() * work.element_size(), st), "mtcp_gpu_rcvread_dev")

    def rcvread(self, req: np.ndarray, max_id: int, state, rbuf, tx, snd, arena, dst: np.ndarray):
        """mtcp_gpu_rcvread: `req` in host memory, the mirrors and the arena GPU
        tensors as for rcvread_dev; the bytes read land in the host array
        `dst` (uint8, in place); returns (rres, total)."""
        req = np.ascontiguousarray(req, dtype=RCVREAD_REQ_DTYPE)
        if dst.dtype != np.uint8 or not dst.flags.c_contiguous:
            raise ValueError("dst: a contiguous uint8 array")
        n = len(req)
        rres, total = np.zeros(max(n, 1), dtype=RCVREAD_RES_DTYPE), np.zeros(2, dtype=np.uint64)
        check(lib().mtcp_gpu_rcvread(self._h, req.ctypes.data, n, max_id, _dptr(state), _dptr(rbuf),
                                     None if tx is None else _dptr(tx), None if snd is None else _dptr(snd),
                                     _dptr(arena), arena.numel() * arena.element_size(), dst.ctypes.data, dst.nbytes,
                                     rres.ctypes.data, total.ctypes.data), "mtcp_gpu_rcvread")
        return rres[:n], total

    # -- the application write into the send buffers (api.c:1416-1567, tcp_send_buffer.c:116-146; mtcp_gpu_sndwrite.h) --
    @staticmethod
    def sndwrite_work_bytes(n: int, max_id: int) -> int:
        """mtcp_gpu_sndwrite_work_bytes (host only, needs no GPU)."""
        return lib().mtcp_gpu_sndwrite_work_bytes(n, max_id)

    @staticmethod
    def sndwrite_tile() -> int:
        return lib().mtcp_gpu_sndwrite_tile()

    def sndwrite_dev(self, wreq, n: int, max_id: int, snd, dtx, src, payload, wres, seg_sid, seg_start, seg_stop,
                     nseg, total, work, src_bytes: int | None = None, payload_bytes: int | None = None,
                     stream=None) -> None:
        """wreq: n x 32 B (SNDWRITE_REQ_DTYPE); snd: (max_id + 1) x 128 B and dtx:
        x 16 B, updated; src: the source region, read (a tensor, or an int: the
        device-accessible address of registered host memory, with src_bytes);
        payload: the arena the send buffers live in, written; wres: n x 16 B
        (SNDWRITE_RES_DTYPE); seg_sid, seg_stop: n x u32; seg_start: (n + 1) x
        u32; nseg: 1 x u32; total: 2 x u64 (requests written, bytes); work: at
        least sndwrite_work_bytes(n, max_id) bytes."""
        sptr = src if isinstance(src, int) else _dptr(src)
        if src_bytes is None:
            src_bytes = src.numel() * src.element_size()
        if payload_bytes is None:
            payload_bytes = payload.numel() * payload.element_size()
        with self._ordered(stream) as st:
            check(lib().mtcp_gpu_sndwrite_dev(self._h, _dptr(wreq), n, max_id, _dptr(snd), _dptr(dtx), sptr, src_bytes,
                                              _dptr(payload), payload_bytes, _dptr(wres), _dptr(seg_sid),
                                              _dptr(seg_start), _dptr(seg_stop), _dptr(nseg), _dptr(total),
                                              _dptr(work), work.numel() * work.element_size(), st),
                  "mtcp_gpu_sndwrite_dev")

    def sndwrite(self, wreq: np.ndarray, max_id: int, snd, dtx, src: np.ndarray, payload):
        """mtcp_gpu_sndwrite: `wreq` and the source bytes `src` (uint8) in host
        memory, the mirrors and the arena GPU tensors as for sndwrite_dev;
        returns (wres, seg_sid, seg_start, seg_stop, nseg, total)."""
        wreq = np.ascontiguousarray(wreq, dtype=SNDWRITE_REQ_DTYPE)
        if src.dtype != np.uint8 or not src.flags.c_contiguous:
            raise ValueError("src: a contiguous uint8 array")
        n = len(wreq)
        k = max(n, 1)
        wres, total = np.zeros(k, dtype=SNDWRITE_RES_DTYPE), np.zeros(2, dtype=np.uint64)
        seg_sid, seg_start = np.zeros(k, dtype=np.uint32), np.full(k + 1, 0xFFFFFFFF, dtype=np.uint32)
        seg_stop, nseg = np.full(k, 0xFFFFFFFF, dtype=np.uint32), np.zeros(1, dtype=np.uint32)
        check(lib().mtcp_gpu_sndwrite(self._h, wreq.ctypes.data, n, max_id, _dptr(snd), _dptr(dtx), src.ctypes.data,
                                      src.nbytes, _dptr(payload), payload.numel() * payload.element_size(),
                                      wres.ctypes.data, seg_sid.ctypes.data, seg_start.ctypes.data,
                                      seg_stop.ctypes.data, nseg.ctypes.data, total.ctypes.data), "mtcp_gpu_sndwrite")
        return wres[:n], seg_sid[:n], seg_start[:n + 1], seg_stop[:n], nseg, total

    def write_send_dev(self, wreq, n: int, max_id: int, snd, dtx, src, payload, wres, seg_sid, seg_start, seg_stop,
                       nseg, wtotal, wwork, idx, state, tx, cur_ts: int, links, buf, buf_off: int, off_shift: int,
                       slot_bytes: int, seg, desc, seg_cap: int, dres, total, status, work, max_mss: int = 0,
                       flags: int = 0, buf_len: int | None = None, stream=None) -> None:
        """sndwrite_dev, then data_send_dev over the table the write made (ack and
        ack_stop None, n bursts), on one stream.  idx: n x u32, any values;
        wtotal, wwork: the write's totals and workspace; total, work: the data
        send's (at least datagen_work_bytes(n, max_id) bytes)."""
        room = buf.numel() * buf.element_size()
        if buf_len is not None and not 0 <= buf_len <= room:
            raise ValueError("buf_len: at most the bytes of buf")
        with self._ordered(stream) as st:
            check(lib().mtcp_gpu_write_send_dev(self._h, _dptr(wreq), n, max_id, _dptr(snd), _dptr(dtx), _dptr(src),
                                                src.numel() * src.element_size(), _dptr(payload),
                                                payload.numel() * payload.element_size(), _dptr(wres), _dptr(seg_sid),
                                                _dptr(seg_start), _dptr(seg_stop), _dptr(nseg), _dptr(wtotal),
                                                _dptr(wwork), wwork.numel() * wwork.element_size(), _dptr(idx),
                                                _dptr(state), _dptr(tx), cur_ts & 0xFFFFFFFF, _dptr(links),
                                                links.numel() * links.element_size() // 12, _dptr(buf), buf_off,
                                                room if buf_len is None else buf_len, off_shift, slot_bytes, max_mss,
                                                flags, _dptr(seg), _dptr(desc), seg_cap, _dptr(dres), _dptr(total),
                                                _dptr(status), _dptr(work), work.numel() * work.element_size(), st),
                  "mtcp_gpu_write_send_dev")

    # -- tx frames from segment records (tcp_out.c:135-354; mtcp_gpu_txbuild.h) --
    def tx_build_dev(self, seg, n: int, payload, links, buf, desc, off_shift: int, status,
                     max_mss: int = 0, flags: int = 0, stream=None) -> None:
        """seg: n x 48 B (TX_SEG_DTYPE); payload: the bytes payload_off points
        into; links: 12 B entries (TX_LINK_DTYPE); buf: the frames' image, of
        which only built frames' bytes are written; desc: the slots; status:
        n x u8."""
        with self._ordered(stream) as st:
            check(lib().mtcp_gpu_tx_build_dev(self._h, _dptr(seg), n, _dptr(payload),
                                              payload.numel() * payload.element_size(), _dptr(links),
                                              links.numel() * links.element_size() // 12, _dptr(buf),
                                              buf.numel() * buf.element_size(), _dptr(desc), off_shift,
                                              max_mss, flags, _dptr(status), st), "mtcp_gpu_tx_build_dev")

    def tx_build(self, seg: np.ndarray, payload: np.ndarray, links: np.ndarray, buf: np.ndarray,
                 desc: np.ndarray, off_shift: int = 0, max_mss: int = 0, flags: int = 0,
                 status: np.ndarray | None = None) -> tuple[np.ndarray, int]:
        """mtcp_gpu_tx_build: builds into the host array `buf` in place;
        returns (status, n_built)."""
        seg = np.ascontiguousarray(seg, dtype=TX_SEG_DTYPE)
        links = np.ascontiguousarray(links, dtype=TX_LINK_DTYPE)
        desc = np.ascontiguousarray(desc, dtype=DESC_DTYPE)
        if status is None:
            status = np.zeros(len(seg), dtype=np.uint8)
        cnt = ctypes.c_uint32(0)
        check(lib().mtcp_gpu_tx_build(self._h, seg.ctypes.data, len(seg), payload.ctypes.data, payload.nbytes,
                                      links.ctypes.data, len(links), buf.ctypes.data, buf.nbytes,
                                      desc.ctypes.data, off_shift, max_mss, flags,
                                      status.ctypes.data, ctypes.byref(cnt)), "mtcp_gpu_tx_build")
        return status, cnt.value

    # -- tx segments from send bursts (tcp_out.c:357-449, :587-674; mtcp_gpu_txseg.h) --
    @staticmethod
    def tx_segment_tile() -> int:
        return lib().mtcp_gpu_tx_segment_tile()

    @staticmethod
    def tx_segment_work_bytes(n_burst: int) -> int:
        return lib().mtcp_gpu_tx_segment_work_bytes(n_burst)

    @staticmethod
    def tx_segment_plan(burst: np.ndarray, payload_bytes: int, n_links: int, buf_off: int, buf_len: int,
                        off_shift: int, slot_bytes: int, seg_cap: int,
                        max_mss: int = 0) -> tuple[np.ndarray, np.ndarray]:
        """mtcp_gpu_tx_segment_plan (host only, no GPU): (results, total[2])."""
        burst = np.ascontiguousarray(burst, dtype=TX_BURST_DTYPE)
        res = np.zeros(len(burst), dtype=TX_BURST_RESULT_DTYPE)
        total = np.zeros(2, dtype=np.uint64)
        check(lib().mtcp_gpu_tx_segment_plan(burst.ctypes.data, len(burst), payload_bytes, n_links, buf_off,
                                             buf_len, off_shift, slot_bytes, seg_cap, max_mss, res.ctypes.data,
                                             total.ctypes.data), "mtcp_gpu_tx_segment_plan")
        return res, total

    def tx_segment_dev(self, burst, n_burst: int, payload_bytes: int, n_links: int, buf_off: int, buf_len: int,
                       off_shift: int, slot_bytes: int, seg, desc, seg_cap: int, res, total, work,
                       max_mss: int = 0, stream=None) -> None:
        """burst: n_burst x 64 B (TX_BURST_DTYPE); seg: seg_cap x 48 B; desc:
        seg_cap x 8 B; res: n_burst x 16 B (TX_BURST_RESULT_DTYPE); total:
        2 x u64; work: at least tx_segment_work_bytes(n_burst) bytes, 16 B aligned."""
        with self._ordered(stream) as st:
            check(lib().mtcp_gpu_tx_segment_dev(self._h, _dptr(burst), n_burst, payload_bytes, n_links, buf_off,
                                                buf_len, off_shift, slot_bytes, max_mss, _dptr(seg), _dptr(desc),
                                                seg_cap, _dptr(res), _dptr(total), _dptr(work),
                                                work.numel() * work.element_size(), st),
                  "mtcp_gpu_tx_segment_dev")

    def tx_send_dev(self, burst, n_burst: int, payload, links, buf, buf_off: int, off_shift: int,
                    slot_bytes: int, seg, desc, seg_cap: int, res, total, status, work,
                    max_mss: int = 0, flags: int = 0, stream=None) -> None:
        """tx_segment_dev, then tx_build_dev over all seg_cap records, on one stream."""
        with self._ordered(stream) as st:
            check(lib().mtcp_gpu_tx_send_dev(self._h, _dptr(burst), n_burst, _dptr(payload),
                                             payload.numel() * payload.element_size(), _dptr(links),
                                             links.numel() * links.element_size() // 12, _dptr(buf), buf_off,
                                             buf.numel() * buf.element_size(), off_shift, slot_bytes, max_mss,
                                             flags, _dptr(seg), _dptr(desc), seg_cap, _dptr(res), _dptr(total),
                                             _dptr(status), _dptr(work), work.numel() * work.element_size(), st),
                  "mtcp_gpu_tx_send_dev")

    def tx_send(self, burst: np.ndarray, payload: np.ndarray, links: np.ndarray, buf: np.ndarray,
                seg_cap: int, buf_off: int = 0, off_shift: int = 0, slot_bytes: int = 0, max_mss: int = 0,
                flags: int = 0, desc: np.ndarray | None = None, res: np.ndarray | None = None,
                status: np.ndarray | None = None):
        """mtcp_gpu_tx_send: builds into the host array `buf` in place;
        returns (desc, res, total, status)."""
        burst = np.ascontiguousarray(burst, dtype=TX_BURST_DTYPE)
        links = np.ascontiguousarray(links, dtype=TX_LINK_DTYPE)
        if desc is None:
            desc = np.zeros(seg_cap, dtype=DESC_DTYPE)
        if res is None:
            res = np.zeros(len(burst), dtype=TX_BURST_RESULT_DTYPE)
        if status is None:
            status = np.zeros(seg_cap, dtype=np.uint8)
        total = np.zeros(2, dtype=np.uint64)
        check(lib().mtcp_gpu_tx_send(self._h, burst.ctypes.data, len(burst), payload.ctypes.data, payload.nbytes,
                                     links.ctypes.data, len(links), buf.ctypes.data, buf_off, buf.nbytes,
                                     off_shift, slot_bytes, max_mss, flags, desc.ctypes.data, seg_cap,
                                     res.ctypes.data, total.ctypes.data, status.ctypes.data), "mtcp_gpu_tx_send")
        return desc, res, total, status

    # -- RSS-friendly address pool (mtcp/src/addr_pool.c:103-180) ------------
    def rss_queue_map_dev(self, saddr_base_h: int, num_addr: int, daddr_h: int, dport_h: int,
                          num_queues: int, endian_check: bool, queue, stream=None) -> None:
        if queue.numel() * queue.element_size() < num_addr * (MAX_PORT - MIN_PORT):
            raise ValueError("queue buffer too small")
        with self._ordered(stream) as st:
            check(lib().mtcp_gpu_rss_queue_map_dev(self._h, saddr_base_h, num_addr, daddr_h, dport_h,
                                                   num_queues, int(endian_check), _dptr(queue),
                                                   st),
                  "mtcp_gpu_rss_queue_map_dev")

    def addr_pool_search(self, core: int, num_queues: int, saddr_base: int, num_addr: int,
                         daddr: int, dport: int, endian_check: bool = True,
                         max_out: int | None = None) -> np.ndarray:
        """CreateAddressPoolPerCore's entries for `core` (network-order arguments,
        as the reference's); returns the ADDR_ENTRY_DTYPE records in pool order."""
        if max_out is None:
            max_out = num_addr * (MAX_PORT - MIN_PORT) // max(num_queues, 1)
        out = np.zeros(max(max_out, 1), dtype=ADDR_ENTRY_DTYPE)
        found = ctypes.c_uint32(0)
        check(lib().mtcp_gpu_addr_pool_search(self._h, core, num_queues, saddr_base, num_addr,
                                              daddr, dport, int(endian_check), out.ctypes.data,
                                              max_out, ctypes.byref(found)),
              "mtcp_gpu_addr_pool_search")
        return out[:min(found.value, max_out)]


class FlowTable:
    """One mtcp_gpu_flowtab (include/mtcp_gpu_flowtab.h): the device mirror of
    a tcp_flow_table (mtcp/src/fhash.c:16-121) bound to `ctx`.  Close it
    before its context."""

    def __init__(self, ctx: Context, cap_log2: int):
        self._h = ctypes.c_void_p()
        self.ctx = ctx
        check(lib().mtcp_gpu_flowtab_create(ctx._h, cap_log2, ctypes.byref(self._h)), "mtcp_gpu_flowtab_create")

    @staticmethod
    def home(key12: bytes, cap_log2: int) -> int:
        """mtcp_gpu_flowtab_home (host only, needs no GPU)."""
        b = (ctypes.c_uint8 * 12).from_buffer_copy(key12)
        return lib().mtcp_gpu_flowtab_home(ctypes.cast(b, ctypes.c_void_p), cap_log2)

    @property
    def capacity(self) -> int:
        return lib().mtcp_gpu_flowtab_capacity(self._h)

    def close(self) -> None:
        if self._h:
            lib().mtcp_gpu_flowtab_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def update_dev(self, dele, n_del: int, ins, n_ins: int, stream=None) -> None:
        """dele / ins: n x 16 B (FLOW_ENTRY_DTYPE) on the device, or None with a
        count of 0; removes run first."""
        with self.ctx._ordered(stream) as st:
            check(lib().mtcp_gpu_flowtab_update_dev(self._h, None if dele is None else _dptr(dele), n_del,
                                                    None if ins is None else _dptr(ins), n_ins, st),
                  "mtcp_gpu_flowtab_update_dev")

    def lookup_dev(self, res, n: int, sid, bins=None, stream=None) -> None:
        """res: n x 40 B rx records; sid: n x u32; bins: n x u32 or None."""
        with self.ctx._ordered(stream) as st:
            check(lib().mtcp_gpu_flowtab_lookup_dev(self._h, _dptr(res), n, _dptr(sid),
                                                    None if bins is None else _dptr(bins), st),
                  "mtcp_gpu_flowtab_lookup_dev")

    def update(self, dele: np.ndarray | None = None, ins: np.ndarray | None = None) -> None:
        """mtcp_gpu_flowtab_update: entries in host memory, removes first."""
        dele = np.zeros(0, FLOW_ENTRY_DTYPE) if dele is None else np.ascontiguousarray(dele, dtype=FLOW_ENTRY_DTYPE)
        ins = np.zeros(0, FLOW_ENTRY_DTYPE) if ins is None else np.ascontiguousarray(ins, dtype=FLOW_ENTRY_DTYPE)
        check(lib().mtcp_gpu_flowtab_update(self._h, dele.ctypes.data if len(dele) else None, len(dele),
                                            ins.ctypes.data if len(ins) else None, len(ins)),
              "mtcp_gpu_flowtab_update")

    def lookup(self, res: np.ndarray, bins: bool = False):
        """mtcp_gpu_flowtab_lookup: sid, or (sid, bins), of 40 B records in host memory."""
        res = np.ascontiguousarray(res, dtype=RESULT_DTYPE)
        sid = np.zeros(len(res), dtype=np.uint32)
        b = np.zeros(len(res), dtype=np.uint32) if bins else None
        check(lib().mtcp_gpu_flowtab_lookup(self._h, res.ctypes.data, len(res), sid.ctypes.data,
                                            b.ctypes.data if bins else None), "mtcp_gpu_flowtab_lookup")
        return (sid, b) if bins else sid

    def stats(self) -> dict:
        c = np.zeros(1, dtype=FLOWTAB_COUNTERS_DTYPE)
        check(lib().mtcp_gpu_flowtab_stats(self._h, c.ctypes.data), "mtcp_gpu_flowtab_stats")
        return {f: int(c[f][0]) for f in FLOWTAB_COUNTERS_DTYPE.names}

    def rehash(self) -> None:
        check(lib().mtcp_gpu_flowtab_rehash(self._h), "mtcp_gpu_flowtab_rehash")


def parse_cpulist(text: str) -> set[int]:
    """The kernel's cpulist format ("0-3,8,10-11") as a set of cpu ids."""
    cpus: set[int] = set()
    for part in text.strip().split(","):
        part = part.strip()
        if not part:
            continue
        lo, _, hi = part.partition("-")
        cpus.update(range(int(lo), int(hi or lo) + 1))
    return cpus


def device_pci_bus_id(device: int) -> str:
    """PCI address of `device` ("0000:a7:00.0"), lower case as sysfs names it."""
    buf = ctypes.create_string_buffer(64)
    check(lib().mtcp_gpu_device_pci_bus_id(device, buf, len(buf)), "mtcp_gpu_device_pci_bus_id")
    return buf.value.decode().lower()


def device_local_cpus(device: int, sysfs: str = "/sys") -> tuple[str, set[int]]:
    """The cpus on `device`'s side of the host (sysfs
    bus/pci/devices/<bdf>/local_cpulist): where a process that stages frames
    for this GPU should run so that its host buffers (first-touched by it) sit
    on the GPU's socket.  mTCP keeps each thread and its memory on one node
    the same way (mtcp_core_affinitize, mtcp/src/cpu.c:54-79; DPDK queues on
    the NIC's socket, dpdk_module.c:660-663; gpu_module.c picks the GPU by the
    thread's node, gpu_topo.h).  An empty set when sysfs does not tell."""
    bdf = device_pci_bus_id(device)
    try:
        with open(os.path.join(sysfs, "bus", "pci", "devices", bdf, "local_cpulist")) as f:
            return bdf, parse_cpulist(f.read())
    except (OSError, ValueError):
        return bdf, set()


def host_register(arr: np.ndarray) -> None:
    check(lib().mtcp_gpu_host_register(arr.ctypes.data, arr.nbytes), "mtcp_gpu_host_register")


def host_unregister(arr: np.ndarray) -> None:
    check(lib().mtcp_gpu_host_unregister(arr.ctypes.data), "mtcp_gpu_host_unregister")


def pktgen_dev(buf, desc, n: int, off_shift: int, seed: int, first_index: int = 0,
               stream=None) -> None:
    """Synthetic frames on the GPU (include/mtcp_gpu_pktgen.h)."""
    check(lib().mtcp_gpu_pktgen_dev(_dptr(buf), buf.numel() * buf.element_size(), _dptr(desc),
                                    n, off_shift, seed, first_index, _stream_handle(stream)),
          "mtcp_gpu_pktgen_dev")


def results_view(t) -> np.ndarray:
    """A device result buffer (uint8 tensor of n*40 bytes) as a numpy record array."""
    return t.cpu().numpy().view(RESULT_DTYPE)
