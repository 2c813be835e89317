"""mtcp_amd — MI355X (gfx950) offload of mTCP's software (--disable-hwcsum)
per-packet path: IPv4/TCP checksums, Eth/IP/TCP header parse + rx verdict,
RSS Toeplitz hash, tx checksum fill.

The product is libmtcp_gpu.so (HIP kernels + the C ABI of include/mtcp_gpu.h);
this package is its Python view for tests and benchmarks.
"""
from ._types import (RCVREAD_REQ_DTYPE, RCVREAD_RES_DTYPE, RCVREAD_VERDICTS, RTO_REC_DTYPE, RTO_VERDICTS, DATAGEN_RES_DTYPE, DATAGEN_STATE_DTYPE, DATAGEN_STATUS, ACKGEN_RES_DTYPE, ACKGEN_STATE_DTYPE, ACKGEN_STATUS, ACK_REC_DTYPE, ACK_STATE_DTYPE, ACK_VERDICTS, DESC_DTYPE, FLOW_ENTRY_DTYPE, FLOW_MISS, FLOW_NONE, RESULT16_DTYPE, RESULT_DTYPE, RCV_PLACE_DTYPE, RCV_STATE_DTYPE,  # noqa: F401
                     RCV_BUF_DTYPE, RCVCOPY_STATS, RCV_VERDICTS, RX_ERROR_VERDICTS,
                     STEER_DROP_BAD, TCPOPT_DTYPE, TX_BURST_DTYPE, TX_BURST_RESULT_DTYPE, TX_LINK_DTYPE,
                     TX_SEG_DTYPE, VERDICTS, compact_of)
from . import pktgen  # noqa: F401

__all__ = ["DESC_DTYPE", "FLOW_ENTRY_DTYPE", "FLOW_MISS", "FLOW_NONE", "RESULT_DTYPE", "RESULT16_DTYPE", "VERDICTS", "RX_ERROR_VERDICTS",
           "STEER_DROP_BAD", "TCPOPT_DTYPE", "TX_SEG_DTYPE", "TX_LINK_DTYPE", "TX_BURST_DTYPE",
           "TX_BURST_RESULT_DTYPE", "RCV_STATE_DTYPE", "RCV_PLACE_DTYPE", "RCV_VERDICTS", "RCV_BUF_DTYPE", "RCVCOPY_STATS", "ACK_STATE_DTYPE", "ACK_REC_DTYPE", "ACK_VERDICTS", "ACKGEN_STATE_DTYPE", "ACKGEN_RES_DTYPE", "ACKGEN_STATUS", "DATAGEN_STATE_DTYPE", "DATAGEN_RES_DTYPE", "DATAGEN_STATUS", "RTO_REC_DTYPE", "RTO_VERDICTS", "RCVREAD_REQ_DTYPE", "RCVREAD_RES_DTYPE", "RCVREAD_VERDICTS", "compact_of", "pktgen"]
# `from mtcp_amd import gpu` loads libmtcp_gpu.so (and raises if it was not built).
