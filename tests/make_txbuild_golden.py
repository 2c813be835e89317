"""Writes tests/golden/txbuild_frames.0.bin and .1.bin: the TCP frames that
mTCP's own SendTCPPacketStandalone / IPOutputStandalone / EthernetOutput chain
(tcp_out.c:135-222, ip_out.c:35-97, eth_out.c:35-80) builds and checksums in
`oracle/_ref/dropin_tx OUT 4096 observe` with MTCP_GPU_TX=0 (dev_ioctl answers
-1: the reference fills both checks itself).  The protocol-6 records are kept,
in send order, as one stream of `u16 len | frame`: 4 054 frames, 1 784 508
bytes, data written by the reference's code.  The stream is cut at a record
boundary into two files, each below 1 MiB.

Needs oracle/_ref (built where the reference tree is present):
    python -m tests.make_txbuild_golden
"""
import os
import subprocess
import tempfile

import numpy as np

from tests import txbuild_model as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE_TX = os.path.join(ROOT, "oracle", "_ref", "dropin_tx")
TX_SLOT = 2048          # one record of dropin_tx's output: u16 len at 0, the frame at 8


def reference_stream() -> np.ndarray:
    """A fresh run's protocol-6 frames as the fixture's stream."""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "tx.bin")
        env = dict(os.environ, MTCP_GPU_TX="0", MTCP_GPU_PIPELINE="1")
        p = subprocess.run([EXE_TX, out, "4096", "observe"], capture_output=True, text=True, timeout=300, env=env)
        if p.returncode != 0:
            raise RuntimeError(p.stderr[-3000:])
        recs = np.fromfile(out, dtype=np.uint8).reshape(-1, TX_SLOT)
    parts = []
    for r in recs:
        n = int(r[0]) | (int(r[1]) << 8)
        if r[8 + 12] == 0x08 and r[8 + 13] == 0x00 and r[8 + 23] == 6:
            parts.append(r[0:2])
            parts.append(r[8:8 + n])
    return np.concatenate(parts)


def split(stream: np.ndarray) -> list:
    """The stream cut after the last record that ends within the first 1 MiB."""
    at = 0
    while True:
        nxt = at + 2 + (int(stream[at]) | (int(stream[at + 1]) << 8))
        if nxt > m.PART_LIMIT:
            break
        at = nxt
    return [stream[:at], stream[at:]]


def main() -> None:
    if not os.path.exists(EXE_TX):
        raise SystemExit("oracle/_ref/dropin_tx is missing: `make ref` where the reference tree is")
    stream = reference_stream()
    frames = m.parse_stream(stream)
    assert (len(frames), len(stream)) == (m.FIXTURE_FRAMES, m.FIXTURE_BYTES), (len(frames), len(stream))
    for path, part in zip(m.FIXTURE_PARTS, split(stream)):
        assert len(part) < m.PART_LIMIT
        part.tofile(path)
        print(f"{path}: {len(part)} bytes")


if __name__ == "__main__":
    main()
