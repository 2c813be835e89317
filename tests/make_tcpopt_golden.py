"""Writes tests/golden/tcpopt_cases.bin: NCASES random option blocks
(tests/tcpopt_model.py gen_block) with both option walks' outputs as the
REFERENCE returned them (ParseTCPTimestamp / ParseTCPOptions of
oracle/_ref/libref_rx.so, mtcp/src/tcp_util.c:14-92).  A walk the restatement
marks as never returning is stored flagged and is not passed to the reference.

Needs oracle/_ref (built where the reference tree is present):
    python -m tests.make_tcpopt_golden
"""
import numpy as np

import oracle
from tests import tcpopt_model as m

SEED = 20260515


def main() -> None:
    if not oracle.ref_available():
        raise SystemExit("oracle/_ref/libref_rx.so is missing: `make ref` where the reference tree is")
    ref = m.RefWalks()
    cases = np.zeros(m.NCASES, dtype=m.CASE_DTYPE)
    for c, (length, b) in zip(cases, m.gen_blocks(m.NCASES, SEED)):
        c["len"], c["bytes"] = length, b
        nonterm = (1 if m.walk_ts(b, length)["nonterm"] else 0) | (2 if m.walk_syn(b, length)["nonterm"] else 0)
        c["nonterm"] = nonterm
        if not nonterm & 1:
            t = ref.ts_walk(b, length)
            c["ts_ret"], c["ts_val"], c["ts_ref"] = t["ret"], t["ts_val"], t["ts_ref"]
        if not nonterm & 2:
            s = ref.syn_walk(b, length)
            for k in m.SYN_KEYS:
                c[k] = s[k]
    cases.tofile(m.FIXTURE)
    print(f"{m.FIXTURE}: {len(cases)} cases, {cases.nbytes} bytes")


if __name__ == "__main__":
    main()
