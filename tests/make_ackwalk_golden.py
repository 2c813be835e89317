"""Regenerate tests/golden/ackwalk_cases.bin with the reference's own code.

    python tests/make_ackwalk_golden.py REFERENCE_ROOT      (or REF=... in the environment, as oracle/Makefile)

Compiles tests/c/ref_ackwalk_gen.c (own text; the reference's tcp_in.c only by
path) with the reference's tcp_send_buffer.c, timer.c, tcp_util.c,
tcp_ring_buffer.c, memory_mgt.c, tcp_rb_frag_queue.c and tcp_sb_queue.c into a
temporary directory, with the flags the oracle's reference build uses, and runs
it.  Needs the reference's sources; the test that reads the fixture
(tests/test_ackwalk_model.py) does not.
"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WALKS = 552                # 16 packets each, 112 B a packet: the fixture stays under 1 MiB
# the REFFLAGS of oracle/Makefile (mtcp/src/Makefile.in:20-31), as tests/make_rcvwalk_golden.py
REFFLAGS = ("-m64 -fPIC -fgnu89-inline -fcommon -DNDEBUG -O3 -DNETSTAT -DINFO -DDBGERR -DDBGCERR -DDISABLE_HWCSUM "
            "-DDISABLE_PSIO -DDISABLE_NETMAP -DDISABLE_DPDK -w").split()
LINKED = ("tcp_send_buffer.c", "timer.c", "tcp_util.c", "tcp_ring_buffer.c", "memory_mgt.c", "tcp_rb_frag_queue.c",
          "tcp_sb_queue.c")


def main(ref):
    src = os.path.join(ref, "mtcp", "src")
    inc = ["-I" + os.path.join(src, "include"), "-I" + os.path.join(ref, "io_engine", "include")]
    out = os.path.join(ROOT, "tests", "golden", "ackwalk_cases.bin")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "ref_ackwalk_gen")
        stubs = os.path.join(tmp, "stubs.o")
        subprocess.run(["gcc", "-O2", "-c", os.path.join(ROOT, "tests", "c", "ref_ackwalk_stubs.c"), "-o", stubs],
                       check=True)
        subprocess.run(["gcc", *REFFLAGS, *inc, '-DREF_TCP_IN_C="%s"' % os.path.join(src, "tcp_in.c"),
                        os.path.join(ROOT, "tests", "c", "ref_ackwalk_gen.c"),
                        *(os.path.join(src, f) for f in LINKED), stubs, "-pthread", "-o", exe], check=True)
        subprocess.run([exe, out, str(WALKS)], check=True)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ["REF"])
