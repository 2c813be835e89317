"""Regenerate tests/golden/sndwrite_cases.bin with the reference's own code.

    python tests/make_sndwrite_golden.py REFERENCE_ROOT      (or REF=... in the environment, as oracle/Makefile)

Compiles tests/c/ref_sndwrite_gen.c (own text; the reference's headers only by
path) with the reference's tcp_send_buffer.c, memory_mgt.c and tcp_sb_queue.c
into a temporary directory, with the flags the oracle's reference build uses,
and runs it.  Needs the reference's sources; the tests that read the fixture
(tests/test_sndwrite_model.py, tests/test_sndwrite_step_rules.py,
tests/test_gpu_sndwrite.py) do not.
"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the REFFLAGS of oracle/Makefile (mtcp/src/Makefile.in:20-31)
REFFLAGS = ("-m64 -fPIC -fgnu89-inline -fcommon -DNDEBUG -O3 -DNETSTAT -DINFO -DDBGERR -DDBGCERR -DDISABLE_HWCSUM "
            "-DDISABLE_PSIO -DDISABLE_NETMAP -DDISABLE_DPDK -w").split()


def main(ref):
    src = os.path.join(ref, "mtcp", "src")
    inc = ["-I" + os.path.join(src, "include"), "-I" + os.path.join(ref, "io_engine", "include")]
    out = os.path.join(ROOT, "tests", "golden", "sndwrite_cases.bin")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "ref_sndwrite_gen")
        subprocess.run(["gcc", *REFFLAGS, *inc, os.path.join(ROOT, "tests", "c", "ref_sndwrite_gen.c"),
                        *(os.path.join(src, f) for f in ("tcp_send_buffer.c", "memory_mgt.c", "tcp_sb_queue.c")),
                        "-pthread", "-o", exe], check=True)
        subprocess.run([exe, out], check=True)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ["REF"])
