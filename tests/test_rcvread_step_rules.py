"""The read's step function (mtcp_amd/csrc/rcvread_step.hpp, the text the plan
kernel runs) on the CPU under AddressSanitizer and UBSan:
tests/c/rcvread_step_test.cpp, a stand-alone program, drives it over every read
and peek of tests/golden/rcvread_cases.bin (the returned length and bytes, the
records after, the flags) with the arena and the destination as heap blocks of
exact size, and over batches of records of random bytes (BAD records, every
tcp_state, duplicates, ranges at the destination's end) against a second literal
restatement of the header's contract.  -fno-sanitize-recover: a shift past the
width, a signed overflow or a read past a block would end the program."""
import json
import os
import subprocess

from tests import rcvread_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rcvread_step_rules(tmp_path):
    exe = tmp_path / "rcvread_step_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-o", str(exe), os.path.join(ROOT, "tests", "c", "rcvread_step_test.cpp")], check=True)
    p = subprocess.run([str(exe), rm.FIXTURE], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stdout[-300:], p.stderr[-2000:])
    r = json.loads(p.stdout.strip())
    reads = sum(ev["kind"] != "put" for c in rm.load_fixture() for ev in c["events"])
    assert r == {"fixture": {"cases": reads, "bad": 0, "first_line": 0},
                 "random": {"cases": 100_000, "bad": 0, "first_line": 0}}
