"""HandleRTO's step function (mtcp_amd/csrc/rto_step.hpp, the text the sweep
kernels run) on the CPU under AddressSanitizer and UBSan:
tests/c/rto_step_test.cpp, a stand-alone program, drives it over every stream of
every CheckRtmTimeout call of tests/golden/rtosweep_cases.bin (the due test, the
fields after, the reference's call counts) and over records of random bytes
(BAD records, every tcp_state, any nrtx) against a second literal restatement
of the header's contract.  -fno-sanitize-recover: a shift past the width, a
signed overflow or a read past the fixture would end the program."""
import json
import os
import subprocess

from tests import rtosweep_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "rtosweep_cases.bin")


def test_rto_step_rules(tmp_path):
    exe = tmp_path / "rto_step_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-o", str(exe), os.path.join(ROOT, "tests", "c", "rto_step_test.cpp")], check=True)
    p = subprocess.run([str(exe), FIXTURE], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stdout[-300:], p.stderr[-2000:])
    r = json.loads(p.stdout.strip())
    checks = sum(len(c["before"]) * len(c["calls"]) for c in rm.load_fixture())
    assert r == {"fixture": {"cases": checks, "bad": 0, "first_line": 0},
                 "random": {"cases": 2_000_000, "bad": 0, "first_line": 0}}
