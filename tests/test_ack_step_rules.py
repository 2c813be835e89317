"""ProcessACK's step function (mtcp_amd/csrc/ack_step.hpp, the text the walk
kernels run) on the CPU under AddressSanitizer and UBSan:
tests/c/ack_step_test.cpp, a stand-alone program, drives it over every walk of
tests/golden/ackwalk_cases.bin (the state after every packet, the bytes that
left the send buffer, the reference's call counts) and over states and inputs
of random bytes (a deferred packet changes nothing, the fixed bytes never
change).  -fno-sanitize-recover: a signed overflow, a division by zero, a shift
past the width or a read past the fixture would end the program; they are what
DEFER_ARITH and the BAD test have to fence off."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ackwalk_cases.bin")


def test_ack_step_rules(tmp_path):
    exe = tmp_path / "ack_step_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-o", str(exe), os.path.join(ROOT, "tests", "c", "ack_step_test.cpp")], check=True)
    p = subprocess.run([str(exe), FIXTURE], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stdout[-300:], p.stderr[-2000:])
    r = json.loads(p.stdout.strip())
    walks = (os.path.getsize(FIXTURE) - 16) // (96 + 16 * 112)
    assert r == {"fixture": {"cases": 16 * walks, "bad": 0, "first_line": 0},
                 "random": {"cases": 2_000_000, "bad": 0, "first_line": 0}}
