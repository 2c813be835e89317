"""The ACK generation's step text (mtcp_amd/csrc/ackgen_step.hpp, what the
kernels run) on the CPU under AddressSanitizer and UBSan:
tests/c/ackgen_step_test.cpp, a stand-alone program, drives it over every case
of tests/golden/ackgen_cases.bin (every record field against the reference's
frame bytes, the stream after, the ack list) and over tx records, states and
placement words of random bytes (the wave's fold over masks equals the fold
packet by packet, a BAD stream changes nothing, the fixed bytes never change,
the emitted records are a prefix of the planned ones).
-fno-sanitize-recover: a shift past the width or a read past the fixture would
end the program; they are what the BAD test has to fence off."""
import json
import os
import struct
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ackgen_cases.bin")


def test_ackgen_step_rules(tmp_path):
    exe = tmp_path / "ackgen_step_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-o", str(exe), os.path.join(ROOT, "tests", "c", "ackgen_step_test.cpp")], check=True)
    p = subprocess.run([str(exe), FIXTURE], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stdout[-300:], p.stderr[-2000:])
    r = json.loads(p.stdout.strip())
    with open(FIXTURE, "rb") as f:
        cases = struct.unpack("<4I", f.read(16))[2]
    assert r == {"fixture": {"cases": 2 * cases, "bad": 0, "first_line": 0},
                 "random": {"cases": 1_000_000, "bad": 0, "first_line": 0}}
