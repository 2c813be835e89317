"""The data generation's step text (mtcp_amd/csrc/datagen_step.hpp, what the
kernels run) on the CPU under AddressSanitizer and UBSan:
tests/c/datagen_step_test.cpp, a stand-alone program, drives it over every
stream of every case of tests/golden/datagen_cases.bin (the records after, ret,
the frames' count and payload bytes, the RTO list, the window probe) and over
records and flag words of random bytes (the wave's ballot fold equals the fold
packet by packet, a BAD stream changes nothing and a BAD_BURST stream nothing
but on_send_list, which takes the fold's value; the fixed bytes never change).  -fno-sanitize-recover: a shift past the width or a read past
the fixture would end the program; they are what the BAD test has to fence
off."""
import json
import os
import subprocess

from tests import datagen_model as dm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_datagen_step_rules(tmp_path):
    exe = tmp_path / "datagen_step_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-o", str(exe), os.path.join(ROOT, "tests", "c", "datagen_step_test.cpp")], check=True)
    p = subprocess.run([str(exe), dm.FIXTURE], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stdout[-300:], p.stderr[-2000:])
    r = json.loads(p.stdout.strip())
    streams = sum(len(c["streams"]) for c in dm.load_fixture())
    assert r == {"fixture": {"cases": streams, "bad": 0, "first_line": 0},
                 "random": {"cases": 1_000_000, "bad": 0, "first_line": 0}}
