"""The write's step function (mtcp_amd/csrc/sndwrite_step.hpp, the text the plan
kernel runs) on the CPU under AddressSanitizer and UBSan:
tests/c/sndwrite_step_test.cpp, a stand-alone program with its own main, run
directly.  It drives the step over every SBPut and SBRemove of
tests/golden/sndwrite_cases.bin (the return value, the offsets, head_seq and every
byte of the chunk, the chunk a heap block of exact size) and over 100 000
batches of records of random bytes (BAD records, every tcp_state, duplicates,
snd_wnd at 0, 1, 2^31 - 1, 2^31 and 2^32 - 1, len at 0, 1 and 2^31 - 1) against a
second literal restatement of the header's contract.  -fno-sanitize-recover: a
shift past the width, a signed overflow or an access past a block would end the
program."""
import json
import os
import subprocess

from tests import sndwrite_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sndwrite_step_rules(tmp_path):
    exe = tmp_path / "sndwrite_step_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-o", str(exe), os.path.join(ROOT, "tests", "c", "sndwrite_step_test.cpp")], check=True)
    p = subprocess.run([str(exe), sm.FIXTURE], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stdout[-300:], p.stderr[-2000:])
    r = json.loads(p.stdout.strip())
    ops = sum(len(c["ops"]) for c in sm.load_fixture())
    assert r == {"fixture": {"cases": ops, "bad": 0, "first_line": 0},
                 "random": {"cases": 100_000, "bad": 0, "first_line": 0}}
