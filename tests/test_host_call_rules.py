"""The wait-limit contract of the host-memory calls (mtcp_amd/csrc/host_call.hpp:
Stage's pending list, HostCall) on the CPU: tests/c/host_call_test.cpp drives
them with a backend that records every queued copy and performs it only when
drained, under AddressSanitizer and UBSan, with the bounce buffers as heap
blocks of exact size.  Two inputs and two outputs of 0, 1, 15, 16 and 17 bytes:
an unbounded call's copies name the caller's own pointers; a bounded call's
never do, its slots are 16 B aligned and apart, and the caller's outputs are
written by a successful finish alone - not after a drain that timed out (the
context abandoned, the late copies landing in the bounce buffers), not after a
failed enqueue (still drained, MTCP_GPU_EIO); a slot may fill its buffer but
not pass it; each of two rounds copies out its own results once."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECTIONS = {"unbounded": 625, "bounded": 625, "pairs": 1250, "timed_out": 625, "enqueue_fails": 128,
            "capacity": 40, "two_rounds": 50, "pending_list": 25}


def test_host_call_rules(tmp_path):
    exe = tmp_path / "host_call_test"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-o", str(exe), os.path.join(ROOT, "tests", "c", "host_call_test.cpp")], check=True)
    r = json.loads(subprocess.run([str(exe)], capture_output=True, text=True, check=True,
                                  timeout=60).stdout.strip())
    assert set(r) == set(SECTIONS)
    for name, cases in SECTIONS.items():
        assert r[name] == {"cases": cases, "bad": 0, "first_line": 0}, name
