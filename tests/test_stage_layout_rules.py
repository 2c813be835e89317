"""The stage-buffer layouts of the host-memory calls (mtcp_amd/csrc/stage_layout.hpp)
on the CPU: tests/c/stage_layout_test.cpp lays out mtcp_gpu_steer, _group,
_rcvwalk, _ackwalk, _ackgen, _datagen, _rto_sweep, _tx_build and _tx_send over
a product of batch geometries, under AddressSanitizer and UBSan.  For every
call and shape: each region meets the alignment its _dev entry checks; the
regions are in order and disjoint, the back piece is contiguous and the
workspace follows it; a bounded HostCall with h_in and h_out blocks of exactly
the sizes the layout asks succeeds, the inputs arrive and the caller's outputs
receive exactly the bytes the contract names; and every offset and size equals
the value of the hand-chained arithmetic the layouts replaced
(tests/golden/stage_layout.txt), the pinned requests never above it."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECTIONS = {"steer": 48, "group": 12, "rcvwalk": 144, "ackwalk": 144, "ackgen": 312, "datagen": 312,
            "rto_sweep": 12, "tx_build": 72, "tx_send": 336}


def test_stage_layout_rules(tmp_path):
    exe = tmp_path / "stage_layout_test"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-o", str(exe), os.path.join(ROOT, "tests", "c", "stage_layout_test.cpp")], check=True)
    r = json.loads(subprocess.run([str(exe), os.path.join(ROOT, "tests", "golden", "stage_layout.txt")],
                                  capture_output=True, text=True, check=True, timeout=60).stdout.strip())
    assert set(r) == set(SECTIONS)
    for name, cases in SECTIONS.items():
        assert r[name] == {"cases": cases, "bad": 0, "first_line": 0}, name
