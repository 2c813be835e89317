"""tests/rcvread_model.py against the reference: tests/golden/rcvread_cases.bin
holds, for 66 streams, every RBPut and every CopyToUser / PeekForUser the
generator ran on the reference's own ring buffer (tests/c/ref_rcvread_gen.c): the
returned length and bytes, the three offsets, head_seq, merged_len, the fragment
list, rcv_wnd and whether a fragment was freed.  The line-by-line model must give
every word and byte; the batch contract on record arrays must give the same for
every read of the fixture and equal a plain loop on random request lists with
duplicates; the step text the plan kernel runs, compiled for the host, must
equal the model on both."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from mtcp_amd import _lib
from mtcp_amd._types import (RCVREAD_FRAG_FREED, RCVREAD_MORE, RCVREAD_ON_ACKQ, RCVREAD_PEEK, RCVREAD_REQ_DTYPE,
                             RCVREAD_RES_DTYPE, RCVREAD_WND_ADV)
from tests import rcvread_cases as rc
from tests import rcvread_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fixture():
    return rm.load_fixture()


def replay(cases):
    """Every event of every case on an App: yields (case index, event, app before the event ran)."""
    for ci, c in enumerate(cases):
        app = rm.App(c["size"], c["init_seq"], c["eff_mss"])
        serial = 0
        for ev in c["events"]:
            yield ci, ev, app
            if ev["kind"] == "put":
                ret = app.put(ev["seq"], rm.payload_bytes(ci, serial, ev["len"]))
                serial += 1
                assert ret == ev["ret"], (ci, ev)
            else:
                app.need_wnd_adv, app.on_ackq = ev["need_wnd_adv"], ev["on_ackq"]
                if ev["kind"] == "peek":
                    ret, got = rm.PeekForUser(app, ev["len"])
                    freed = False
                else:
                    ret, got, freed = rm.CopyToUser(app, ev["len"])
                assert (ret, got, int(freed)) == (ev["ret"], ev["bytes"], ev["freed"]), (ci, ev)
                assert (app.need_wnd_adv, app.on_ackq) == (ev["need_wnd_adv_after"], ev["on_ackq_after"]), (ci, ev)
            assert app.snapshot() == ev["after"], (ci, ev, app.snapshot())


def test_the_model_gives_every_word_and_byte_of_the_fixture(fixture):
    kinds = {"put": 0, "read": 0, "peek": 0}
    for _, ev, _ in replay(fixture):
        kinds[ev["kind"]] += 1
    assert kinds["put"] > 300 and kinds["read"] > 300 and kinds["peek"] > 60, kinds


def test_the_fixture_covers_what_the_issue_lists(fixture):
    seen = set()
    for c in fixture:
        for ev in c["events"]:
            head, _, _, head_seq, merged, rcv_wnd, frags = ev["after"]
            if ev["kind"] == "put":
                continue
            before = merged + max(ev["ret"], 0) if ev["kind"] == "read" else merged
            seen.add("eagain" if ev["ret"] < 0 else "below" if ev["len"] < before else
                     "equal" if ev["len"] == before else "above")
            if ev["len"] == 1 and ev["ret"] == 1:
                seen.add("len1")
            if ev["kind"] == "read" and ev["ret"] > 0:
                seen.add(("freed", ev["freed"], min(len(frags) + ev["freed"], 4)))
                if head in (1, 15, 16, 17, c["size"] - 1):
                    seen.add(("head", head if head < 18 else "size-1"))
                if head_seq < ev["ret"]:
                    seen.add("wrap")
                if c["family"] == 5:
                    seen.add(("wnd", rcv_wnd - c["eff_mss"], ev["need_wnd_adv"], ev["on_ackq"],
                              ev["need_wnd_adv"] and not ev["need_wnd_adv_after"]))
    want = {"eagain", "below", "equal", "above", "len1", "wrap"}
    want |= {("freed", f, k) for f in (0, 1) for k in (2, 3, 4)} | {("head", h) for h in (1, 15, 16, 17, "size-1")}
    want |= {("wnd", d, nwa, ackq, int(bool(d > 0 and nwa and not ackq))) for d in (-1, 0, 1) for nwa in (0, 1)
             for ackq in (0, 1)}
    assert want <= seen, want - seen


def check_read_event(ev, app_before, run):
    """One read or peek of the fixture as a batch of one request on the records of app_before."""
    if len(app_before.st.frags) > 4:
        return False
    app_before.need_wnd_adv = ev["need_wnd_adv"]
    b = rc.lay_out([app_before], src_align=[5])
    flags = (RCVREAD_PEEK if ev["kind"] == "peek" else 0) | (RCVREAD_ON_ACKQ if ev["on_ackq"] else 0)
    b.requests([0], [ev["len"]], [flags], dst_align=[3])
    state, rbuf, tx, dst, rres, total = run(b)
    r, at = rres[0], int(b.req["dst_off"][0])
    head, tail, last, head_seq, merged, rcv_wnd, frags = ev["after"]
    want_dst = b.dst.copy()
    if ev["ret"] < 0:
        assert (r["verdict"], r["copylen"]) == (rm.EAGAIN, 0) and total.tolist() == [0, 0]
    else:
        assert (r["verdict"], r["copylen"]) == (rm.PEEKED if ev["kind"] == "peek" else rm.READ, ev["ret"])
        want_dst[at:at + ev["ret"]] = np.frombuffer(ev["bytes"], dtype=np.uint8)
        assert total.tolist() == [1, ev["ret"]]
    assert (dst == want_dst).all()
    assert (int(rbuf["head_offset"][0]), int(rbuf["tail_offset"][0]), int(rbuf["last_len"][0])) == (head, tail, last)
    s = state[0]
    assert (int(s["head_seq"]), int(s["merged_len"]), int(s["nfrag"])) == (head_seq, merged, len(frags))
    assert [(int(s["frag"]["seq"][k]), int(s["frag"]["len"][k])) for k in range(len(frags))] == frags
    assert not s["frag"]["len"][len(frags):].any() and not s["frag"]["seq"][len(frags):].any()
    assert int(s["rcv_wnd"]) == rcv_wnd == int(r["rcv_wnd"])
    assert int(tx["need_wnd_adv"][0]) == ev["need_wnd_adv_after"]
    fired = ev["on_ackq_after"] and not ev["on_ackq"]
    want_flags = ((RCVREAD_MORE if merged else 0) | (RCVREAD_WND_ADV if fired else 0) |
                  (RCVREAD_FRAG_FREED if ev["freed"] else 0))
    assert int(r["flags"]) == want_flags, (ev, r)
    return True


def test_the_batch_contract_gives_every_read_of_the_fixture(fixture):
    done = sum(check_read_event(ev, app, lambda b: b.expect()) for _, ev, app in replay(fixture) if ev["kind"] != "put")
    assert done > 400


def test_the_batch_equals_a_plain_loop_with_duplicates():
    rng = np.random.default_rng(17)
    verdicts = set()
    for trial in range(60):
        b = rc.random_batch(rng, 1 + int(rng.integers(12)), 1 + int(rng.integers(40)), dup=0.3, with_tx=trial % 5 != 0)
        state, rbuf, tx, dst, rres, total = b.expect()
        s2, r2, t2, snd, arena, d2 = b.copies()
        rres2, total2 = rm.read_loop(b.req, b.max_id, s2, r2, t2, snd, arena, d2)
        assert rres.tobytes() == rres2.tobytes() and total.tolist() == total2.tolist(), trial
        assert state.tobytes() == s2.tobytes() and rbuf.tobytes() == r2.tobytes() and (dst == d2).all(), trial
        assert (tx is None and t2 is None) or tx.tobytes() == t2.tobytes()
        verdicts |= set(rres["verdict"].tolist())
        # a DUP is never the first request of its sid, every first request is something else
        for i in range(len(b.req)):
            earlier = int(b.req["sid"][i]) in b.req["sid"][:i].tolist()
            assert (rres["verdict"][i] == rm.DUP) <= earlier
        # guards: no byte outside the accepted ranges changed
        mask = np.ones(len(dst), dtype=bool)
        for q, r in zip(b.req, rres):
            mask[int(q["dst_off"]):int(q["dst_off"]) + int(r["copylen"])] = False
        assert (dst[mask] == 0x5A).all()
    assert verdicts == set(range(1, 8)), verdicts


# ---- the step text on the host ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def step_lib(tmp_path_factory):
    so = tmp_path_factory.mktemp("rcvread_step") / "librcvread_step.so"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__",
                    "-I/opt/rocm/include", "-o", str(so), os.path.join(ROOT, "tests", "c", "rcvread_step_lib.cpp")],
                   check=True)
    L = ctypes.CDLL(str(so))
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    L.rcvread_step_batch.argtypes = [vp, u32, u32, vp, vp, vp, vp, vp, u64, vp, u64, vp, vp]
    L.rcvread_step_batch.restype = u64
    return L


def run_step(L, b):
    state, rbuf, tx, snd, arena, dst = b.copies()
    rres, total = np.zeros(max(len(b.req), 1), dtype=RCVREAD_RES_DTYPE), np.zeros(2, dtype=np.uint64)
    units = L.rcvread_step_batch(b.req.ctypes.data, len(b.req), b.max_id, state.ctypes.data, rbuf.ctypes.data,
                                 None if tx is None else tx.ctypes.data, None if snd is None else snd.ctypes.data,
                                 arena.ctypes.data, len(arena), dst.ctypes.data, len(dst), rres.ctypes.data,
                                 total.ctypes.data)
    rres = rres[:len(b.req)]
    assert units == sum(rm.units(int(q["dst_off"]), int(r["copylen"])) for q, r in zip(b.req, rres))
    return state, rbuf, tx, dst, rres, total


def same(got, want):
    for g, w in zip(got, want):
        assert (g is None and w is None) or g.tobytes() == w.tobytes()


def test_the_step_text_equals_the_model_on_the_fixture(fixture, step_lib):
    done = sum(check_read_event(ev, app, lambda b: run_step(step_lib, b)) for _, ev, app in replay(fixture)
               if ev["kind"] != "put")
    assert done > 400


def test_the_step_text_equals_the_model_on_random_batches_and_random_record_bytes(step_lib):
    rng = np.random.default_rng(23)
    for trial in range(40):
        b = rc.random_batch(rng, 1 + int(rng.integers(12)), 1 + int(rng.integers(40)), dup=0.3, with_tx=trial % 5 != 0)
        same(run_step(step_lib, b), b.expect())
    verdicts = set()
    for trial in range(300):
        b = rc.random_records(rng, 16, 24)
        got = run_step(step_lib, b)
        same(got, b.expect())
        verdicts |= set(got[4]["verdict"].tolist())
    assert {rm.BAD_REQ, rm.DUP, rm.BAD_STATE, rm.EAGAIN, rm.READ} <= verdicts, verdicts


def test_struct_sizes_offsets_and_exports(tmp_path):
    src = open(os.path.join(ROOT, "include", "mtcp_gpu_rcvread.h")).read()
    assert "#define MTCP_GPU_HAS_RCVREAD" in src
    decl = set(re.findall(r"\b(mtcp_gpu_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))
    assert decl == {"mtcp_gpu_rcvread_work_bytes", "mtcp_gpu_rcvread_tile", "mtcp_gpu_rcvread_dev",
                    "mtcp_gpu_rcvread"} and decl <= set(_lib.EXPORTS)
    L = _lib.lib()
    assert all(hasattr(L, f) for f in decl) and L.mtcp_gpu_abi_version() == 5
    # the header as a C compiler lays it out
    prog = tmp_path / "layout.c"
    fields = {"mtcp_gpu_rcvread_req": RCVREAD_REQ_DTYPE, "mtcp_gpu_rcvread_res": RCVREAD_RES_DTYPE}
    lines = [f'printf("%zu\\n", sizeof({t}));' for t in fields]
    lines += [f'printf("%zu\\n", offsetof({t}, {f}));' for t, dt in fields.items() for f in dt.names]
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mtcp_gpu_rcvread.h"\nint main(void) {\n' +
                    "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(prog)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [dt.itemsize for dt in fields.values()] + [dt.fields[f][1] for dt in fields.values() for f in dt.names]
    assert got == want
    consts = dict(re.findall(r"#define (MTCP_GPU_RCVREAD_\w+)\s+(0x[0-9a-fA-F]+)u", src))
    assert {k: int(v, 16) for k, v in consts.items()} == {
        "MTCP_GPU_RCVREAD_PEEK": RCVREAD_PEEK, "MTCP_GPU_RCVREAD_ON_ACKQ": RCVREAD_ON_ACKQ,
        "MTCP_GPU_RCVREAD_MORE": RCVREAD_MORE, "MTCP_GPU_RCVREAD_WND_ADV": RCVREAD_WND_ADV,
        "MTCP_GPU_RCVREAD_FRAG_FREED": RCVREAD_FRAG_FREED}
    enum = re.findall(r"MTCP_GPU_RCVREAD_(\w+)\s*= (\d),", src) + re.findall(r"MTCP_GPU_RCVREAD_(READ)\s*= (\d)", src)
    from mtcp_amd._types import RCVREAD_VERDICTS
    assert [name for name, _ in sorted(set(enum), key=lambda e: int(e[1]))] == list(RCVREAD_VERDICTS)


def test_work_bytes_are_monotone_and_the_tile_is_the_models():
    L = _lib.lib()
    wb = L.mtcp_gpu_rcvread_work_bytes
    assert L.mtcp_gpu_rcvread_tile() == rm.UNIT
    assert wb((1 << 26) + 1, 0) == 0 and wb(1, 0xFFFFFFF0) == 0
    prev = 0
    for max_id in (0, 1, 4095, 4096, 65535, (1 << 20) - 1, 1 << 24, 0xFFFFFFEF):
        got = [wb(n, max_id) for n in (0, 1, 255, 256, 257, 65536, 1 << 20, 1 << 26)]
        assert got[0] > 0 and got == sorted(got) and got[0] >= prev
        prev = got[0]
