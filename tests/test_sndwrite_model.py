"""tests/sndwrite_model.py against the reference: tests/golden/sndwrite_cases.bin
holds every SBPut and SBRemove the generator ran on the reference's own send
buffer (tests/c/ref_sndwrite_gen.c): the return value, head_off, tail_off, len,
cum_len, head_seq and the whole chunk after every operation.  The line-by-line
model must give every word and byte; the batch contract on anchored records
must give the same and equal a plain loop on random request lists with
duplicates; its table must flush the written bytes through the data
generation's model; the step text the plan kernel runs, compiled for the host,
must equal the model on both."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from mtcp_amd import _lib
from mtcp_amd._types import (FLOW_NONE, SNDWRITE_COMPACTED, SNDWRITE_HOST_MAX_BYTES, SNDWRITE_REQ_DTYPE,
                             SNDWRITE_RES_DTYPE, SNDWRITE_ROOM, SNDWRITE_SEND_LIST_ADD, SNDWRITE_VERDICTS)
from tests import sndwrite_cases as sc
from tests import sndwrite_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fixture():
    return sm.load_fixture()


def replay(cases):
    """Every operation of every case on a SendBuf: yields (case index, op, the
    put's bytes or None, the buffer before the operation ran) and runs the model."""
    for ci, c in enumerate(cases):
        buf = sm.SendBuf(c["size"], c["init_seq"])
        serial = 0
        for op in c["ops"]:
            data = None
            if op["kind"] == "put":
                data = sm.payload_bytes(ci, serial, op["len"])
                serial += 1
            yield ci, op, data, buf
            ret = sm.SBPut(buf, data, op["len"])[0] if op["kind"] == "put" else sm.SBRemove(buf, op["len"])
            assert ret == op["ret"], (ci, op["kind"], op["len"])
            assert buf.snapshot() == op["after"], (ci, op["kind"], op["len"], buf.snapshot(), op["after"])
            assert (buf.data == op["data"]).all(), (ci, op["kind"], op["len"])


def test_the_model_gives_every_word_and_byte_of_the_fixture(fixture):
    kinds = {"put": 0, "rem": 0}
    for _, op, _, _ in replay(fixture):
        kinds[op["kind"]] += 1
    assert kinds["put"] > 200 and kinds["rem"] > 100, kinds


def test_the_fixture_covers_what_the_issue_lists(fixture):
    seen = set()
    for _, op, _, buf in replay(fixture):
        size, ret = buf.size, op["ret"]
        if op["kind"] == "rem":
            if ret > 0 and op["after"][2] == 0:
                seen.add("emptied")
                assert op["after"][:2] == (0, 0)
            continue
        if ret == -2:
            seen.add("full")
            continue
        if op["len"] == 1:
            seen.add("len1")
        if ret < op["len"]:
            seen.add("clamped")
        if buf.len == 0 and buf.head_seq != 0 and op["after"][2] == ret and "emptied" in seen:
            seen.add("put after reset")
        if buf.head_seq > (buf.head_seq + buf.len + ret) & sm.M32 or buf.head_seq + buf.len + ret > sm.M32:
            seen.add("wrap")
        if buf.tail_off + ret < size:
            seen.add("below")
            continue
        seen.add(("exact", buf.head_off > 0) if buf.tail_off + ret == size else "beyond")
        if buf.head_off in (1, 15, 16, 17, size - 1):
            seen.add(("head", buf.head_off if buf.head_off < 18 else "size-1"))
        if buf.head_off:
            for m in (1, 15, 16, 17, 1023, 1024, 1025, 2047, 2048, 2049):
                if buf.len == m:
                    seen.add(("moved", m))
            if buf.len < buf.head_off + buf.len and buf.len + ret > buf.head_off:
                seen.add("overlap")           # the destination [len, len + ret) reaches into the old window
    want = {"emptied", "full", "len1", "clamped", "put after reset", "wrap", "below", ("exact", False), ("exact", True),
            "beyond", "overlap"}
    want |= {("head", h) for h in (1, 15, 16, 17, "size-1")}
    want |= {("moved", m) for m in (1, 15, 16, 17, 1023, 1024, 1025, 2047, 2048, 2049)}
    assert want <= seen, want - seen


def check_case(ci, c, run):
    """One case of the fixture on anchored records: puts as batches of one
    request through run(batch), removes as the record updates the ACK walk
    makes.  Every word and every byte of the arena after every operation."""
    buf0 = sm.SendBuf(c["size"], c["init_seq"])
    b = sc.lay_out([buf0], chunk_align=[ci], stale_base=[c["init_seq"] ^ 0x1234])
    off = b.chunks[0][0]
    serial, cum, done = 0, 0, 0
    for op in c["ops"]:
        head_off, tail_off, blen, cum_len, head_seq = op["after"]
        if op["kind"] == "put":
            data = sm.payload_bytes(ci, serial, op["len"])
            serial += 1
            b.snd["snd_wnd"][0] = c["size"]           # an open window: SBPut's own clamp decides
            on_before = int(b.dtx["on_send_list"][0])
            tail_before = sm.offsets_of(b.snd[0], b.dtx[0])[1]
            b.requests([0], [op["len"]], src_align=[ci + serial], fill=lambda i, n: data)
            snd, dtx, payload, wres, seg_sid, seg_start, seg_stop, nseg, total = run(b)
            r = wres[0]
            if op["ret"] > 0:
                cum += op["ret"]
                assert (r["verdict"], r["written"]) == (sm.WRITTEN, op["ret"]) and total.tolist() == [1, op["ret"]]
                want = ((SNDWRITE_ROOM if blen < c["size"] else 0) | (0 if on_before else SNDWRITE_SEND_LIST_ADD) |
                        (SNDWRITE_COMPACTED if tail_before + op["ret"] >= c["size"] else 0))
                assert int(r["flags"]) == want and seg_sid.tolist() == [0] and dtx["on_send_list"][0] == 1
            else:
                assert op["ret"] == -2 and (r["verdict"], r["written"], r["flags"]) == (sm.FULL, 0, 0)
                assert total.tolist() == [0, 0] and seg_sid.tolist() == [FLOW_NONE]
            assert int(r["snd_wnd"]) == int(snd["snd_wnd"][0]) == c["size"] - blen
            assert seg_start.tolist() == [0, 0] and seg_stop.tolist() == [0] and nseg.tolist() == [1]
            b.snd, b.dtx, b.payload = snd, dtx, payload
            done += 1
        elif op["ret"] > 0:                           # tcp_in.c's SBRemove as mtcp_gpu_ackwalk.h mirrors it
            b.snd["sb_head_seq"][0] = (int(b.snd["sb_head_seq"][0]) + op["ret"]) & sm.M32
            b.snd["sb_len"][0] -= op["ret"]
        got_head, got_tail = sm.offsets_of(b.snd[0], b.dtx[0])
        assert (got_head, int(b.snd["sb_len"][0]), int(b.snd["sb_head_seq"][0])) == (head_off, blen, head_seq)
        assert blen == 0 or got_tail == tail_off
        assert cum == cum_len
        assert (b.payload[off:off + c["size"]] == op["data"]).all(), (ci, op["kind"], op["len"])
        guard = np.ones(len(b.payload), dtype=bool)
        guard[off:off + c["size"]] = False
        assert (b.payload[guard] == sc.ARENA_FILL).all()
    return done


def test_the_anchored_records_give_every_operation_of_the_fixture(fixture):
    done = sum(check_case(ci, c, lambda b: b.expect()) for ci, c in enumerate(fixture))
    assert done > 200


def test_the_batch_equals_a_plain_loop_with_duplicates():
    rng = np.random.default_rng(18)
    verdicts = set()
    for trial in range(80):
        b = sc.random_batch(rng, 1 + int(rng.integers(12)), 1 + int(rng.integers(40)), dup=0.3)
        snd, dtx, payload, wres, seg_sid, seg_start, seg_stop, nseg, total = b.expect()
        s2, d2, p2 = b.copies()
        wres2, sid2, total2 = sm.write_loop(b.wreq, b.max_id, s2, d2, b.src, p2)
        assert wres.tobytes() == wres2.tobytes() and total.tolist() == total2.tolist(), trial
        assert snd.tobytes() == s2.tobytes() and dtx.tobytes() == d2.tobytes() and (payload == p2).all(), trial
        assert seg_sid.tolist() == sid2.tolist() and not seg_start.any() and not seg_stop.any() and nseg[0] == len(wres)
        verdicts |= set(wres["verdict"].tolist())
        for i in range(len(b.wreq)):
            earlier = int(b.wreq["sid"][i]) in b.wreq["sid"][:i].tolist()
            assert (wres["verdict"][i] == sm.DUP) <= earlier
        # no stream twice in the table, and exactly the written ones
        listed = [s for s in seg_sid.tolist() if s != FLOW_NONE]
        assert len(listed) == len(set(listed)) == int(total[0])
        assert [s != FLOW_NONE for s in seg_sid.tolist()] == (wres["verdict"] == sm.WRITTEN).tolist()
        # guards: no byte outside the streams' chunks changed
        mask = np.ones(len(payload), dtype=bool)
        for off, size in b.chunks:
            mask[off:off + size] = False
        assert (payload[mask] == sc.ARENA_FILL).all()
    assert verdicts == set(range(1, 10)), verdicts


def test_random_record_bytes_equal_a_plain_loop():
    rng = np.random.default_rng(19)
    verdicts = set()
    for trial in range(300):
        b = sc.random_records(rng, 12, 20)
        snd, dtx, payload, wres, seg_sid, *_, total = b.expect()
        s2, d2, p2 = b.copies()
        wres2, sid2, total2 = sm.write_loop(b.wreq, b.max_id, s2, d2, b.src, p2)
        assert wres.tobytes() == wres2.tobytes() and total.tolist() == total2.tolist(), trial
        assert snd.tobytes() == s2.tobytes() and dtx.tobytes() == d2.tobytes() and (payload == p2).all(), trial
        verdicts |= set(wres["verdict"].tolist())
    assert verdicts == set(range(1, 10)), verdicts


def test_the_table_flushes_the_written_bytes_from_snd_nxt():
    """The table and the records the write leaves, through tests/datagen_model.py
    as row f15 reads them: every WRITTEN stream sends, in request order, the
    bytes of its buffer from snd_nxt, the written ones last."""
    from tests import datagen_model as dm
    from tests import rtosweep_model as rs
    rng = np.random.default_rng(20)
    bufs = [sc.buffer(rng, 4096, 0), sc.buffer(rng, 4096, 500, head_off=0), sc.buffer(rng, 4096, 700, head_off=3000),
            sc.buffer(rng, 2048, 100, head_off=1900), sc.buffer(rng, 4096, 4096)]
    b = sc.lay_out(bufs, rng=rng, stale_base=[99, None, None, None, None])
    b.snd["cwnd"], b.snd["peer_wnd"], b.snd["rto"] = 1 << 20, 1 << 20, 200
    b.requests([2, 0, 4, 3, 1, 2], [900, 1000, 10, 300, 1448, 5], rng=rng)
    snd, dtx, payload, wres, seg_sid, seg_start, seg_stop, nseg, total = b.expect()
    assert wres["verdict"].tolist() == [sm.WRITTEN, sm.WRITTEN, sm.EAGAIN, sm.WRITTEN, sm.WRITTEN, sm.DUP]
    assert wres["flags"][0] & SNDWRITE_COMPACTED and wres["flags"][3] & SNDWRITE_COMPACTED
    n = len(wres)
    state, tx, _ = rs.send_side(len(bufs), 5)
    seg_cap = 16
    seg, desc, dres, dtotal, snd2, tx2, dtx2, bursts = dm.datagen(
        None, None, n, b.max_id, np.zeros(n, np.uint32), seg_sid, seg_start, int(nseg[0]), seg_stop, state, snd, tx, dtx,
        1000, len(payload), rs.N_LINKS, 0, seg_cap * rs.SLOT, 0, rs.SLOT, seg_cap)
    for i in range(n):
        if wres["verdict"][i] != sm.WRITTEN:
            assert dres["status"][i] == dm.NONE and dres["n_seg"][i] == 0
            continue
        sid = int(wres["sid"][i])
        assert dres["status"][i] == dm.SENT and not dtx2["on_send_list"][sid]
        before, put = int(b.snd["sb_len"][sid]), int(wres["written"][i])
        assert int(dres["bytes"][i]) == before + put       # snd_nxt was the buffer's head
        got = b""
        for k in range(int(dres["first_seg"][i]), int(dres["first_seg"][i]) + int(dres["n_seg"][i])):
            o, ln = int(seg["payload_off"][k]), int(seg["payload_len"][k])
            got += payload[o:o + ln].tobytes()
        start, _ = b.ranges[i]
        old = b.payload[b.chunks[sid][0] + bufs[sid].head_off:][:before].tobytes()
        assert got == old + b.src[start:start + put].tobytes()
        assert int(snd2["snd_nxt"][sid]) == (int(b.snd["snd_nxt"][sid]) + before + put) & sm.M32


# ---- the step text on the host ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def step_lib(tmp_path_factory):
    so = tmp_path_factory.mktemp("sndwrite_step") / "libsndwrite_step.so"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__",
                    "-I/opt/rocm/include", "-o", str(so), os.path.join(ROOT, "tests", "c", "sndwrite_step_lib.cpp")],
                   check=True)
    L = ctypes.CDLL(str(so))
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    L.sndwrite_step_batch.argtypes = [vp, u32, u32, vp, vp, vp, u64, vp, u64, vp, vp, vp, vp, vp, vp]
    L.sndwrite_step_batch.restype = u64
    return L


def run_step(L, b):
    snd, dtx, payload = b.copies()
    n = len(b.wreq)
    wres, total = np.zeros(max(n, 1), dtype=SNDWRITE_RES_DTYPE), np.zeros(2, dtype=np.uint64)
    seg_sid, seg_start = np.full(max(n, 1), 7, dtype=np.uint32), np.full(n + 1, 7, dtype=np.uint32)
    seg_stop, nseg = np.full(max(n, 1), 7, dtype=np.uint32), np.full(1, 7, dtype=np.uint32)
    src = np.ascontiguousarray(b.src)
    units = L.sndwrite_step_batch(b.wreq.ctypes.data, n, b.max_id, snd.ctypes.data, dtx.ctypes.data, src.ctypes.data,
                                  len(src), payload.ctypes.data, len(payload), wres.ctypes.data, seg_sid.ctypes.data,
                                  seg_start.ctypes.data, seg_stop.ctypes.data, nseg.ctypes.data, total.ctypes.data)
    assert units < 1 << 40
    return snd, dtx, payload, wres[:n], seg_sid[:n], seg_start, seg_stop[:n], nseg, total


def same(got, want):
    for g, w in zip(got, want):
        assert g.tobytes() == w.tobytes()


def test_the_step_text_equals_the_model_on_the_fixture(fixture, step_lib):
    done = sum(check_case(ci, c, lambda b: run_step(step_lib, b)) for ci, c in enumerate(fixture))
    assert done > 200


def test_the_step_text_equals_the_model_on_random_batches_and_random_record_bytes(step_lib):
    rng = np.random.default_rng(24)
    for trial in range(40):
        b = sc.random_batch(rng, 1 + int(rng.integers(12)), 1 + int(rng.integers(40)), dup=0.3)
        same(run_step(step_lib, b), b.expect())
    verdicts = set()
    for trial in range(300):
        b = sc.random_records(rng, 16, 24)
        got = run_step(step_lib, b)
        same(got, b.expect())
        verdicts |= set(got[3]["verdict"].tolist())
    assert verdicts == set(range(1, 10)), verdicts


def test_struct_sizes_offsets_and_exports(tmp_path):
    src = open(os.path.join(ROOT, "include", "mtcp_gpu_sndwrite.h")).read()
    assert "#define MTCP_GPU_HAS_SNDWRITE" in src
    decl = set(re.findall(r"\b(mtcp_gpu_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))
    assert decl == {"mtcp_gpu_sndwrite_work_bytes", "mtcp_gpu_sndwrite_tile", "mtcp_gpu_sndwrite_dev",
                    "mtcp_gpu_sndwrite", "mtcp_gpu_write_send_dev"} and decl <= set(_lib.EXPORTS)
    L = _lib.lib()
    assert all(hasattr(L, f) for f in decl) and L.mtcp_gpu_abi_version() == 5
    # the header as a C compiler lays it out
    prog = tmp_path / "layout.c"
    fields = {"mtcp_gpu_sndwrite_req": SNDWRITE_REQ_DTYPE, "mtcp_gpu_sndwrite_res": SNDWRITE_RES_DTYPE}
    lines = [f'printf("%zu\\n", sizeof({t}));' for t in fields]
    lines += [f'printf("%zu\\n", offsetof({t}, {f}));' for t, dt in fields.items() for f in dt.names]
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mtcp_gpu_sndwrite.h"\nint main(void) {\n' +
                    "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(prog)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [dt.itemsize for dt in fields.values()] + [dt.fields[f][1] for dt in fields.values() for f in dt.names]
    assert got == want
    consts = dict(re.findall(r"#define (MTCP_GPU_SNDWRITE_\w+)\s+(0x[0-9a-fA-F]+)u", src))
    assert {k: int(v, 16) for k, v in consts.items()} == {
        "MTCP_GPU_SNDWRITE_ROOM": SNDWRITE_ROOM, "MTCP_GPU_SNDWRITE_SEND_LIST_ADD": SNDWRITE_SEND_LIST_ADD,
        "MTCP_GPU_SNDWRITE_COMPACTED": SNDWRITE_COMPACTED}
    assert re.search(r"#define MTCP_GPU_SNDWRITE_HOST_MAX_BYTES \(32u << 20\)", src) and SNDWRITE_HOST_MAX_BYTES == 32 << 20
    enum = re.findall(r"MTCP_GPU_SNDWRITE_(\w+)\s*= (\d),", src) + re.findall(r"MTCP_GPU_SNDWRITE_(WRITTEN)\s*= (\d)", src)
    assert [name for name, _ in sorted(set(enum), key=lambda e: int(e[1]))] == list(SNDWRITE_VERDICTS)


def test_work_bytes_are_monotone_and_the_tile_is_the_models():
    L = _lib.lib()
    wb = L.mtcp_gpu_sndwrite_work_bytes
    assert L.mtcp_gpu_sndwrite_tile() == sm.UNIT
    assert wb((1 << 26) + 1, 0) == 0 and wb(1, 0xFFFFFFF0) == 0
    prev = 0
    for max_id in (0, 1, 4095, 4096, 65535, (1 << 20) - 1, 1 << 24, 0xFFFFFFEF):
        got = [wb(n, max_id) for n in (0, 1, 255, 256, 257, 65536, 1 << 20, 1 << 26)]
        assert got[0] > 0 and got == sorted(got) and got[0] >= prev
        prev = got[0]
