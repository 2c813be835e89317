// sndwrite_step.hpp — one write request of the batched application write
// (SURVEY §8 row f18): mtcp_write's body (mtcp/src/api.c:1458-1567),
// CopyFromUser (api.c:1416-1456) and SBPut's bookkeeping
// (mtcp/src/tcp_send_buffer.c:116-146) on the mirrors, with the verdict chain of
// include/mtcp_gpu_sndwrite.h on top.  One text, __host__ __device__: the plan
// kernel (sndwrite_kernels.hpp), tests/c/sndwrite_step_test.cpp (a plain g++
// build under the sanitizers) and tests/c/sndwrite_step_lib.cpp run it.  No HIP
// call is made here and no byte is copied: the step says what to move and what
// to copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mtcp_gpu_sndwrite.h"

namespace mg {

constexpr uint32_t kWriteUnit = 4096;                 // bytes of the destination's 16 B grid one wave moves
constexpr uint32_t kWriteUnitChunks = kWriteUnit / 16;

// What the step reads.  req: the request's 8 dwords; of d_snd[sid] snd_wnd
// (dword 2), sb_head_seq, sb_len, sb_size (16-18), mss2 = mss | eff_mss << 16
// (19), bits = tcp_state | saw_timestamp << 8 | wscale_peer << 16 | dup_acks <<
// 24 (20) and bits2 = nrtx | on_rto << 8 | has_sndbuf << 16 | rsvd << 24 (21);
// d_dtx[sid]: sb_off, sb_base_seq and dflags = on_send_list | on_control_list <<
// 8 | rsvd << 16 (all zero where sid > max_id: they are not looked at then);
// dup: the claim went to a lower request index.
struct WriteIn {
    uint32_t req[8];
    uint32_t snd_wnd, sb_head_seq, sb_len, sb_size, mss2, bits, bits2;
    uint64_t sb_off;
    uint32_t sb_base_seq, dflags, max_id;
    uint64_t src_bytes, payload_bytes;
    bool dup;
};

// What the step says.  res: the 4 dwords of the result record.  st_wnd:
// d_snd[sid].snd_wnd = snd_wnd is to be stored (FULL and WRITTEN); st_rec:
// d_snd[sid].sb_len = sb_len, d_dtx[sid].sb_base_seq = sb_base_seq and
// on_send_list = 1 as well (WRITTEN).  to_put != 0: to_put bytes go from byte src
// of the source region to byte dst of the arena.  move_len != 0: before that,
// move_len bytes of the arena move down from dst - sb_len(old) + head_off to dst -
// sb_len(old), that is from sb_off + head_off to sb_off (tcp_send_buffer.c:136).
struct WriteOut {
    uint32_t res[4], snd_wnd, sb_len, sb_base_seq, to_put, move_len, head_off;
    uint64_t src, dst;
    bool st_wnd, st_rec;
};

// mtcp_gpu_ackwalk.h's BAD rule on the dwords of a send state.
__host__ __device__ __forceinline__ bool write_snd_bad(const WriteIn &s) {
    const uint32_t eff_mss = s.mss2 >> 16, wscale_peer = (s.bits >> 16) & 0xFFu;
    return (s.bits2 >> 24) != 0 || eff_mss == 0 || wscale_peer > 31u || s.sb_size > MTCP_GPU_ACK_MAX_SIZE ||
           s.sb_len > s.sb_size;
}

// mtcp_gpu_datagen.h's BAD rule on the flag dword of a d_dtx record.
__host__ __device__ __forceinline__ bool write_dtx_bad(uint32_t dflags) {
    return (dflags >> 16) || (dflags & 0xFFu) > 1u || ((dflags >> 8) & 0xFFu) > 1u;
}

// The units of a copy of len bytes to destination byte dst: the 16 B pieces of
// the destination's grid that hold a byte of it, kWriteUnitChunks to a unit.
__host__ __device__ __forceinline__ uint32_t write_units(uint64_t dst, uint32_t len) {
    if (len == 0) return 0;
    const uint64_t nch = ((dst + len + 15) >> 4) - (dst >> 4);
    return (uint32_t)((nch + kWriteUnitChunks - 1) / kWriteUnitChunks);
}

__host__ __device__ __forceinline__ WriteOut write_step(const WriteIn &in) {
    WriteOut o{};
    const uint32_t sid = in.req[0], len = in.req[1];
    const uint64_t src_off = (uint64_t)in.req[3] << 32 | in.req[2];
    o.snd_wnd = in.snd_wnd, o.sb_len = in.sb_len, o.sb_base_seq = in.sb_base_seq;
    o.res[0] = sid;
    auto done = [&](uint32_t verdict, uint32_t flags, uint32_t written, uint32_t snd_wnd) {
        o.res[1] = written, o.res[2] = snd_wnd, o.res[3] = verdict | flags << 8;
        return o;
    };
    // 1. BAD_REQ
    if (sid > in.max_id || (in.req[4] | in.req[5] | in.req[6] | in.req[7]) != 0 || len > 0x7FFFFFFFu ||
        src_off > in.src_bytes || len > in.src_bytes - src_off)
        return done(MTCP_GPU_SNDWRITE_BAD_REQ, 0, 0, 0);
    // 2. DUP
    if (in.dup) return done(MTCP_GPU_SNDWRITE_DUP, 0, 0, 0);
    // 3. BAD_STATE
    const bool has_sndbuf = ((in.bits2 >> 16) & 0xFFu) != 0;
    // an empty buffer has head_off == 0: tcp_send_buffer.c:166-170
    const uint32_t head_off = in.sb_len == 0 ? 0u : in.sb_head_seq - in.sb_base_seq;
    if (write_snd_bad(in) || write_dtx_bad(in.dflags) ||
        (has_sndbuf && (in.sb_size == 0 || in.sb_off > in.payload_bytes || in.sb_size > in.payload_bytes - in.sb_off ||
                        head_off > in.sb_size - in.sb_len)))
        return done(MTCP_GPU_SNDWRITE_BAD_STATE, 0, 0, 0);
    const uint32_t room = in.snd_wnd > 0 ? MTCP_GPU_SNDWRITE_ROOM : 0u;           // api.c:1549
    // 4. DEFER_STATE: api.c:1495-1501
    if ((in.bits & 0xFFu) != MTCP_GPU_ACK_ST_ESTABLISHED) return done(MTCP_GPU_SNDWRITE_DEFER_STATE, room, 0, in.snd_wnd);
    // 5. ZERO: api.c:1503-1510
    if (len == 0) return done(MTCP_GPU_SNDWRITE_ZERO, room, 0, in.snd_wnd);
    // 6. EAGAIN: api.c:1423-1427, both operands as int (len <= 0x7FFFFFFF here)
    const int32_t wnd = (int32_t)in.snd_wnd;
    const int32_t sndlen = wnd < (int32_t)len ? wnd : (int32_t)len;
    if (sndlen <= 0) return done(MTCP_GPU_SNDWRITE_EAGAIN, room, 0, in.snd_wnd);
    // 7. NO_SNDBUF: api.c:1430-1438, SBInit stays with the host
    if (!has_sndbuf) return done(MTCP_GPU_SNDWRITE_NO_SNDBUF, room, 0, in.snd_wnd);
    // SBPut: tcp_send_buffer.c:124
    const uint32_t space = in.sb_size - in.sb_len;
    const uint32_t to_put = (uint32_t)sndlen < space ? (uint32_t)sndlen : space;
    // 8. FULL: :125-128, then api.c:1442 and :1443-1448
    if (to_put == 0) {
        o.st_wnd = true;
        o.snd_wnd = space;
        return done(MTCP_GPU_SNDWRITE_FULL, space > 0 ? MTCP_GPU_SNDWRITE_ROOM : 0u, 0, space);
    }
    // 9. WRITTEN
    uint32_t flags = 0;
    const uint32_t tail_off = head_off + in.sb_len;
    o.st_wnd = o.st_rec = true;
    o.to_put = to_put;
    o.src = src_off;
    if (tail_off + to_put < in.sb_size) {                                         // :130-133
        o.dst = in.sb_off + tail_off;
        if (in.sb_len == 0) o.sb_base_seq = in.sb_head_seq;                       // head_off was taken as 0
    } else {                                                                      // :134-141
        o.head_off = head_off;
        o.move_len = head_off ? in.sb_len : 0u;                                   // :136; onto itself with head_off == 0
        o.dst = in.sb_off + in.sb_len;                                            // :140
        o.sb_base_seq = in.sb_head_seq;                                           // :138-139
        flags |= MTCP_GPU_SNDWRITE_COMPACTED;
    }
    o.sb_len = in.sb_len + to_put;                                                // :142
    o.snd_wnd = in.sb_size - o.sb_len;                                            // api.c:1442
    if (!(in.dflags & 0xFFu)) flags |= MTCP_GPU_SNDWRITE_SEND_LIST_ADD;           // api.c:1535-1541, core.c:479-483
    if (o.snd_wnd > 0) flags |= MTCP_GPU_SNDWRITE_ROOM;
    return done(MTCP_GPU_SNDWRITE_WRITTEN, flags, to_put, o.snd_wnd);
}

}  // namespace mg
