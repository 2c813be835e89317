// rcvread_step.hpp — one read request of the batched application read
// (SURVEY §8 row f17): CopyToUser / PeekForUser (mtcp/src/api.c:1096-1149) and
// RBRemove (mtcp/src/tcp_ring_buffer.c:384-421) on the mirrors, with the verdict
// chain of include/mtcp_gpu_rcvread.h on top.  One text, __host__ __device__:
// the plan kernel (rcvread_kernels.hpp), tests/c/rcvread_step_test.cpp (a plain
// g++ build under the sanitizers) and tests/c/rcvread_step_lib.cpp run it.  No
// HIP call is made here and no byte is copied: the step says what to copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mtcp_gpu_rcvread.h"

namespace mg {

constexpr uint32_t kReadUnit = 4096;                  // bytes of the destination's 16 B grid one wave moves
constexpr uint32_t kReadUnitChunks = kReadUnit / 16;

// What the step reads.  req: the request's 8 dwords; st: the 16 dwords of
// d_state[sid]; rb: the 8 dwords of d_rbuf[sid] (both zero where sid > max_id:
// they are not looked at then); need_wnd_adv: d_tx[sid] byte 19 and eff_mss:
// d_snd[sid] bytes 78-79, read where has_tx; dup: the claim went to a lower
// request index.
struct ReadIn {
    uint32_t req[8], st[16], rb[8];
    uint32_t need_wnd_adv, eff_mss, max_id;
    uint64_t arena_bytes, dst_bytes;
    bool has_tx, dup;
};

// What the step says.  res: the 4 dwords of the result record.  st_rec: st[]
// (the whole new state record) and rb_head / rb_last (dwords 3 and 5 of the
// buffer record) are to be stored; st_tx: d_tx[sid] byte 19 = 0.  copylen != 0:
// copylen bytes go from byte src of the arena to the request's destination.
struct ReadOut {
    uint32_t res[4], st[16], rb_head, rb_last, copylen;
    uint64_t src;
    bool st_rec, st_tx;
};

// mtcp_gpu_rcvwalk.h's BAD rule on the 16 dwords of a state record.
__host__ __device__ __forceinline__ bool read_state_bad(const uint32_t (&st)[16]) {
    const uint32_t nfrag = (st[7] >> 16) & 0xFFu;
    bool bad = (st[7] >> 24) != 0 || nfrag > MTCP_GPU_RCV_MAX_FRAGS || st[4] > MTCP_GPU_RCV_MAX_SIZE || st[3] > st[4];
    for (uint32_t k = 0; k < MTCP_GPU_RCV_MAX_FRAGS; ++k) bad |= k < nfrag && (st[9 + 2 * k] >> 31) != 0;
    return bad;
}

// mtcp_gpu_rcvcopy.h's BAD rule on the 8 dwords of a buffer record.
__host__ __device__ __forceinline__ bool read_buf_bad(const uint32_t (&rb)[8], uint64_t arena_bytes) {
    const uint64_t data_off = (uint64_t)rb[1] << 32 | rb[0];
    const uint32_t size = rb[2], head = rb[3], tail = rb[4], last = rb[5];
    return (rb[6] | rb[7]) != 0 || size == 0 || size > MTCP_GPU_RCV_MAX_SIZE || data_off > arena_bytes ||
           size > arena_bytes - data_off || head > tail || tail > size || last != tail - head;
}

// The units of a copy of len bytes to destination byte dst: the 16 B pieces of
// the destination's grid that hold a byte of it, kReadUnitChunks to a unit.
__host__ __device__ __forceinline__ uint32_t read_units(uint64_t dst, uint32_t len) {
    if (len == 0) return 0;
    const uint64_t nch = ((dst + len + 15) >> 4) - (dst >> 4);
    return (uint32_t)((nch + kReadUnitChunks - 1) / kReadUnitChunks);
}

__host__ __device__ __forceinline__ ReadOut read_step(const ReadIn &in) {
    ReadOut o{};
    const uint32_t sid = in.req[0], len = in.req[1], rflags = in.req[4];
    const uint64_t dst_off = (uint64_t)in.req[3] << 32 | in.req[2];
    for (int i = 0; i < 16; ++i) o.st[i] = in.st[i];
    o.rb_head = in.rb[3], o.rb_last = in.rb[5];
    o.res[0] = sid;
    auto done = [&](uint32_t verdict, uint32_t flags, uint32_t copylen, uint32_t rcv_wnd) {
        o.res[1] = copylen, o.res[2] = rcv_wnd, o.res[3] = verdict | flags << 8;
        return o;
    };
    // 1. BAD_REQ
    if (sid > in.max_id || (in.req[5] | in.req[6] | in.req[7]) != 0 ||
        (rflags & ~(MTCP_GPU_RCVREAD_PEEK | MTCP_GPU_RCVREAD_ON_ACKQ)) != 0)
        return done(MTCP_GPU_RCVREAD_BAD_REQ, 0, 0, 0);
    const uint32_t need = len < in.rb[2] ? len : in.rb[2];                        // MIN(len, size)
    if (dst_off > in.dst_bytes || need > in.dst_bytes - dst_off) return done(MTCP_GPU_RCVREAD_BAD_REQ, 0, 0, 0);
    // 2. DUP
    if (in.dup) return done(MTCP_GPU_RCVREAD_DUP, 0, 0, 0);
    // 3. BAD_STATE
    const uint32_t head_seq = in.st[2], merged_len = in.st[3], size = in.st[4];
    const uint32_t nfrag = (in.st[7] >> 16) & 0xFFu, tcp_state = in.st[7] & 0xFFu;
    const uint32_t copylen = merged_len < len ? merged_len : len;                 // api.c:1102, :1121
    if (read_state_bad(in.st) || read_buf_bad(in.rb, in.arena_bytes) || size != in.rb[2] || merged_len > in.rb[5] ||
        (merged_len > 0 && (nfrag == 0 || in.st[8] != head_seq)) || (copylen > 0 && copylen > in.st[9]))
        return done(MTCP_GPU_RCVREAD_BAD_STATE, 0, 0, 0);
    // 4. DEFER_STATE
    const uint32_t more = merged_len > 0 ? MTCP_GPU_RCVREAD_MORE : 0u;
    if (tcp_state != MTCP_GPU_RCV_ST_ESTABLISHED) return done(MTCP_GPU_RCVREAD_DEFER_STATE, more, 0, in.st[1]);
    // 5. EAGAIN: api.c:1103-1106, :1122-1125
    if (copylen == 0) return done(MTCP_GPU_RCVREAD_EAGAIN, more, 0, in.st[1]);
    // the memcpy from rcvbuf->head: api.c:1109, :1129
    o.copylen = copylen;
    o.src = ((uint64_t)in.rb[1] << 32 | in.rb[0]) + in.rb[3];
    // 6. PEEKED
    if (rflags & MTCP_GPU_RCVREAD_PEEK) return done(MTCP_GPU_RCVREAD_PEEKED, more, copylen, in.st[1]);
    // 7. READ: RBRemove, tcp_ring_buffer.c:395-415
    uint32_t flags = 0;
    o.st_rec = true;
    o.rb_head = in.rb[3] + copylen;                                               // :395
    o.st[2] = head_seq + copylen;                                                 // :397
    o.st[3] = merged_len - copylen;                                               // :399
    o.rb_last = in.rb[5] - copylen;                                               // :400
    if (copylen == in.st[9]) {                                                    // :403-411
        // the live entries shift down, the freed slot (the last live one) is zero, the slots past it keep their value
        for (uint32_t k = 0; k + 1 < MTCP_GPU_RCV_MAX_FRAGS; ++k)
            if (k + 1 < nfrag) o.st[8 + 2 * k] = in.st[10 + 2 * k], o.st[9 + 2 * k] = in.st[11 + 2 * k];
        for (uint32_t k = 0; k < MTCP_GPU_RCV_MAX_FRAGS; ++k)
            if (k + 1 == nfrag) o.st[8 + 2 * k] = 0, o.st[9 + 2 * k] = 0;
        o.st[7] = (in.st[7] & 0xFF00FFFFu) | (nfrag - 1) << 16;
        flags |= MTCP_GPU_RCVREAD_FRAG_FREED;
    } else {                                                                      // :412-415
        o.st[8] = in.st[8] + copylen;
        o.st[9] = in.st[9] - copylen;
    }
    o.st[1] = size - o.st[3];                                                     // api.c:1131
    // api.c:1134-1145
    if (in.has_tx && in.need_wnd_adv == 1 && o.st[1] > in.eff_mss && !(rflags & MTCP_GPU_RCVREAD_ON_ACKQ)) {
        o.st_tx = true;
        flags |= MTCP_GPU_RCVREAD_WND_ADV;
    }
    if (o.st[3] > 0) flags |= MTCP_GPU_RCVREAD_MORE;
    return done(MTCP_GPU_RCVREAD_READ, flags, copylen, o.st[1]);
}

}  // namespace mg
