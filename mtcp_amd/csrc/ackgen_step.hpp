// ackgen_step.hpp — EnqueueACK's count, WriteTCPACKList's plan for one stream
// and SendTCPPacket's record for one pure ACK (mtcp/src/tcp_out.c:911-935,
// :697-761, :220-354; mtcp/src/ip_out.c:139), with the rules of
// include/mtcp_gpu_ackgen.h on top.  One text, __host__ __device__: the
// kernels (ackgen_kernels.hpp) and tests/c/ackgen_step_test.cpp (a plain g++
// build under the sanitizers, with a host loop over it) run it.  No HIP call
// is made here.
//
// Four pieces: the fold of one packet's placement word (and of 64 of them
// given as masks, for the wave), the plan of one stream (the BAD test, to_ack,
// the planned count), the record of one frame, the commit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mtcp_gpu_ackgen.h"

namespace mg {

// One mtcp_gpu_ackgen_state as its eight dwords.  id_cnt: ip_id | ack_cnt << 16
// | is_wack << 24; misc: wscale_mine | link << 8 | has_rcvbuf << 16 |
// need_wnd_adv << 24.
struct AckGenTx {
    uint32_t saddr, daddr, ports, id_cnt, misc, ts_lastack_sent, rsvd0, rsvd1;
};
static_assert(sizeof(AckGenTx) == 32, "mtcp_gpu_ackgen_state");

// The fold's state: the count in bits 0-5, and what the list had.
constexpr uint32_t kAckgenAny = 0x40u;   // a packet with an EnqueueACK: the stream is on the ack list
constexpr uint32_t kAckgenPut = 0x80u;   // a PUT_* verdict: tcp_in.c:555-566 allocated the receive buffer

// w: the last dword of a placement record, put_len | verdict << 16 | flags << 24.
__host__ __device__ __forceinline__ uint32_t ackgen_fold(uint32_t f, uint32_t w) {
    const uint32_t flags = w >> 24, verdict = (w >> 16) & 0xFFu;
    uint32_t cnt = f & 63u;
    if (flags & MTCP_GPU_RCV_ACK_NOW) cnt = (cnt + 1u) & 63u;               // tcp_out.c:923-926, a 6-bit field
    if ((flags & MTCP_GPU_RCV_ACK_AGGREGATE) && cnt == 0) cnt = 1;          // tcp_out.c:927-930
    f = (f & ~63u) | cnt;
    if (flags & (MTCP_GPU_RCV_ACK_NOW | MTCP_GPU_RCV_ACK_AGGREGATE)) f |= kAckgenAny;   // tcp_out.c:934
    if (verdict >= MTCP_GPU_RCV_PUT_DROPPED && verdict <= MTCP_GPU_RCV_PUT_STORED) f |= kAckgenPut;
    return f;
}
__host__ __device__ __forceinline__ bool ackgen_is_put(uint32_t w) {
    const uint32_t verdict = (w >> 16) & 0xFFu;
    return verdict >= MTCP_GPU_RCV_PUT_DROPPED && verdict <= MTCP_GPU_RCV_PUT_STORED;
}

// The same fold over up to 64 packets in list order, packet i being bit i of
// the masks: now, agg: its flags; put: ackgen_is_put.  Exact: an AGGREGATE
// acts only where the count is 0 when it is reached, so the NOWs up to and
// including each AGGREGATE's position are added first (a packet with both
// bits applies NOW first); once the count is not 0 and the NOWs left cannot
// wrap it, no AGGREGATE that is left can act.
__host__ __device__ __forceinline__ uint32_t ackgen_fold_masks(uint32_t f, uint64_t now, uint64_t agg, uint64_t put) {
    uint32_t cnt = f & 63u;
    if (now | agg) f |= kAckgenAny;
    if (put) f |= kAckgenPut;
    while (agg) {
        if (cnt != 0 && cnt + (uint32_t)__builtin_popcountll(now) < 64u) break;
        const uint64_t low = agg & (~agg + 1ull);
        const uint64_t upto = low | (low - 1ull);
        cnt = (cnt + (uint32_t)__builtin_popcountll(now & upto)) & 63u;
        if (cnt == 0) cnt = 1;
        now &= ~upto, agg &= ~upto;
    }
    cnt = (cnt + (uint32_t)__builtin_popcountll(now)) & 63u;
    return (f & ~63u) | cnt;
}

// The BAD test of a tx record.
__host__ __device__ __forceinline__ bool ackgen_bad(const AckGenTx &t, uint32_t n_links) {
    const uint32_t cnt = (t.id_cnt >> 16) & 0xFFu, wack = t.id_cnt >> 24;
    const uint32_t wscale = t.misc & 0xFFu, link = (t.misc >> 8) & 0xFFu, has = (t.misc >> 16) & 0xFFu, nwa = t.misc >> 24;
    return t.rsvd0 || t.rsvd1 || cnt > 63u || wack > 1u || has > 1u || nwa > 1u || wscale > 31u || link >= n_links;
}

// What the emit and the commit need of one segment, 32 B in the workspace.
// win_id: the wire window | ip_id << 16.  meta: ack_cnt after the fold (bits
// 0-5; 0 with NOT_TO_ACK) | is_wack << 6 | has_rcvbuf << 7 | link << 8 |
// status << 16 | ON_LIST << 19 | (window32 == 0) << 20 | need_wnd_adv << 21 |
// wscale_mine << 24.  The status is the plan's: SENT stands for "emits", and
// the commit makes it NO_ROOM where the room cut it.
struct AckGenPlan {
    uint32_t saddr, daddr, ports, snd_nxt, rcv_nxt, ts_recent, win_id, meta;
};
static_assert(sizeof(AckGenPlan) == 32, "two 16 B pieces");

__host__ __device__ __forceinline__ uint32_t ackgen_status(const AckGenPlan &p) { return (p.meta >> 16) & 7u; }
// frames planned: ack_cnt plain ACKs, then the probe (tcp_out.c:729-748)
__host__ __device__ __forceinline__ uint32_t ackgen_planned(const AckGenPlan &p) {
    return ackgen_status(p) == MTCP_GPU_ACKGEN_SENT ? (p.meta & 63u) + ((p.meta >> 6) & 1u) : 0u;
}

// TCP_SEQ_LEQ (tcp_in.h:37-41)
__host__ __device__ __forceinline__ bool ackgen_seq_leq(uint32_t a, uint32_t b) { return (int32_t)(a - b) <= 0; }

// The plan of one stream.  t: its record, not BAD; f: the fold's result from
// the record's ack_cnt over the walked part of its list; deferred: the list
// has a host tail; the rest: d_state[id] and d_snd[id].snd_nxt.
__host__ __device__ __forceinline__ AckGenPlan ackgen_plan(const AckGenTx &t, uint32_t f, bool deferred,
                                                           uint32_t rcv_nxt, uint32_t rcv_wnd, uint32_t head_seq,
                                                           uint32_t merged_len, uint32_t ts_recent,
                                                           uint32_t snd_nxt) {
    const uint32_t cnt0 = (t.id_cnt >> 16) & 63u, wack0 = (t.id_cnt >> 24) & 1u;
    const uint32_t wscale = t.misc & 31u, link = (t.misc >> 8) & 0xFFu;
    const uint32_t has = ((t.misc >> 16) & 1u) | ((f & kAckgenPut) ? 1u : 0u);
    const uint32_t nwa = (t.misc >> 24) & 1u;
    const bool on_list = (f & kAckgenAny) || cnt0 || wack0;
    const uint32_t window32 = rcv_wnd >> wscale;                            // tcp_out.c:301
    const uint32_t wire = window32 < 65535u ? window32 : 65535u;            // tcp_out.c:302
    uint32_t cnt = f & 63u, wack = wack0, status;
    if (deferred) {
        status = MTCP_GPU_ACKGEN_DEFERRED;
    } else if (!on_list) {
        status = MTCP_GPU_ACKGEN_IDLE;
    } else if (!(has && ackgen_seq_leq(rcv_nxt, head_seq + merged_len))) {  // tcp_out.c:708-714
        status = MTCP_GPU_ACKGEN_NOT_TO_ACK;                                // tcp_out.c:755-761
        cnt = 0, wack = 0;
    } else {
        status = MTCP_GPU_ACKGEN_SENT;
    }
    AckGenPlan p;
    p.saddr = t.saddr, p.daddr = t.daddr, p.ports = t.ports;
    p.snd_nxt = snd_nxt, p.rcv_nxt = rcv_nxt, p.ts_recent = ts_recent;
    p.win_id = wire | (t.id_cnt & 0xFFFFu) << 16;
    p.meta = cnt | wack << 6 | has << 7 | link << 8 | status << 16 | (on_list ? 1u << 19 : 0u) |
             (window32 == 0 ? 1u << 20 : 0u) | nwa << 21 | wscale << 24;
    return p;
}

// The plan of a segment that is no stream's, or whose record is BAD.
__host__ __device__ __forceinline__ AckGenPlan ackgen_plan_none(uint32_t status) {
    AckGenPlan p{};
    p.meta = status << 16;
    return p;
}

// Frame i of a stream as the twelve dwords of a mtcp_gpu_tx_seg: i below the
// count is a plain ACK, i equal to it the probe (tcp_out.c:266, :284, :289;
// ip_out.c:139).
__host__ __device__ __forceinline__ void ackgen_record(const AckGenPlan &p, uint32_t i, uint32_t cur_ts, uint32_t out[12]) {
    const uint32_t cnt = p.meta & 63u, link = (p.meta >> 8) & 0xFFu;
    const uint32_t ip_id = ((p.win_id >> 16) + i) & 0xFFFFu;
    out[0] = 0, out[1] = 0;                                                 // payload_off
    out[2] = p.saddr, out[3] = p.daddr, out[4] = p.ports;
    out[5] = i < cnt ? p.snd_nxt : p.snd_nxt - 1u;
    out[6] = p.rcv_nxt;
    out[7] = cur_ts, out[8] = p.ts_recent;                                  // tcp_out.c:118-122
    out[9] = (p.win_id & 0xFFFFu) | ip_id << 16;
    out[10] = 0;                                                            // payload_len, mss
    out[11] = MTCP_GPU_TXB_FLAG_ACK | 1u << 8 | link << 24;                 // form 1, wscale 0
}

// The commit of a stream whose first record is S, E being the records the
// call has room for: dwords 3, 4 and 5 of its tx record (tx[2] only where
// *store_ts) and its result, 16 B.  first: S capped at the call's total.
__host__ __device__ __forceinline__ void ackgen_commit(const AckGenPlan &p, uint32_t S, uint32_t E, uint32_t first,
                                                       uint32_t cur_ts, uint32_t tx[3], bool *store_ts,
                                                       uint32_t res[4]) {
    const uint32_t planned = ackgen_planned(p);
    const uint32_t cnt = p.meta & 63u, wack = (p.meta >> 6) & 1u, has = (p.meta >> 7) & 1u;
    const uint32_t link = (p.meta >> 8) & 0xFFu, wscale = (p.meta >> 24) & 31u;
    const uint32_t left = S < E ? E - S : 0u;
    const uint32_t e = planned < left ? planned : left;
    const uint32_t n_ack = e < cnt ? e : cnt;                               // tcp_out.c:729-737
    const uint32_t probe = e > cnt ? 1u : 0u;                               // tcp_out.c:740-748
    uint32_t status = ackgen_status(p);
    if (e < planned) status = MTCP_GPU_ACKGEN_NO_ROOM;
    const bool set_nwa = e && ((p.meta >> 20) & 1u);                        // tcp_out.c:304-306
    const uint32_t nwa = ((p.meta >> 21) & 1u) | (set_nwa ? 1u : 0u);
    tx[0] = (((p.win_id >> 16) + e) & 0xFFFFu) | (cnt - n_ack) << 16 | (wack & ~probe) << 24;
    tx[1] = wscale | link << 8 | has << 16 | nwa << 24;
    tx[2] = cur_ts;                                                         // tcp_out.c:290
    *store_ts = e != 0;
    const uint32_t flags = ((p.meta >> 19) & 1u ? MTCP_GPU_ACKGEN_ON_LIST : 0u) |
                           (set_nwa ? MTCP_GPU_ACKGEN_NEED_WND_ADV : 0u);
    res[0] = first;
    res[1] = n_ack | probe << 8 | status << 16 | flags << 24;
    res[2] = p.rcv_nxt;
    res[3] = p.win_id & 0xFFFFu;
}

// The records a call has room for: k < seg_cap, frame k ends at or before
// buf_len, its offset fits 32 bits (mtcp_gpu_txseg.h's rule; all three are
// monotone in k).
inline uint32_t ackgen_room(uint64_t buf_off, uint64_t buf_len, uint32_t off_shift, uint32_t slot, uint32_t seg_cap) {
    const uint64_t lim = 0xFFFFFFFFull << off_shift;
    if (buf_off > lim || buf_len < MTCP_GPU_ACKGEN_FRAME_LEN || buf_off > buf_len - MTCP_GPU_ACKGEN_FRAME_LEN) return 0;
    const uint64_t last = lim < buf_len - MTCP_GPU_ACKGEN_FRAME_LEN ? lim : buf_len - MTCP_GPU_ACKGEN_FRAME_LEN;
    const uint64_t fit = (last - buf_off) / slot + 1;
    return fit < seg_cap ? (uint32_t)fit : seg_cap;
}
inline uint32_t ackgen_slot(uint32_t off_shift, uint32_t slot_bytes) {
    const uint32_t a = off_shift ? 1u << off_shift : 2u;
    return slot_bytes ? slot_bytes : (MTCP_GPU_ACKGEN_FRAME_LEN + a - 1) & ~(a - 1);
}

}  // namespace mg
