// ack_step.hpp — ProcessACK for one packet of one ESTABLISHED stream
// (mtcp/src/tcp_in.c:302-531 with EstimateRTT, :249-300, SBRemove's
// bookkeeping, mtcp/src/tcp_send_buffer.c:149-173, and
// UpdateRetransmissionTimer, mtcp/src/timer.c:149-173), with the deferral rules
// of include/mtcp_gpu_ackwalk.h on top.  One function, __host__ __device__:
// the walk kernels (ackwalk_kernels.hpp), the host loop of
// tools/ackwalk_pattern.hip and tests/c/ack_step_test.cpp (a plain g++ build
// under the sanitizers) all run this text.  No HIP call is made here.
//
// The reference's statements in the reference's order; where two forms differ
// only at wrap or truncation the reference's form stands (the header's
// contract names each).  The step works on copies and commits at its exit, so
// a deferred packet changes nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mtcp_gpu_ackwalk.h"

namespace mg {

// bits 24-31 of a walk input's last word (the gather writes them)
constexpr uint32_t kAckInNoPayload = 1;     // payload_len == 0
constexpr uint32_t kAckInValid = 2;         // the placement verdict is 12-15: ValidateSequence returned TRUE
constexpr uint32_t kAckInRcvDeferred = 4;   // the placement verdict is anything but 7-15
constexpr uint32_t kAckInHasTs = 8;         // an option record with MTCP_GPU_TCPOPT_TS_FOUND

// TCP_SEQ_* (tcp_in.h:37-41)
__host__ __device__ __forceinline__ bool ack_seq_lt(uint32_t a, uint32_t b) { return (int32_t)(a - b) < 0; }
__host__ __device__ __forceinline__ bool ack_seq_gt(uint32_t a, uint32_t b) { return (int32_t)(a - b) > 0; }
__host__ __device__ __forceinline__ bool ack_seq_geq(uint32_t a, uint32_t b) { return (int32_t)(a - b) >= 0; }

// Bytes 0-87 of one mtcp_gpu_ack_state in registers.  mss2: mss | eff_mss << 16;
// bits: tcp_state | saw_timestamp << 8 | wscale_peer << 16 | dup_acks << 24;
// bits2: nrtx | on_rto << 8 | has_sndbuf << 16 | rsvd << 24.
struct AckState {
    uint32_t snd_nxt, snd_una, snd_wnd, peer_wnd;
    uint32_t snd_wl1, snd_wl2, last_ack_seq, cwnd;
    uint32_t ssthresh, rto, ts_rto, srtt;
    uint32_t mdev, mdev_max, rttvar, rtt_seq;
    uint32_t sb_head_seq, sb_len, sb_size, mss2;
    uint32_t bits, bits2;
};
static_assert(sizeof(AckState) == 88, "bytes 0-87 of mtcp_gpu_ack_state");

// An ACK record as one 16 B piece: w = flags | verdict << 16 | dup_acks << 24.
__host__ __device__ __forceinline__ uint4 ack_rec(uint32_t rmlen, uint32_t snd_nxt, uint32_t cwnd, uint32_t flags,
                                                  uint32_t verdict, uint32_t dup_acks) {
    uint4 r;
    r.x = rmlen, r.y = snd_nxt, r.z = cwnd, r.w = flags | verdict << 16 | dup_acks << 24;
    return r;
}

// The 16 B pieces of the record a walked packet may have changed: 1 for
// pieces 0, 1 and 5 (ACK_OLD and ACK_NEW), 2 for pieces 2, 3 and 4 (ACK_NEW; a
// fast retransmit's ssthresh).
__host__ __device__ __forceinline__ uint32_t ack_dirty(const uint4 rec) {
    const uint32_t v = (rec.w >> 16) & 0xFFu;
    if (v < MTCP_GPU_ACK_ACK_OLD) return 0;
    return 1u | ((v == MTCP_GPU_ACK_ACK_NEW || (rec.w & MTCP_GPU_ACK_FAST_RTX)) ? 2u : 0u);
}

// One packet.  in: seq, ack_seq, ts_ref, window | tcp_flags << 16 | kAckIn* <<
// 24.  `deferred`: an earlier packet of this stream in this batch was deferred;
// set when this one is.  Nothing of s changes then.
__host__ __device__ __forceinline__ uint4 ack_step(AckState &s, const uint4 in, const uint32_t cur_ts, bool &deferred) {
    if (deferred) return ack_rec(0, 0, 0, 0, MTCP_GPU_ACK_DEFER_BEHIND, 0);
    const uint32_t seq = in.x, ack_seq = in.y, ts_ref = in.z;
    const uint32_t window = in.w & 0xFFFFu, tcp_flags = (in.w >> 16) & 0xFFu, ib = in.w >> 24;
    const uint32_t mss = s.mss2 & 0xFFFFu, eff_mss = s.mss2 >> 16;
    const uint32_t saw_ts = (s.bits >> 8) & 0xFFu, wscale = (s.bits >> 16) & 0xFFu;
    uint32_t dup_acks = s.bits >> 24, nrtx = s.bits2 & 0xFFu, on_rto = (s.bits2 >> 8) & 0xFFu;
    uint32_t dv = 0;
    if ((s.bits2 >> 24) != 0 || eff_mss == 0 || wscale > 31 || s.sb_size > MTCP_GPU_ACK_MAX_SIZE || s.sb_len > s.sb_size)
        dv = MTCP_GPU_ACK_DEFER_BAD_STATE;
    else if ((s.bits & 0xFFu) != MTCP_GPU_ACK_ST_ESTABLISHED) dv = MTCP_GPU_ACK_DEFER_STATE;
    else if (tcp_flags & 0x07u) dv = MTCP_GPU_ACK_DEFER_FLAGS;                  // FIN, SYN, RST
    else if ((ib & kAckInRcvDeferred) || ((ib & kAckInValid) && saw_ts && !(ib & kAckInHasTs)))
        dv = MTCP_GPU_ACK_DEFER_RCV;
    if (dv) {
        deferred = true;
        return ack_rec(0, 0, 0, 0, dv, 0);
    }
    if (!(ib & kAckInValid)) return ack_rec(0, s.snd_nxt, s.cwnd, 0, MTCP_GPU_ACK_NOT_VALID, dup_acks);
    if (!(tcp_flags & 0x10u)) return ack_rec(0, s.snd_nxt, s.cwnd, 0, MTCP_GPU_ACK_NO_ACK_FLAG, dup_acks);    // :864
    if (!((s.bits2 >> 16) & 0xFFu)) return ack_rec(0, s.snd_nxt, s.cwnd, 0, MTCP_GPU_ACK_NO_SNDBUF, dup_acks);  // :865

    // ProcessACK, tcp_in.c:302-531 (tcph->syn is clear, the state ESTABLISHED)
    uint32_t flags = 0;
    const uint32_t cwindow = window << wscale;                                  // :315-318
    const uint32_t right_wnd_edge = s.peer_wnd + s.snd_wl2;                     // :319
    if (ack_seq_gt(ack_seq, s.sb_head_seq + s.sb_len))                          // :332-338
        return ack_rec(0, s.snd_nxt, s.cwnd, 0, MTCP_GPU_ACK_ACK_BEYOND, dup_acks);
    uint32_t peer_wnd = s.peer_wnd, wl1 = s.snd_wl1, wl2 = s.snd_wl2, last_ack = s.last_ack_seq;
    uint32_t snd_nxt = s.snd_nxt, cwnd = s.cwnd, ssthresh = s.ssthresh;
    if (ack_seq_lt(wl1, seq) || (wl1 == seq && ack_seq_lt(wl2, ack_seq)) ||
        (wl2 == ack_seq && cwindow > peer_wnd)) {                               // :341-349
        const uint32_t cwindow_prev = peer_wnd;
        peer_wnd = cwindow, wl1 = seq, wl2 = ack_seq;
        flags |= MTCP_GPU_ACK_WND_UPDATE;
        if (cwindow_prev < snd_nxt - s.snd_una && peer_wnd >= snd_nxt - s.snd_una)   // :355-363
            flags |= MTCP_GPU_ACK_WRITE_EVENT_WND;
    }
    bool dup = false;                                                           // :375-389
    if (ack_seq_lt(ack_seq, snd_nxt) && ack_seq == last_ack && (ib & kAckInNoPayload) &&
        wl2 + peer_wnd == right_wnd_edge) {
        dup_acks = (dup_acks + 1) & 0xFFu;                                      // :379 holds in int; the uint8_t wraps
        dup = true;
        flags |= MTCP_GPU_ACK_DUP;
    }
    if (!dup) dup_acks = 0, last_ack = ack_seq;
    if (dup && dup_acks == 3) {                                                 // :392-426
        if (ack_seq_lt(ack_seq, snd_nxt)) snd_nxt = ack_seq;
        ssthresh = (cwnd < peer_wnd ? cwnd : peer_wnd) / 2;
        if (ssthresh < 2 * mss) ssthresh = 2 * mss;
        cwnd = ssthresh + 3 * mss;
        if (nrtx < MTCP_GPU_ACK_MAX_RTX) nrtx++;
        flags |= MTCP_GPU_ACK_FAST_RTX;
    } else if (dup_acks > 3) {                                                  // :428-435
        if ((uint32_t)(cwnd + mss) > cwnd) cwnd += mss;
    }
    if (ack_seq_gt(ack_seq, snd_nxt)) {                                         // :444-455
        snd_nxt = ack_seq;
        flags |= MTCP_GPU_ACK_SND_NXT_RECOVERED;
        if (s.sb_len == 0) flags |= MTCP_GPU_ACK_SEND_LIST_REMOVE;
    }
    if (ack_seq_geq(s.sb_head_seq, ack_seq)) {                                  // :459-461
        s.peer_wnd = peer_wnd, s.snd_wl1 = wl1, s.snd_wl2 = wl2, s.last_ack_seq = last_ack;
        s.snd_nxt = snd_nxt, s.cwnd = cwnd, s.ssthresh = ssthresh;
        s.bits = (s.bits & 0x00FFFFFFu) | dup_acks << 24;
        s.bits2 = (s.bits2 & 0xFFFFFF00u) | nrtx;
        return ack_rec(0, snd_nxt, cwnd, flags, MTCP_GPU_ACK_ACK_OLD, dup_acks);
    }

    const uint32_t rmlen = ack_seq - s.sb_head_seq;                             // :464; not 0 behind :459
    uint32_t packets = (rmlen / eff_mss) & 0xFFFFu;                             // :467-473, a uint16_t
    if ((rmlen / eff_mss) * eff_mss > rmlen) packets = (packets + 1) & 0xFFFFu;
    uint32_t srtt = s.srtt, mdev = s.mdev, mdev_max = s.mdev_max, rttvar = s.rttvar, rtt_seq = s.rtt_seq, rto = s.rto;
    if (saw_ts) {                                                               // :476-480; EstimateRTT, :249-300
        int64_t m = (uint32_t)(cur_ts - ts_ref);                                // ts_lastack_rcvd, :138
        if (m == 0) m = 1;
        if (srtt != 0) {
            m -= (srtt >> 3);
            srtt = (uint32_t)((int64_t)srtt + m);
            if (m < 0) {
                m = -m;
                m -= (mdev >> 2);
                if (m > 0) m >>= 3;
            } else {
                m -= (mdev >> 2);
            }
            mdev = (uint32_t)((int64_t)mdev + m);
            if (mdev > mdev_max) {
                mdev_max = mdev;
                if (mdev_max > rttvar) rttvar = mdev_max;
            }
            if (ack_seq_gt(s.snd_una, rtt_seq)) {
                if (mdev_max < rttvar) rttvar -= (rttvar - mdev_max) >> 2;
                rtt_seq = snd_nxt;
                mdev_max = 0;                                                   // TCP_RTO_MIN, :253
            }
        } else {
            srtt = (uint32_t)(m << 3);
            mdev = (uint32_t)(m << 1);
            mdev_max = rttvar = mdev;                                           // MAX(mdev, 0)
            rtt_seq = snd_nxt;
        }
        rto = (srtt >> 3) + rttvar;
    }
    if (cwnd < ssthresh) {                                                      // :487-504
        if ((uint32_t)(cwnd + mss) > cwnd) {
            if ((uint64_t)mss * packets > 0x7FFFFFFFull) {                      // an int product, :490
                deferred = true;
                return ack_rec(0, 0, 0, 0, MTCP_GPU_ACK_DEFER_ARITH, 0);
            }
            cwnd += mss * packets;
        }
    } else {
        if ((uint64_t)packets * mss * mss > 0x7FFFFFFFull || cwnd == 0) {       // an int product, then / cwnd, :495-497
            deferred = true;
            return ack_rec(0, 0, 0, 0, MTCP_GPU_ACK_DEFER_ARITH, 0);
        }
        const uint32_t new_cwnd = cwnd + packets * mss * mss / cwnd;
        if (new_cwnd > cwnd) cwnd = new_cwnd;
    }
    uint32_t sb_head_seq = s.sb_head_seq, sb_len = s.sb_len;                    // SBRemove, tcp_send_buffer.c:149-173
    const uint32_t to_remove = rmlen < sb_len ? rmlen : sb_len;
    sb_head_seq += to_remove, sb_len -= to_remove;
    const uint32_t snd_wnd_prev = s.snd_wnd;                                    // :512-524
    if (snd_wnd_prev == 0) flags |= MTCP_GPU_ACK_WRITE_EVENT_ROOM;
    nrtx = 0;                                                                   // UpdateRetransmissionTimer, timer.c:149-173
    uint32_t ts_rto = s.ts_rto;
    if (on_rto) flags |= MTCP_GPU_ACK_RTO_REMOVE, on_rto = 0;
    if (ack_seq_gt(snd_nxt, ack_seq)) {                                         // snd_una is ack_seq by now
        ts_rto = cur_ts + rto;
        on_rto = 1;
        flags |= MTCP_GPU_ACK_RTO_ADD;
    }
    s.snd_nxt = snd_nxt, s.snd_una = ack_seq, s.snd_wnd = s.sb_size - sb_len, s.peer_wnd = peer_wnd;
    s.snd_wl1 = wl1, s.snd_wl2 = wl2, s.last_ack_seq = last_ack, s.cwnd = cwnd;
    s.ssthresh = ssthresh, s.rto = rto, s.ts_rto = ts_rto, s.srtt = srtt;
    s.mdev = mdev, s.mdev_max = mdev_max, s.rttvar = rttvar, s.rtt_seq = rtt_seq;
    s.sb_head_seq = sb_head_seq, s.sb_len = sb_len;
    s.bits = (s.bits & 0x00FFFFFFu) | dup_acks << 24;
    s.bits2 = (s.bits2 & 0xFFFF0000u) | nrtx | on_rto << 8;
    return ack_rec(to_remove, snd_nxt, cwnd, flags, MTCP_GPU_ACK_ACK_NEW, dup_acks);
}

}  // namespace mg
