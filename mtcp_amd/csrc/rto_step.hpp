// rto_step.hpp — CheckRtmTimeout's firing test and HandleRTO for one ESTABLISHED
// stream with the AddtoSendList it ends in (mtcp/src/timer.c:380, :394-398,
// :176-337; mtcp/src/tcp_out.c:837-855), with the rules of
// include/mtcp_gpu_rtosweep.h on top.  One text, __host__ __device__: the sweep
// kernels (rtosweep_kernels.hpp) and tests/c/rto_step_test.cpp (a plain g++
// build under the sanitizers) run it.  No HIP call is made here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mtcp_gpu_rtosweep.h"

namespace mg {

// The firing test.  bits2: d_snd dword 21 (nrtx | on_rto << 8 | has_sndbuf <<
// 16 | rsvd << 24); ts_rto: dword 10.  on_rto == 1 and the slot's time has
// come (timer.c:380, for a stream the wheel holds in the slot of its ts_rto).
__host__ __device__ __forceinline__ bool rto_on(uint32_t bits2) { return ((bits2 >> 8) & 0xFFu) == 1u; }
__host__ __device__ __forceinline__ bool rto_due(uint32_t bits2, uint32_t ts_rto, uint32_t cur_ts) {
    return rto_on(bits2) && (int32_t)(cur_ts - ts_rto) >= 0;
}

// What the step reads of one stream: d_snd dwords 1, 3, 7, 9, 11, 14, 17-21
// (mss2, bits, bits2 as ack_step.hpp's AckState) and d_dtx dword 3 (on_send_list
// | on_control_list << 8 | rsvd << 16).
struct RtoIn {
    uint32_t snd_una, peer_wnd, cwnd, rto, srtt, rttvar;
    uint32_t sb_len, sb_size, mss2, bits, bits2, dflags;
};

// What the step stores: d_snd dwords 0, 7, 8, 9 (where st_win), 20 and 21
// (where st_bits), d_dtx byte 12 = 1 (where st_on); rec: dwords 1-3 of the
// stream's mtcp_gpu_rto_rec (rto, nrtx | verdict << 8 | flags << 16, 0).
struct RtoOut {
    uint32_t snd_nxt, cwnd, ssthresh, rto, bits, bits2;
    uint32_t rec[3];
    bool st_win, st_bits, st_on;
};

// The BAD test: d_snd by mtcp_gpu_ackwalk.h's rule, d_dtx by mtcp_gpu_datagen.h's.
__host__ __device__ __forceinline__ bool rto_bad(const RtoIn &s) {
    const uint32_t eff_mss = s.mss2 >> 16, wscale_peer = (s.bits >> 16) & 0xFFu;
    if ((s.bits2 >> 24) != 0 || eff_mss == 0 || wscale_peer > 31u || s.sb_size > MTCP_GPU_ACK_MAX_SIZE ||
        s.sb_len > s.sb_size)
        return true;
    return (s.dflags >> 16) || (s.dflags & 0xFFu) > 1u || ((s.dflags >> 8) & 0xFFu) > 1u;
}

// One handled stream: the stream was taken off the wheel (timer.c:394-397) and
// HandleRTO runs (:398).
__host__ __device__ __forceinline__ RtoOut rto_step(const RtoIn &s) {
    RtoOut o{};
    uint32_t nrtx = s.bits2 & 0xFFu, verdict, flags = 0;
    o.rto = s.rto, o.bits = s.bits, o.bits2 = s.bits2;
    if (rto_bad(s)) {
        verdict = MTCP_GPU_RTO_BAD;
    } else if ((s.bits & 0xFFu) != MTCP_GPU_ACK_ST_ESTABLISHED) {
        verdict = MTCP_GPU_RTO_DEFER_STATE;
    } else if (nrtx >= MTCP_GPU_ACK_MAX_RTX) {                                   // timer.c:186-206
        verdict = MTCP_GPU_RTO_LOST;
        o.bits2 = s.bits2 & 0xFFFF00FFu;                                        // timer.c:395-397
        o.bits = (s.bits & 0xFFFFFF00u) | MTCP_GPU_RTO_ST_CLOSED;               // timer.c:196
        o.st_bits = true;
    } else {
        verdict = MTCP_GPU_RTO_RETRANSMIT;
        nrtx += 1;                                                              // timer.c:187
        o.bits2 = (s.bits2 & 0xFFFF0000u) | nrtx;                               // on_rto = 0, timer.c:395-397
        o.st_bits = true;
        const uint32_t backoff = nrtx < MTCP_GPU_RTO_MAX_BACKOFF ? nrtx : MTCP_GPU_RTO_MAX_BACKOFF;   // timer.c:214
        const uint32_t rto = ((s.srtt >> 3) + s.rttvar) << backoff;             // timer.c:217-218
        if (rto != 0) o.rto = rto;                                              // timer.c:219-224
        const uint32_t mss = s.mss2 & 0xFFFFu;
        uint32_t ssthresh = (s.cwnd < s.peer_wnd ? s.cwnd : s.peer_wnd) / 2;    // timer.c:234
        if (ssthresh < 2 * mss) ssthresh = mss * 2;                             // timer.c:235-237
        o.ssthresh = ssthresh;
        o.cwnd = mss;                                                           // timer.c:238
        o.snd_nxt = s.snd_una;                                                  // timer.c:305
        o.st_win = true;
        if ((s.bits2 >> 16) & 0xFFu) {                                          // tcp_out.c:842-848
            if (!(s.dflags & 0xFFu)) o.st_on = true, flags |= MTCP_GPU_RTO_SEND_LIST_ADD;   // tcp_out.c:850-851
        }
    }
    o.rec[0] = o.rto;
    o.rec[1] = (o.bits2 & 0xFFu) | verdict << 8 | flags << 16;
    o.rec[2] = 0;
    return o;
}

}  // namespace mg
