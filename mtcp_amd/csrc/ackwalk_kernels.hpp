// ackwalk_kernels.hpp — gfx950 kernels of the per-stream ProcessACK walk (SURVEY
// §8 row f13): ProcessACK (mtcp/src/tcp_in.c:302-531) with EstimateRTT
// (:249-300), SBRemove's bookkeeping (mtcp/src/tcp_send_buffer.c:149-173) and
// UpdateRetransmissionTimer (mtcp/src/timer.c:149-173) for every stream of a
// grouped batch, behind the receive walk.  include/mtcp_gpu_ackwalk.h has the
// contract, ack_step.hpp the walk of one packet.
//
// Two launches, ordered by the stream, in the shape of rcvwalk_kernels.hpp:
//
//   gather  one lane per position j of d_idx: the 16 B walk input of packet
//           d_idx[j] (seq, ack_seq, ts_ref, window | tcp_flags << 16 | bits <<
//           24; the bits: no payload, the placement verdict valid, the
//           placement verdict deferred, a timestamp record) to position j of
//           the workspace; and d_ack[j] = 0, so that every ACK record is
//           written whatever the lists hold;
//   walk    one lane per segment of the group's table, 64 consecutive segments
//           a wave.  The lanes walk their own segments in rounds of
//           kAckShortLen packets while more than kAckWaveMax of them have
//           packets left; the wave then takes what is left one segment after
//           the other: 64 inputs loaded coalesced, the state in scalar
//           registers (v_readlane with a uniform lane), lane k keeping the
//           record of step k, 64 records stored at once.
//
// The two constants are the receive walk's (DESIGN §8 f11 measured them; f13
// inherits them).  The state is 22 dwords: bytes 0-87 of a record, loaded as
// five 16 B pieces and one 8 B piece; only the pieces a walked packet can have
// changed are stored, and never bytes 88-127.  No workgroup waits on another,
// no atomic, no LDS; every loop's trip count is fixed by the segment table
// clamped to n; every store is bounded by n, max_id and min(d_nseg[0], n).  A
// long list is serial by nature, as in the receive walk.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mtcp_gpu.h"
#include "../../include/mtcp_gpu_ackwalk.h"
#include "ack_step.hpp"
#include "rcvwalk_kernels.hpp"   // rcv_bcast; kWave, kBlock through rx_kernels.hpp

namespace mg {

constexpr uint32_t kAckShortLen = kRcvShortLen;   // packets a lane walks per round
constexpr uint32_t kAckWaveMax = kRcvWaveMax;     // the wave form takes over when at most this many lanes have packets left

struct AckWork {
    uint64_t in_off, bytes;
};
inline AckWork ack_work(uint32_t n) {
    AckWork w{};
    w.in_off = 0;
    w.bytes = n ? 16ull * n : 16ull;
    return w;
}

// ---- gather -------------------------------------------------------------------
// grid: one lane per position.  res: 40 B records; opt: 16 B records or NULL;
// place: the receive walk's 16 B records.
__global__ __launch_bounds__(kBlock) void ackwalk_gather_kernel(const uint8_t *__restrict__ res,
                                                                const uint4 *__restrict__ opt,
                                                                const uint4 *__restrict__ place,
                                                                const uint32_t *__restrict__ idx, uint32_t n,
                                                                uint4 *__restrict__ win, uint4 *__restrict__ ack) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    const uint32_t p = idx[j];
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (p < n) {
        const uint32_t *r = reinterpret_cast<const uint32_t *>(res + 40ull * p);
        const uint32_t w8 = r[8];                                 // payload_len | ihl_doff << 16 | tcp_flags << 24
        const uint32_t pv = (place[p].w >> 16) & 0xFFu;           // enum mtcp_gpu_rcv_verdict
        uint32_t bits = (w8 & 0xFFFFu) == 0 ? kAckInNoPayload : 0u;
        if (pv >= MTCP_GPU_RCV_ACK_ONLY && pv <= MTCP_GPU_RCV_PUT_STORED) bits |= kAckInValid;
        else if (!(pv >= MTCP_GPU_RCV_PAWS_NO_TS && pv <= MTCP_GPU_RCV_SEQ_AHEAD)) bits |= kAckInRcvDeferred;
        v.x = r[3];                                               // seq
        v.y = r[4];                                               // ack_seq
        if (opt) {
            const uint4 o = opt[p];
            v.z = o.y;                                            // ts_ref
            if ((o.w >> 24) & MTCP_GPU_TCPOPT_TS_FOUND) bits |= kAckInHasTs;
        }
        v.w = (r[5] & 0xFFFFu) | (w8 >> 24) << 16 | bits << 24;   // window
    }
    win[j] = v;
    ack[j] = make_uint4(0u, 0u, 0u, 0u);
}

// ---- walk ---------------------------------------------------------------------
// rec: the record's first byte.  Bytes 0-87 and no more.
__device__ __forceinline__ void ack_load_state(AckState &s, const uint4 *__restrict__ rec) {
    const uint4 a = rec[0], b = rec[1], c = rec[2], d = rec[3], e = rec[4];
    const uint2 f = *reinterpret_cast<const uint2 *>(rec + 5);
    s.snd_nxt = a.x, s.snd_una = a.y, s.snd_wnd = a.z, s.peer_wnd = a.w;
    s.snd_wl1 = b.x, s.snd_wl2 = b.y, s.last_ack_seq = b.z, s.cwnd = b.w;
    s.ssthresh = c.x, s.rto = c.y, s.ts_rto = c.z, s.srtt = c.w;
    s.mdev = d.x, s.mdev_max = d.y, s.rttvar = d.z, s.rtt_seq = d.w;
    s.sb_head_seq = e.x, s.sb_len = e.y, s.sb_size = e.z, s.mss2 = e.w;
    s.bits = f.x, s.bits2 = f.y;
}
// dirty: ack_dirty's bits.  Bytes 88-127 are never written.
__device__ __forceinline__ void ack_store_state(const AckState &s, uint4 *__restrict__ rec, uint32_t dirty) {
    if (dirty & 1u) {
        rec[0] = make_uint4(s.snd_nxt, s.snd_una, s.snd_wnd, s.peer_wnd);
        rec[1] = make_uint4(s.snd_wl1, s.snd_wl2, s.last_ack_seq, s.cwnd);
        *reinterpret_cast<uint2 *>(rec + 5) = make_uint2(s.bits, s.bits2);
    }
    if (dirty & 2u) {
        rec[2] = make_uint4(s.ssthresh, s.rto, s.ts_rto, s.srtt);
        rec[3] = make_uint4(s.mdev, s.mdev_max, s.rttvar, s.rtt_seq);
        rec[4] = make_uint4(s.sb_head_seq, s.sb_len, s.sb_size, s.mss2);
    }
}
__device__ __forceinline__ AckState ack_bcast_state(const AckState &s, int l) {
    AckState u;
    u.snd_nxt = rcv_bcast(s.snd_nxt, l), u.snd_una = rcv_bcast(s.snd_una, l);
    u.snd_wnd = rcv_bcast(s.snd_wnd, l), u.peer_wnd = rcv_bcast(s.peer_wnd, l);
    u.snd_wl1 = rcv_bcast(s.snd_wl1, l), u.snd_wl2 = rcv_bcast(s.snd_wl2, l);
    u.last_ack_seq = rcv_bcast(s.last_ack_seq, l), u.cwnd = rcv_bcast(s.cwnd, l);
    u.ssthresh = rcv_bcast(s.ssthresh, l), u.rto = rcv_bcast(s.rto, l);
    u.ts_rto = rcv_bcast(s.ts_rto, l), u.srtt = rcv_bcast(s.srtt, l);
    u.mdev = rcv_bcast(s.mdev, l), u.mdev_max = rcv_bcast(s.mdev_max, l);
    u.rttvar = rcv_bcast(s.rttvar, l), u.rtt_seq = rcv_bcast(s.rtt_seq, l);
    u.sb_head_seq = rcv_bcast(s.sb_head_seq, l), u.sb_len = rcv_bcast(s.sb_len, l);
    u.sb_size = rcv_bcast(s.sb_size, l), u.mss2 = rcv_bcast(s.mss2, l);
    u.bits = rcv_bcast(s.bits, l), u.bits2 = rcv_bcast(s.bits2, l);
    return u;
}

// grid: one lane per segment, for n segments (m is known only on the device;
// a wave whose first segment is at or past m ends at once).  SHORT: the
// packets a lane walks per round; WAVE_MAX: the lanes' rounds go on while more
// lanes than this have packets left.  snd: 128 B records, 8 pieces each.
template <uint32_t SHORT, uint32_t WAVE_MAX>
__global__ __launch_bounds__(kBlock) void ackwalk_walk_kernel(const uint4 *__restrict__ win,
                                                              const uint32_t *__restrict__ idx, uint32_t n,
                                                              uint32_t max_id, const uint32_t *__restrict__ seg_sid,
                                                              const uint32_t *__restrict__ seg_start,
                                                              const uint32_t *__restrict__ nseg, uint32_t cur_ts,
                                                              uint4 *__restrict__ snd, uint4 *__restrict__ ack,
                                                              uint32_t *__restrict__ ack_stop) {
    const uint32_t m = min(nseg[0], n);
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t j0 = (blockIdx.x * kBlock + threadIdx.x) - lane;
    if (j0 >= m) return;                                          // the whole wave
    const uint32_t j = j0 + lane;
    const bool valid = j < m;
    uint32_t start = 0, end = 0, sid = 0xFFFFFFFFu;
    if (valid) {
        start = min(seg_start[j], n);
        end = max(min(seg_start[j + 1], n), start);
        sid = seg_sid[j];
    }
    const bool is_stream = valid && sid <= max_id;
    if (!is_stream) end = start;
    static_assert(SHORT >= 1, "a round walks at least one packet");
    AckState s{};
    if (is_stream) ack_load_state(s, snd + 8ull * sid);
    bool deferred = false;
    uint32_t dirty = 0, stop = end, mid = start;                  // mid: the lane's own part ends here
    uint64_t todo;
    do {
        const uint32_t lim = end - mid > SHORT ? mid + SHORT : end;
        for (; mid < lim; ++mid) {
            const uint32_t p = idx[mid];
            if (p >= n) continue;
            const uint4 rec = ack_step(s, win[mid], cur_ts, deferred);
            if (deferred) stop = min(stop, mid);
            else dirty |= ack_dirty(rec);
            ack[p] = rec;
        }
        todo = __ballot(mid < end);
    } while ((uint32_t)__popcll(todo) > WAVE_MAX);
    // what is left of the last few segments of these 64, one after the other,
    // as a whole wave: the state and every step are scalar
    while (todo) {
        const int l = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1;
        AckState u = ack_bcast_state(s, l);
        const uint32_t lstart = rcv_bcast(mid, l), lend = rcv_bcast(end, l);
        bool ldef = rcv_bcast(deferred, l) != 0;
        uint32_t ldirty = rcv_bcast(dirty, l), lstop = rcv_bcast(stop, l);
        for (uint32_t base = lstart; base < lend; base += kWave) {
            const uint32_t cnt = min((uint32_t)kWave, lend - base);
            uint4 mine = make_uint4(0u, 0u, 0u, 0u);
            uint32_t p = 0xFFFFFFFFu;
            if (lane < cnt) {
                mine = win[base + lane];
                p = idx[base + lane];
            }
            uint4 rec = make_uint4(0u, 0u, 0u, 0u);
            for (uint32_t k = 0; k < cnt; ++k) {
                const uint32_t pk = rcv_bcast(p, (int)k);
                const uint4 in = make_uint4(rcv_bcast(mine.x, (int)k), rcv_bcast(mine.y, (int)k),
                                            rcv_bcast(mine.z, (int)k), rcv_bcast(mine.w, (int)k));
                if (pk >= n) continue;                            // the same in every lane
                const uint4 r = ack_step(u, in, cur_ts, ldef);
                if (ldef) lstop = min(lstop, base + k);
                else ldirty |= ack_dirty(r);
                if (lane == k) rec = r;
            }
            if (p < n) ack[p] = rec;
        }
        if ((int)lane == l) {
            s = u;
            stop = lstop, dirty = ldirty;
        }
    }
    if (is_stream && dirty) ack_store_state(s, snd + 8ull * sid, dirty);
    if (valid) ack_stop[j] = stop;
}

}  // namespace mg
