// rcvwalk_kernels.hpp — gfx950 kernels of the per-stream receive walk (SURVEY
// §8 row f11): ValidateSequence (mtcp/src/tcp_in.c:101-179), the payload branch
// of Handle_TCP_ST_ESTABLISHED (tcp_in.c:854-862), ProcessTCPPayload
// (tcp_in.c:537-610) and the bookkeeping of RBPut
// (mtcp/src/tcp_ring_buffer.c:280-382) for every stream of a grouped batch.
// include/mtcp_gpu_rcvwalk.h has the contract.
//
// Two launches, ordered by the stream:
//
//   gather  one lane per position j of d_idx: the 16 B walk input of packet
//           d_idx[j] (seq, ts_val, ts_ref, payload_len | tcp_flags | option
//           flags) to position j of the workspace, so that a walker reads a
//           list as one contiguous run; and d_place[j] = 0, so that every
//           placement record is written whatever the lists hold;
//   walk    one lane per segment of the group's table, 64 consecutive segments
//           a wave.  The lanes walk their own segments in rounds of
//           kRcvShortLen packets while more than kRcvWaveMax of them have
//           packets left.  The wave then takes what is left (of at most
//           kRcvWaveMax segments) one segment after the other as a whole wave:
//           64 inputs loaded coalesced, stepped through with the state in
//           scalar registers, lane k keeping the placement record of step k,
//           64 records stored at once.  A step of the wave form takes about a
//           third of a lane's step (no dependent load, no divergence between
//           lanes), so it pays for the last few segments only.  The walker
//           scatters the records to packet order itself.
//
// rcv_step is the walk of one packet; both forms run the same code.  The four
// fragment slots live in registers: every index into them is a constant after
// unrolling, the runtime positions (the insert, the compaction) are compare
// chains.  No workgroup waits on another, no atomic, no LDS; every loop's trip
// count is fixed by the segment table clamped to n; every store is bounded by
// n, max_id and min(d_nseg[0], n).  A long list is serial by nature: a batch
// with one heavy stream runs as long as that stream's walk.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mtcp_gpu.h"
#include "../../include/mtcp_gpu_rcvwalk.h"
#include "rx_kernels.hpp"        // kWave, kBlock, kWavesPerBlock

namespace mg {

constexpr uint32_t kRcvShortLen = 32;    // packets a lane walks per round (DESIGN §8 f11 has the measurement)
constexpr uint32_t kRcvWaveMax = 3;      // the wave form takes over when at most this many lanes have packets left

struct RcvWork {
    uint64_t in_off, bytes;
};
inline RcvWork rcv_work(uint32_t n) {
    RcvWork w{};
    w.in_off = 0;
    w.bytes = n ? 16ull * n : 16ull;
    return w;
}

// ---- the reference's comparisons ----------------------------------------------
// TCP_SEQ_* (tcp_in.h:37-41)
__host__ __device__ __forceinline__ bool rcv_seq_lt(uint32_t a, uint32_t b) { return (int32_t)(a - b) < 0; }
__host__ __device__ __forceinline__ bool rcv_seq_leq(uint32_t a, uint32_t b) { return (int32_t)(a - b) <= 0; }
__host__ __device__ __forceinline__ bool rcv_seq_gt(uint32_t a, uint32_t b) { return (int32_t)(a - b) > 0; }
__host__ __device__ __forceinline__ bool rcv_seq_geq(uint32_t a, uint32_t b) { return (int32_t)(a - b) >= 0; }
// GetMinSeq / GetMaxSeq (tcp_ring_buffer.c:234-254), MAXSEQ/2 = 0x7FFFFFFF
__host__ __device__ __forceinline__ uint32_t rcv_min_seq(uint32_t a, uint32_t b) {
    if (a == b) return a;
    if (a < b) return (b - a) <= 0x7FFFFFFFu ? a : b;
    return (a - b) <= 0x7FFFFFFFu ? b : a;
}
__host__ __device__ __forceinline__ uint32_t rcv_max_seq(uint32_t a, uint32_t b) {
    if (a == b) return a;
    if (a < b) return (b - a) <= 0x7FFFFFFFu ? b : a;
    return (a - b) <= 0x7FFFFFFFu ? a : b;
}

// One mtcp_gpu_rcv_state in registers.  bits: tcp_state | saw_timestamp << 8 |
// nfrag << 16 | rsvd << 24 (the record's bytes 28..31).
struct RcvState {
    uint32_t rcv_nxt, rcv_wnd, head_seq, merged_len, size, ts_recent, ts_lastack, bits;
    uint32_t fs[MTCP_GPU_RCV_MAX_FRAGS], fl[MTCP_GPU_RCV_MAX_FRAGS];
};

// A placement record as one 16 B piece: w = put_len | verdict << 16 | flags << 24.
__host__ __device__ __forceinline__ uint4 rcv_place(uint32_t put_off, uint32_t rcv_nxt, uint32_t rcv_wnd,
                                                    uint32_t put_len, uint32_t verdict, uint32_t flags) {
    return uint4{put_off, rcv_nxt, rcv_wnd, put_len | verdict << 16 | flags << 24};
}

// The walk of one packet.  in: seq, ts_val, ts_ref, payload_len | tcp_flags <<
// 16 | option flags << 24.  `deferred`: an earlier packet of this stream in
// this batch was deferred; set when this one is.  Nothing of s changes then.
__host__ __device__ __forceinline__ uint4 rcv_step(RcvState &s, const uint4 in, const bool has_opt, bool &deferred) {
    constexpr int F = MTCP_GPU_RCV_MAX_FRAGS;
    const uint32_t seq = in.x, ts_val = in.y, ts_ref = in.z;
    const uint32_t len = in.w & 0xFFFFu, tcp_flags = (in.w >> 16) & 0xFFu, opt_flags = in.w >> 24;
    if (deferred) return rcv_place(0, 0, 0, 0, MTCP_GPU_RCV_DEFER_BEHIND, 0);
    uint32_t nf = (s.bits >> 16) & 0xFFu;
    const bool saw_ts = ((s.bits >> 8) & 0xFFu) != 0;
    bool bad = (s.bits >> 24) != 0 || nf > (uint32_t)F || s.size > MTCP_GPU_RCV_MAX_SIZE || s.merged_len > s.size;
#pragma unroll
    for (int k = 0; k < F; ++k) bad |= (uint32_t)k < nf && (s.fl[k] >> 31) != 0;
    uint32_t dv = 0;
    if (bad) dv = MTCP_GPU_RCV_DEFER_BAD_STATE;
    else if ((s.bits & 0xFFu) != MTCP_GPU_RCV_ST_ESTABLISHED) dv = MTCP_GPU_RCV_DEFER_STATE;
    else if (tcp_flags & 0x07u) dv = MTCP_GPU_RCV_DEFER_FLAGS;                  // FIN, SYN, RST
    else if (saw_ts && (!has_opt || (opt_flags & MTCP_GPU_TCPOPT_TS_UNPINNED))) dv = MTCP_GPU_RCV_DEFER_TS;
    if (dv) {
        deferred = true;
        return rcv_place(0, 0, 0, 0, dv, 0);
    }

    // ValidateSequence, tcp_in.c:101-179 (tcph->rst is clear here)
    uint32_t flags = 0, ts_recent = s.ts_recent, ts_lastack = s.ts_lastack;
    if (saw_ts) {
        if (!(opt_flags & MTCP_GPU_TCPOPT_TS_FOUND))                            // :109-115
            return rcv_place(0, s.rcv_nxt, s.rcv_wnd, 0, MTCP_GPU_RCV_PAWS_NO_TS, 0);
        if (rcv_seq_lt(ts_val, ts_recent))                                      // :119-126
            return rcv_place(0, s.rcv_nxt, s.rcv_wnd, 0, MTCP_GPU_RCV_PAWS_OLD, MTCP_GPU_RCV_ACK_NOW);
        if (rcv_seq_gt(ts_val, ts_recent)) flags |= MTCP_GPU_RCV_TS_NEWER;      // :129-135
        ts_recent = ts_val;                                                     // :137-138
        ts_lastack = ts_ref;
    }
    const uint32_t seg_end = seq + len;
    if (!(rcv_seq_geq(seg_end, s.rcv_nxt) && rcv_seq_leq(seg_end, s.rcv_nxt + s.rcv_wnd))) {   // :143-144
        s.ts_recent = ts_recent, s.ts_lastack = ts_lastack;
        if (seq + 1 == s.rcv_nxt)                                               // :152-158
            return rcv_place(0, s.rcv_nxt, s.rcv_wnd, 0, MTCP_GPU_RCV_SEQ_WINPROBE, flags | MTCP_GPU_RCV_ACK_AGGREGATE);
        if (rcv_seq_leq(seq, s.rcv_nxt))                                        // :162-163
            return rcv_place(0, s.rcv_nxt, s.rcv_wnd, 0, MTCP_GPU_RCV_SEQ_OLD, flags | MTCP_GPU_RCV_ACK_AGGREGATE);
        return rcv_place(0, s.rcv_nxt, s.rcv_wnd, 0, MTCP_GPU_RCV_SEQ_AHEAD, flags | MTCP_GPU_RCV_ACK_NOW);   // :164-165
    }
    if (len == 0) {                                                             // tcp_in.c:854 not taken
        s.ts_recent = ts_recent, s.ts_lastack = ts_lastack;
        return rcv_place(0, s.rcv_nxt, s.rcv_wnd, 0, MTCP_GPU_RCV_ACK_ONLY, flags);
    }

    // ProcessTCPPayload, tcp_in.c:537-610 (:546 and :550 repeat the test above); RBPut, tcp_ring_buffer.c:280-382
    uint32_t verdict, put_off = 0, put_len = 0, merged_len = s.merged_len;
    uint32_t fs[F], fl[F];
#pragma unroll
    for (int k = 0; k < F; ++k) fs[k] = s.fs[k], fl[k] = s.fl[k];
    if (rcv_min_seq(s.head_seq, seq) != s.head_seq) {                           // :294
        verdict = MTCP_GPU_RCV_PUT_DROPPED;
    } else if ((uint64_t)s.size < (uint64_t)(seq - s.head_seq) + len) {         // :297-301
        verdict = MTCP_GPU_RCV_PUT_NO_ROOM;
    } else {
        verdict = MTCP_GPU_RCV_PUT_STORED;
        put_off = seq - s.head_seq, put_len = len, flags |= MTCP_GPU_RCV_COPY;
        // the traversal, :332-358: new_ctx is (cs, cl); b: the index of iter when the loop ends
        uint32_t cs = seq, cl = len, del = 0, b = nf;
        bool merged = false, stop = false;
#pragma unroll
        for (int i = 0; i < F; ++i) {
            if ((uint32_t)i < nf && !stop) {
                const uint32_t a_end = cs + cl + 1, b_end = fs[i] + fl[i] + 1;  // CanMerge, :259-265
                if (!(rcv_min_seq(a_end, fs[i]) == a_end || rcv_min_seq(b_end, cs) == b_end)) {
                    const uint32_t mn = rcv_min_seq(cs, fs[i]);                 // MergeFragments, :269-278
                    const uint32_t mx = rcv_max_seq(cs + cl, fs[i] + fl[i]);
                    fs[i] = mn, fl[i] = (mx - mn) & 0x7FFFFFFFu;
                    if (i > 0 && merged) del |= 1u << (i - 1);                  // prev == new_ctx, :341-347
                    cs = fs[i], cl = fl[i], merged = true;
                } else if (merged || rcv_max_seq(seq + len, fs[i]) == fs[i]) {  // :352-357
                    stop = true, b = (uint32_t)i;
                }
            }
        }
        if (!merged) {                                                          // :360-375
            uint32_t pos = 0;
            if (nf != 0 && rcv_min_seq(seq, fs[0]) != seq) pos = b;
            if (nf == (uint32_t)F || (nf != 0 && rcv_min_seq(seq, fs[0]) != seq && b == 0)) {
                deferred = true;                                                // a fifth fragment; prev == NULL at :370-372
                return rcv_place(0, 0, 0, 0, nf == (uint32_t)F ? MTCP_GPU_RCV_DEFER_FRAG_FULL : MTCP_GPU_RCV_DEFER_BAD_STATE, 0);
            }
#pragma unroll
            for (int k = F - 1; k > 0; --k)
                if ((uint32_t)k > pos) fs[k] = fs[k - 1], fl[k] = fl[k - 1];
#pragma unroll
            for (int k = 0; k < F; ++k)
                if ((uint32_t)k == pos) fs[k] = seq, fl[k] = len;
            nf += 1;
        } else if (del) {                                                       // the fragments merged away leave the list
            uint32_t os[F], ol[F], cnt = 0;
#pragma unroll
            for (int k = 0; k < F; ++k) os[k] = ol[k] = 0;
#pragma unroll
            for (int i = 0; i < F; ++i) {
                if ((uint32_t)i < nf && !((del >> i) & 1u)) {
#pragma unroll
                    for (int k = 0; k < F; ++k)
                        if (cnt == (uint32_t)k) os[k] = fs[i], ol[k] = fl[i];
                    cnt += 1;
                }
            }
#pragma unroll
            for (int k = 0; k < F; ++k) fs[k] = os[k], fl[k] = ol[k];
            nf = cnt;
        }
#pragma unroll
        for (int k = 0; k < F; ++k)
            if ((uint32_t)k >= nf) fs[k] = fl[k] = 0;
        if (s.head_seq == fs[0]) merged_len = fl[0];                            // :376-379
    }
    // commit; tcp_in.c:588-593
    s.ts_recent = ts_recent, s.ts_lastack = ts_lastack;
    if (verdict == MTCP_GPU_RCV_PUT_STORED) {
#pragma unroll
        for (int k = 0; k < F; ++k) s.fs[k] = fs[k], s.fl[k] = fl[k];
        s.bits = (s.bits & 0xFF00FFFFu) | nf << 16;
        s.merged_len = merged_len;
    }
    const uint32_t prev_rcv_nxt = s.rcv_nxt;
    s.rcv_nxt = s.head_seq + s.merged_len;
    s.rcv_wnd = s.size - s.merged_len;
    flags |= rcv_seq_leq(s.rcv_nxt, prev_rcv_nxt) ? MTCP_GPU_RCV_ACK_NOW
                                                  : MTCP_GPU_RCV_READ_EVENT | MTCP_GPU_RCV_ACK_AGGREGATE;
    return rcv_place(put_off, s.rcv_nxt, s.rcv_wnd, put_len, verdict, flags);
}

// ---- gather -------------------------------------------------------------------
// grid: one lane per position.  res: 40 B records; opt: 16 B records or NULL.
__global__ __launch_bounds__(kBlock) void rcvwalk_gather_kernel(const uint8_t *__restrict__ res,
                                                                const uint4 *__restrict__ opt,
                                                                const uint32_t *__restrict__ idx, uint32_t n,
                                                                uint4 *__restrict__ win, uint4 *__restrict__ place) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    const uint32_t p = idx[j];
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (p < n) {
        const uint32_t *r = reinterpret_cast<const uint32_t *>(res + 40ull * p);
        const uint32_t w8 = r[8];                                 // payload_len | ihl_doff << 16 | tcp_flags << 24
        v.x = r[3];                                               // seq
        v.w = (w8 & 0xFFFFu) | (w8 >> 24) << 16;
        if (opt) {
            const uint4 o = opt[p];
            v.y = o.x, v.z = o.y, v.w |= (o.w >> 24) << 24;
        }
    }
    win[j] = v;
    place[j] = make_uint4(0u, 0u, 0u, 0u);
}

// ---- walk ---------------------------------------------------------------------
__device__ __forceinline__ void rcv_load_state(RcvState &s, const uint4 *__restrict__ rec) {
    const uint4 a = rec[0], b = rec[1], c = rec[2], d = rec[3];
    s.rcv_nxt = a.x, s.rcv_wnd = a.y, s.head_seq = a.z, s.merged_len = a.w;
    s.size = b.x, s.ts_recent = b.y, s.ts_lastack = b.z, s.bits = b.w;
    s.fs[0] = c.x, s.fl[0] = c.y, s.fs[1] = c.z, s.fl[1] = c.w;
    s.fs[2] = d.x, s.fl[2] = d.y, s.fs[3] = d.z, s.fl[3] = d.w;
}
__device__ __forceinline__ void rcv_store_state(const RcvState &s, uint4 *__restrict__ rec) {
    rec[0] = make_uint4(s.rcv_nxt, s.rcv_wnd, s.head_seq, s.merged_len);
    rec[1] = make_uint4(s.size, s.ts_recent, s.ts_lastack, s.bits);
    rec[2] = make_uint4(s.fs[0], s.fl[0], s.fs[1], s.fl[1]);
    rec[3] = make_uint4(s.fs[2], s.fl[2], s.fs[3], s.fl[3]);
}
// Lane `lane`'s value in every lane, as a scalar: lane is the same in every
// lane (a ballot's first set bit, a loop counter), so what is computed from the
// result is scalar code.
__device__ __forceinline__ uint32_t rcv_bcast(uint32_t v, int lane) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, lane);
}

// grid: one lane per segment, for n segments (m is known only on the device;
// a wave whose first segment is at or past m ends at once).  SHORT: the
// packets a lane walks per round; WAVE_MAX: the lanes' rounds go on while more
// lanes than this have packets left.
template <uint32_t SHORT, uint32_t WAVE_MAX>
__global__ __launch_bounds__(kBlock) void rcvwalk_walk_kernel(const uint4 *__restrict__ win,
                                                              const uint32_t *__restrict__ idx, uint32_t n,
                                                              uint32_t max_id, const uint32_t *__restrict__ seg_sid,
                                                              const uint32_t *__restrict__ seg_start,
                                                              const uint32_t *__restrict__ nseg, uint32_t has_opt,
                                                              uint4 *__restrict__ state, uint4 *__restrict__ place,
                                                              uint32_t *__restrict__ seg_stop) {
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
    RcvState s{};
    if (is_stream) rcv_load_state(s, state + 4ull * sid);
    bool deferred = false, dirty = false;
    uint32_t stop = end, mid = start;                             // mid: the lane's own part ends here
    uint64_t todo;
    do {
        const uint32_t lim = end - mid > SHORT ? mid + SHORT : end;
        for (; mid < lim; ++mid) {
            const uint32_t p = idx[mid];
            if (p >= n) continue;
            const uint4 rec = rcv_step(s, win[mid], has_opt != 0, deferred);
            if (deferred) stop = min(stop, mid);
            else dirty = true;
            place[p] = rec;
        }
        todo = __ballot(mid < end);
    } while ((uint32_t)__popcll(todo) > WAVE_MAX);
    // what is left of the last few segments of these 64, one after the other,
    // as a whole wave: the state and every step are scalar
    while (todo) {
        const int l = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1;
        RcvState u;
        u.rcv_nxt = rcv_bcast(s.rcv_nxt, l), u.rcv_wnd = rcv_bcast(s.rcv_wnd, l);
        u.head_seq = rcv_bcast(s.head_seq, l), u.merged_len = rcv_bcast(s.merged_len, l);
        u.size = rcv_bcast(s.size, l), u.ts_recent = rcv_bcast(s.ts_recent, l);
        u.ts_lastack = rcv_bcast(s.ts_lastack, l), u.bits = rcv_bcast(s.bits, l);
#pragma unroll
        for (int k = 0; k < MTCP_GPU_RCV_MAX_FRAGS; ++k) u.fs[k] = rcv_bcast(s.fs[k], l), u.fl[k] = rcv_bcast(s.fl[k], l);
        const uint32_t lstart = rcv_bcast(mid, l), lend = rcv_bcast(end, l);
        bool ldef = rcv_bcast(deferred, l) != 0, ldirty = rcv_bcast(dirty, l) != 0;
        uint32_t lstop = rcv_bcast(stop, l);
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
                const uint4 r = rcv_step(u, in, has_opt != 0, ldef);
                if (ldef) lstop = min(lstop, base + k);
                else ldirty = true;
                if (lane == k) rec = r;
            }
            if (p < n) place[p] = rec;
        }
        if ((int)lane == l) {
            s = u;
            stop = lstop, dirty = ldirty;
        }
    }
    if (is_stream && dirty) rcv_store_state(s, state + 4ull * sid);
    if (valid) seg_stop[j] = stop;
}

}  // namespace mg
