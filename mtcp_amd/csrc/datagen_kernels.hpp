// datagen_kernels.hpp — gfx950 kernels that turn a walked rx batch into send
// bursts for row f8 and commit what the flush leaves behind (SURVEY §8 row
// f15): WriteTCPDataList's body and the head of FlushTCPSendingBuffer
// (mtcp/src/tcp_out.c:607-660, :357-449) for every stream of a grouped batch.
// include/mtcp_gpu_datagen.h has the contract, datagen_step.hpp the fold, the
// status, the burst and the commit.
//
// Two launches around row f8's own, ordered by the stream:
//
//   burst   one lane per index j < n, 64 consecutive segments a wave.  For a
//           segment of the group's table: the stream's 16 B d_dtx record, its
//           32 B tx record, the first 32 B of its receive state and four 16 B
//           pieces and 8 B of its send state; the fold of the ACK walk's
//           FAST_RTX / SEND_LIST_REMOVE flags over the walked part of the list,
//           one flag dword per packet gathered through d_idx.  A list of at
//           most kDatagenLaneMax packets is its lane's own loop; a longer one
//           is taken by the whole wave afterwards, 64 flag dwords loaded at
//           once, the two flags as two ballots, the highest set position
//           deciding.  The status, parked in one dword; the 64 B burst as four
//           16 B stores.  Every other index gets the void burst.
//   (mtcp_gpu_tx_segment_dev over the n bursts: plan, scan, place, emit, or its
//    one-workgroup form)
//   commit  one lane per segment: the parked status, row f8's 16 B result, the
//           stream's own dwords; snd_nxt, ts_rto, on_rto, ip_id, ack_cnt,
//           is_wack, need_wnd_adv, ts_lastack_sent and on_send_list as
//           datagen_commit says; the 16 B result.
//
// The burst kernel writes nothing but the workspace, so what the commit reads
// of a record is what the call was given.  No workgroup waits on another, no
// atomic, every loop's trip count is fixed by the segment table clamped to n,
// and every store is bounded by n, min(d_nseg[0], n) and max_id whatever the
// inputs or the workspace hold.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mtcp_gpu_datagen.h"
#include "datagen_step.hpp"
#include "rcvwalk_kernels.hpp"   // rcv_bcast; kWave, kBlock, gload through rx_kernels.hpp
#include "txbuild_kernels.hpp"   // gsv4u, gload32, gload64

namespace mg {

// The longest list a lane folds by itself: row f14's measured threshold (DESIGN
// §8 f14), inherited; this fold gathers the same one dword per packet.
constexpr uint32_t kDatagenLaneMax = 64;

// The workspace: the n bursts (64 B each), row f8's n results (16 B), the n
// parked statuses (4 B, padded to 16 B), row f8's own workspace.
struct DataGenWork {
    uint64_t burst_off, res_off, park_off, f8_off;
};
inline DataGenWork datagen_work(uint32_t n) {
    DataGenWork w{};
    w.burst_off = 0;
    w.res_off = 64ull * n;
    w.park_off = w.res_off + 16ull * n;
    w.f8_off = (w.park_off + 4ull * n + 15) & ~15ull;
    return w;
}

struct DataGenParams {
    uint32_t n, max_id, n_links, cur_ts;
};

// ---- burst ----------------------------------------------------------------------
// grid: one workgroup per kBlock indices, for n.  ack: 16 B records or NULL
// (with ack_stop); state: 64 B; snd: 128 B; tx: 32 B; dtx: 16 B.  burst[j] for
// j < n, park[j] for j < m.
template <uint32_t LANE_MAX>
__global__ __launch_bounds__(kBlock) void datagen_burst_kernel(
    const uint8_t *__restrict__ ack, const uint32_t *__restrict__ idx, const DataGenParams P,
    const uint32_t *__restrict__ seg_sid, const uint32_t *__restrict__ seg_start, const uint32_t *__restrict__ nseg,
    const uint32_t *__restrict__ seg_stop, const uint32_t *__restrict__ ack_stop, const uint8_t *__restrict__ state,
    const uint8_t *__restrict__ snd, const uint8_t *__restrict__ tx, const uint8_t *__restrict__ dtx,
    uint8_t *__restrict__ burst, uint32_t *__restrict__ park) {
    const uint32_t n = P.n, m = min(nseg[0], n);
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    const bool valid = j < m;
    uint32_t start = 0, end = 0, sid = 0xFFFFFFFFu;
    if (valid) {
        start = min(seg_start[j], n);
        end = max(min(seg_start[j + 1], n), start);
        sid = seg_sid[j];
    }
    const bool is_stream = valid && sid <= P.max_id;
    DataGenIn s{};
    uint32_t stopc = start;
    bool bad = false, host_tail = false;
    if (is_stream) {
        const v4u d = gload((uint64_t)dtx + 16ull * sid);
        s.sb_off = ((uint64_t)d.y << 32) | d.x, s.sb_base_seq = d.z, s.dflags = d.w;
        const v4u a = gload((uint64_t)tx + 32ull * sid), b = gload((uint64_t)tx + 32ull * sid + 16);
        s.tx.saddr = a.x, s.tx.daddr = a.y, s.tx.ports = a.z, s.tx.id_cnt = a.w;
        s.tx.misc = b.x, s.tx.ts_lastack_sent = b.y, s.tx.rsvd0 = b.z, s.tx.rsvd1 = b.w;
        const v4u r0 = gload((uint64_t)state + 64ull * sid);        // rcv_nxt, rcv_wnd, head_seq, merged_len
        const v4u r1 = gload((uint64_t)state + 64ull * sid + 16);   // size, ts_recent, ts_lastack_rcvd, tcp_state | ...
        s.rcv_nxt = r0.x, s.rcv_wnd = r0.y, s.ts_recent = r1.y, s.rstate = r1.w;
        const uint64_t sa = (uint64_t)snd + 128ull * sid;
        const v4u q0 = gload(sa), q1 = gload(sa + 16), q4 = gload(sa + 64);
        const v2u q5 = gload64(sa + 80);                            // bytes 88-127 are the caller's: not read
        s.snd_nxt = q0.x, s.snd_una = q0.y, s.peer_wnd = q0.w, s.cwnd = q1.w;
        s.sb_head_seq = q4.x, s.sb_len = q4.y, s.sb_size = q4.z, s.mss2 = q4.w;
        s.bits = q5.x, s.bits2 = q5.y;
        bad = datagen_bad(s, P.n_links);
        host_tail = seg_stop[j] < end;
        if (ack_stop) {
            const uint32_t as = ack_stop[j];
            host_tail = host_tail || as < end;
            if (!bad && ack) stopc = min(max(as, start), end);
        }
    }
    const uint32_t on_before = s.dflags & 1u;
    uint32_t on = on_before;
    const bool lng = stopc - start > LANE_MAX;
    if (!lng) {
        for (uint32_t p = start; p < stopc; ++p) {
            const uint32_t q = idx[p];
            if (q >= n) continue;
            on = datagen_fold(on, gload32((uint64_t)ack + 16ull * q + 12));
        }
    }
    // the long lists of these 64 segments, one after the other, as a whole wave
    uint64_t todo = __ballot(lng);
    while (todo) {
        const int l = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1;
        const uint32_t lstart = rcv_bcast(start, l), lend = rcv_bcast(stopc, l);
        uint32_t lon = rcv_bcast(on, l);
        for (uint32_t base = lstart; base < lend; base += kWave) {
            uint32_t w = 0;
            if (lane < lend - base) {
                const uint32_t q = idx[base + lane];
                if (q < n) w = gload32((uint64_t)ack + 16ull * q + 12);
            }
            lon = datagen_fold_masks(lon, __ballot(w & MTCP_GPU_ACK_FAST_RTX), __ballot(w & MTCP_GPU_ACK_SEND_LIST_REMOVE));
        }
        if ((int)lane == l) on = lon;
    }
    uint32_t w[16];
    uint32_t status = MTCP_GPU_DATAGEN_NONE;
    if (is_stream) status = datagen_status(s, P.n_links, on, host_tail);
    if (status == MTCP_GPU_DATAGEN_SENT) datagen_burst(s, P.cur_ts, w);
    else datagen_burst_void(w);
    if (j < n) {
        const uint64_t at = (uint64_t)burst + 64ull * j;
        const v4u b0 = {w[0], w[1], w[2], w[3]}, b1 = {w[4], w[5], w[6], w[7]};
        const v4u b2 = {w[8], w[9], w[10], w[11]}, b3 = {w[12], w[13], w[14], w[15]};
        *reinterpret_cast<gsv4u *>(at) = b0;
        *reinterpret_cast<gsv4u *>(at + 16) = b1;
        *reinterpret_cast<gsv4u *>(at + 32) = b2;
        *reinterpret_cast<gsv4u *>(at + 48) = b3;
    }
    if (valid) {
        const bool win0 = status > MTCP_GPU_DATAGEN_BAD && datagen_window32(s) == 0;
        park[j] = datagen_park(status, status > MTCP_GPU_DATAGEN_BAD ? on_before : 0u, on, win0);
    }
}

// ---- commit -----------------------------------------------------------------------
// grid: one lane per segment, for n.  f8res: row f8's results of the n bursts.
__global__ __launch_bounds__(kBlock) void datagen_commit_kernel(
    const uint32_t *__restrict__ park, const uint8_t *__restrict__ f8res, const DataGenParams P,
    const uint32_t *__restrict__ seg_sid, const uint32_t *__restrict__ nseg, uint8_t *__restrict__ snd,
    uint8_t *__restrict__ tx, uint8_t *__restrict__ dtx, mtcp_gpu_datagen_res *__restrict__ dres) {
    const uint32_t m = min(nseg[0], P.n);
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= m) return;
    const uint32_t sid = seg_sid[k];
    uint32_t pk = park[k];
    if (sid > P.max_id) pk = MTCP_GPU_DATAGEN_NONE;                  // holds already: the burst kernel said so
    const v4u r = gload((uint64_t)f8res + 16ull * k);
    const uint32_t f8[4] = {r.x, r.y, r.z, r.w};
    uint32_t snd_nxt = 0, rto = 0, bits2 = 0, id_cnt = 0, misc = 0, ts_last = 0;
    const bool live = (pk & 0xFFu) > MTCP_GPU_DATAGEN_BAD;
    const uint64_t sa = (uint64_t)snd + 128ull * sid, ta = (uint64_t)tx + 32ull * sid;
    if (live) {
        snd_nxt = gload32(sa), rto = gload32(sa + 36), bits2 = gload32(sa + 84);
        id_cnt = gload32(ta + 12), misc = gload32(ta + 16), ts_last = gload32(ta + 20);
    }
    const DataGenCommit c = datagen_commit(pk, f8, snd_nxt, rto, bits2, id_cnt, misc, ts_last, P.cur_ts);
    if (live) {
        uint32_t *srec = reinterpret_cast<uint32_t *>(snd + 128ull * sid);
        uint32_t *trec = reinterpret_cast<uint32_t *>(tx + 32ull * sid);
        if (c.st_snd_nxt) srec[0] = c.snd_nxt;
        if (c.st_rto) srec[10] = c.ts_rto, snd[128ull * sid + 85] = 1;
        if (c.st_id_cnt) trec[3] = c.id_cnt;
        if (c.st_misc) trec[4] = c.misc;
        if (c.st_ts) trec[5] = c.ts_lastack_sent;
        if (c.st_on) dtx[16ull * sid + 12] = (uint8_t)c.on_send_list;
    }
    const v4u rv = {c.res[0], c.res[1], c.res[2], c.res[3]};
    *reinterpret_cast<gsv4u *>((uint64_t)dres + 16ull * k) = rv;
}

}  // namespace mg
