// rtosweep_kernels.hpp — gfx950 kernels of the retransmission-timeout sweep over
// device send states: CheckRtmTimeout's firing decision for
// every stream of d_snd[max_id + 1], HandleRTO's ESTABLISHED path and the
// AddtoSendList it ends in for the first `cap` of them in ascending id
// (mtcp/src/timer.c:363-419, :176-337; mtcp/src/tcp_out.c:837-855).
// include/mtcp_gpu_rtosweep.h has the contract, rto_step.hpp the test and the
// step.
//
// A lane per stream, kRtoRounds streams a lane: a wave owns kRtoWaveChunk
// consecutive ids, a workgroup kRtoTile.  Of a 128 B record the test loads
// dword 21 (on_rto) and dword 10 (ts_rto), both at once: loading ts_rto only
// where on_rto is 1 puts a dependent load behind the first and measured slower
// wherever streams are on the RTO list.  The order is an
// ordered compaction, count / scan / emit as steer_kernels.hpp:
//
//   count  per wave and round one ballot of "due"; the wave's 16 ballots go to
//          the workspace (128 B, one store), their popcount to cnt[wave];
//   scan   steer_scan_kernel (steer_kernels.hpp), ONE workgroup: the exclusive
//          prefix of the wave counts in place, the total = due;
//   emit   per wave its ballots again (not the records: they change under the
//          emit of other lanes): a due stream's rank is the wave's prefix plus
//          the popcount of the ballots below it; a rank below cap loads the
//          stream's bytes 0-87 and its 16 B d_dtx record, runs rto_step and
//          stores what it says, its 16 B d_rto record and its d_seg_sid entry.
//          The grid also zeroes d_seg_start[0 .. cap] and d_seg_stop[0 .. cap)
//          and writes d_nseg and d_total.
//
// rto_one_kernel does all three in one workgroup for max_id + 1 <= kRtoTile: the
// ballots stay in registers, the four wave counts go through the block scan.
//
// No atomic decides an order, no workgroup waits on another, no LDS beyond the
// scan's, every loop's trip count is fixed by the tile or by cap, and every
// store is bounded by max_id, cap and min(due, cap) whatever the records or the
// workspace hold.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mtcp_gpu_rtosweep.h"
#include "rto_step.hpp"
#include "steer_kernels.hpp"     // steer_scan_kernel, block_exclusive_scan; kWave, kBlock, gload through rx_kernels.hpp
#include "txbuild_kernels.hpp"   // gsv4u, gload32, gload64

namespace mg {

constexpr int kRtoRounds = 16;                                    // streams per lane
constexpr uint32_t kRtoWaveChunk = kWave * kRtoRounds;            // 1 024 consecutive ids per wave
constexpr uint32_t kRtoTile = kBlock * kRtoRounds;                // 4 096 per workgroup

// The workspace: per wave its 16 ballots (128 B) and its count (4 B), the total.
struct RtoSweepWork {
    uint32_t ntiles, nwaves;
    uint64_t ballot_off, cnt_off, tot_off, bytes;
};
inline RtoSweepWork rto_sweep_work(uint32_t max_id) {
    RtoSweepWork w{};
    w.ntiles = (uint32_t)(((uint64_t)max_id + kRtoTile) / kRtoTile);
    w.nwaves = w.ntiles * kWavesPerBlock;
    w.ballot_off = 0;
    w.cnt_off = 8ull * kRtoRounds * w.nwaves;
    w.tot_off = w.cnt_off + ((4ull * w.nwaves + 15) & ~15ull);
    w.bytes = w.tot_off + 16;
    return w;
}

struct RtoSweepParams {
    uint32_t max_id, cap, cur_ts;
};

// "due" of the kRtoRounds streams of this lane, bit r for id base + r * kWave;
// an id above max_id is not due and is not read.
__device__ __forceinline__ uint32_t rto_lane_due(const uint8_t *__restrict__ snd, uint64_t base,
                                                 const RtoSweepParams &P) {
    uint32_t b2[kRtoRounds], ts[kRtoRounds];
#pragma unroll
    for (int r = 0; r < kRtoRounds; ++r) {
        const uint64_t id = base + (uint32_t)r * kWave;
        b2[r] = 0, ts[r] = 0;
        if (id <= P.max_id) {
            b2[r] = gload32((uint64_t)snd + 128ull * id + 84);
            ts[r] = gload32((uint64_t)snd + 128ull * id + 40);
        }
    }
    uint32_t due = 0;
#pragma unroll
    for (int r = 0; r < kRtoRounds; ++r) due |= rto_due(b2[r], ts[r], P.cur_ts) ? 1u << r : 0u;
    return due;
}

// One handled stream: HandleRTO and AddtoSendList for stream `id`, the rank-th
// handled one.  rank < cap and id <= max_id hold.
__device__ __forceinline__ void rto_handle(uint32_t id, uint32_t rank, uint8_t *__restrict__ snd,
                                           uint8_t *__restrict__ dtx, mtcp_gpu_rto_rec *__restrict__ rec,
                                           uint32_t *__restrict__ seg_sid) {
    const uint64_t sa = (uint64_t)snd + 128ull * id;
    const v4u q0 = gload(sa), q1 = gload(sa + 16), q2 = gload(sa + 32), q3 = gload(sa + 48), q4 = gload(sa + 64);
    const v2u q5 = gload64(sa + 80);                                // bytes 88-127 are the caller's: not read
    const v4u d = gload((uint64_t)dtx + 16ull * id);
    RtoIn s;
    s.snd_una = q0.y, s.peer_wnd = q0.w, s.cwnd = q1.w, s.rto = q2.y, s.srtt = q2.w, s.rttvar = q3.z;
    s.sb_len = q4.y, s.sb_size = q4.z, s.mss2 = q4.w, s.bits = q5.x, s.bits2 = q5.y, s.dflags = d.w;
    const RtoOut o = rto_step(s);
    uint32_t *srec = reinterpret_cast<uint32_t *>(snd + 128ull * id);
    if (o.st_win) srec[0] = o.snd_nxt, srec[7] = o.cwnd, srec[8] = o.ssthresh, srec[9] = o.rto;
    if (o.st_bits) srec[20] = o.bits, srec[21] = o.bits2;
    if (o.st_on) dtx[16ull * id + 12] = 1;
    const v4u rv = {id, o.rec[0], o.rec[1], o.rec[2]};
    *reinterpret_cast<gsv4u *>((uint64_t)rec + 16ull * rank) = rv;
    seg_sid[rank] = id;
}

// The emit of one wave: b(r) is round r's ballot, run the number of due streams
// below the wave.
template <typename B>
__device__ __forceinline__ void rto_wave_emit(B b, uint32_t run, uint64_t base, const RtoSweepParams &P,
                                              uint8_t *__restrict__ snd, uint8_t *__restrict__ dtx,
                                              mtcp_gpu_rto_rec *__restrict__ rec, uint32_t *__restrict__ seg_sid) {
    const uint32_t lane = threadIdx.x & (kWave - 1);
#pragma unroll
    for (int r = 0; r < kRtoRounds; ++r) {
        const uint64_t m = b(r);
        const uint32_t rank = run + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        const uint64_t id = base + (uint32_t)r * kWave;
        if (((m >> lane) & 1ull) && rank < P.cap && id <= P.max_id) rto_handle((uint32_t)id, rank, snd, dtx, rec, seg_sid);
        run += (uint32_t)__popcll(m);
    }
}

// The table's fixed part and the totals, by every lane of the grid: i = this
// lane's index in it, stride = its lanes.
__device__ __forceinline__ void rto_table(uint32_t i, uint32_t stride, uint32_t due, const RtoSweepParams &P,
                                          uint32_t *__restrict__ seg_start, uint32_t *__restrict__ seg_stop,
                                          uint32_t *__restrict__ nseg, uint64_t *__restrict__ total) {
    const uint32_t handled = due < P.cap ? due : P.cap;
    if (i == 0) nseg[0] = handled, total[0] = due, total[1] = handled;
    for (uint64_t k = i; k <= P.cap; k += stride) {
        seg_start[k] = 0;
        if (k < P.cap) seg_stop[k] = 0;
    }
}

// ---- count ------------------------------------------------------------------
// grid: one workgroup per tile.  ballots[16 * wave + r], cnt[wave].
__global__ __launch_bounds__(kBlock) void rto_count_kernel(const uint8_t *__restrict__ snd, const RtoSweepParams P,
                                                           uint64_t *__restrict__ ballots,
                                                           uint32_t *__restrict__ cnt) {
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
    const uint32_t due = rto_lane_due(snd, (uint64_t)wave * kRtoWaveChunk + lane, P);
    uint64_t mine = 0;
    uint32_t c = 0;
#pragma unroll
    for (int r = 0; r < kRtoRounds; ++r) {
        const uint64_t m = __ballot((due >> r) & 1u);
        c += (uint32_t)__popcll(m);
        if ((int)lane == r) mine = m;
    }
    if (lane < (uint32_t)kRtoRounds) ballots[(uint64_t)wave * kRtoRounds + lane] = mine;
    if (lane == 0) cnt[wave] = c;
}

// ---- emit -------------------------------------------------------------------
// grid: as count.  cnt: the scanned counts; tot[0]: due.
__global__ __launch_bounds__(kBlock) void rto_emit_kernel(const uint64_t *__restrict__ ballots,
                                                          const uint32_t *__restrict__ cnt,
                                                          const uint32_t *__restrict__ tot, const RtoSweepParams P,
                                                          uint8_t *__restrict__ snd, uint8_t *__restrict__ dtx,
                                                          mtcp_gpu_rto_rec *__restrict__ rec,
                                                          uint32_t *__restrict__ seg_sid,
                                                          uint32_t *__restrict__ seg_start,
                                                          uint32_t *__restrict__ seg_stop, uint32_t *__restrict__ nseg,
                                                          uint64_t *__restrict__ total) {
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
    const uint32_t run = cnt[wave];
    if (run < P.cap) {                                              // the same in every lane of the wave
        const uint64_t *wb = ballots + (uint64_t)wave * kRtoRounds;
        rto_wave_emit([&](int r) { return wb[r]; }, run, (uint64_t)wave * kRtoWaveChunk + lane, P, snd, dtx, rec,
                      seg_sid);
    }
    rto_table(blockIdx.x * kBlock + threadIdx.x, gridDim.x * kBlock, tot[0], P, seg_start, seg_stop, nseg, total);
}

// ---- max_id + 1 <= kRtoTile: everything in one workgroup -----------------------
__global__ __launch_bounds__(kBlock) void rto_one_kernel(const RtoSweepParams P, uint8_t *__restrict__ snd,
                                                         uint8_t *__restrict__ dtx,
                                                         mtcp_gpu_rto_rec *__restrict__ rec,
                                                         uint32_t *__restrict__ seg_sid,
                                                         uint32_t *__restrict__ seg_start,
                                                         uint32_t *__restrict__ seg_stop, uint32_t *__restrict__ nseg,
                                                         uint64_t *__restrict__ total) {
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const uint64_t base = (uint64_t)wave * kRtoWaveChunk + lane;
    const uint32_t due = rto_lane_due(snd, base, P);
    uint64_t m[kRtoRounds];
    uint32_t c = 0;
#pragma unroll
    for (int r = 0; r < kRtoRounds; ++r) {
        m[r] = __ballot((due >> r) & 1u);
        c += (uint32_t)__popcll(m[r]);
    }
    uint32_t excl;
    const uint32_t all = block_exclusive_scan(lane == 0 ? c : 0u, excl);
    const uint32_t run = __shfl(excl, 0, kWave);                   // lane 0's: the waves below this one
    rto_wave_emit([&](int r) { return m[r]; }, run, base, P, snd, dtx, rec, seg_sid);
    rto_table(threadIdx.x, kBlock, all, P, seg_start, seg_stop, nseg, total);
}

}  // namespace mg
