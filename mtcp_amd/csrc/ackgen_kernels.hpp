// ackgen_kernels.hpp — gfx950 kernels that turn a walked rx batch into pure-ACK
// tx segment records: EnqueueACK's count, WriteTCPACKList
// and SendTCPPacket's record (mtcp/src/tcp_out.c:911-935, :697-761, :220-354)
// for every stream of a grouped batch.  include/mtcp_gpu_ackgen.h has the
// contract, ackgen_step.hpp the fold, the plan, the record and the commit.
//
// A stream's fan-out is 0 to 64 records, so this is count, scan and emit,
// three launches ordered by the stream:
//
//   plan   one lane per segment of the group's table, 64 consecutive segments
//          a wave: the 32 B tx record and the first 32 B of the receive state
//          as 16 B loads, the one dword snd_nxt; the fold over the walked part
//          of the list, one placement dword per packet gathered through d_idx.
//          A list of at most kAckgenLaneMax packets is its lane's own loop; a
//          longer one is taken by the whole wave afterwards, 64 placement
//          dwords loaded at once, their flags as three ballots, the fold over
//          the masks scalar (ackgen_fold_masks: exact, and O(1) for a chunk in
//          which no wrap to 0 can meet an AGGREGATE).  The plan, parked in
//          32 B; the exclusive prefix of the planned counts within the
//          workgroup; each workgroup's sum.
//   scan   txseg_scan_kernel (txseg_kernels.hpp), ONE workgroup: the exclusive
//          prefix of those sums and their total.
//   emit   one lane per OUTPUT record k < seg_cap: the workgroup of its
//          segment is searched in the scanned sums, the segment in that
//          workgroup's prefixes; three 16 B stores and the 8 B descriptor,
//          consecutive lanes consecutive records; records at and past the
//          total are void.  In the same grid one lane per segment applies the
//          room rule (closed form: every slot has one size, so the records
//          with room are the first E of the call), commits dwords 3-5 of the
//          stream's tx record and writes its result; d_total.
//
// The emit reads only the parked plans, so the commit's stores to d_tx race
// with nothing.  The counts saturate at seg_cap, as in txseg_kernels.hpp: a
// saturated prefix is past every room test.  No workgroup waits on another, no
// atomic, every loop's trip count is fixed by the segment table clamped to n,
// and every store is bounded by min(d_nseg[0], n), max_id and seg_cap whatever
// the inputs or the workspace hold.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mtcp_gpu_ackgen.h"
#include "ackgen_step.hpp"
#include "rcvwalk_kernels.hpp"   // rcv_bcast; kWave, kBlock, gload through rx_kernels.hpp
#include "txseg_kernels.hpp"     // txseg_block_scan, txseg_scan_kernel, txseg_search, txseg_store_void

namespace mg {

// The longest list a lane folds by itself.  Measured (the sweep
// of tools/ackgen_bench.py over lists of 8 to 64 packets): thresholds 4 to 32
// cost 84 to 91 us where 64 and 128 cost 75 us, so a list is its lane's own
// until it is longer than one cooperative step takes in.
constexpr uint32_t kAckgenLaneMax = 64;

struct AckGenWork {
    uint64_t plan_off, local_off, pc_off, pb_off, tot_off, bytes;
    uint32_t nwg;
};
inline AckGenWork ackgen_work(uint32_t n) {
    AckGenWork w{};
    w.nwg = (n + kBlock - 1) / kBlock;
    w.plan_off = 0;
    w.local_off = 32ull * n;
    w.pc_off = (w.local_off + 4ull * n + 15) & ~15ull;
    w.pb_off = (w.pc_off + 4ull * w.nwg + 15) & ~15ull;
    w.tot_off = w.pb_off + 8ull * w.nwg;
    w.bytes = w.tot_off + 16;
    return w;
}

struct AckGenParams {
    uint64_t buf_off;
    uint32_t n, max_id, n_links, cur_ts, off_shift, slot, seg_cap;
    uint32_t room;        // ackgen_room: the records the call has room for
};

// ---- plan ---------------------------------------------------------------------
// grid: one workgroup per kBlock segments, for n segments.  LANE_MAX: the
// longest list a lane folds by itself (kAckgenLaneMax in the library; the
// bench tool sweeps it).  place: 16 B records; state: 64 B; snd: 128 B; tx:
// 32 B.  plan[j], local[j] for j < m; part_c / part_b[workgroup] (part_b is the
// scan kernel's second operand: 0).
template <uint32_t LANE_MAX>
__global__ __launch_bounds__(kBlock) void ackgen_plan_kernel(
    const uint8_t *__restrict__ place, const uint32_t *__restrict__ idx, const AckGenParams P,
    const uint32_t *__restrict__ seg_sid, const uint32_t *__restrict__ seg_start, const uint32_t *__restrict__ nseg,
    const uint32_t *__restrict__ seg_stop, const uint32_t *__restrict__ ack_stop, const uint8_t *__restrict__ state,
    const uint8_t *__restrict__ snd, const uint8_t *__restrict__ tx, v4u *__restrict__ plan,
    uint32_t *__restrict__ local, uint32_t *__restrict__ part_c, uint64_t *__restrict__ part_b) {
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
    AckGenTx t{};
    v4u s0 = {0, 0, 0, 0}, s1 = {0, 0, 0, 0};
    uint32_t snd_nxt = 0, stopc = start;
    bool bad = false, deferred = false;
    if (is_stream) {
        const v4u a = gload((uint64_t)tx + 32ull * sid), b = gload((uint64_t)tx + 32ull * sid + 16);
        t.saddr = a.x, t.daddr = a.y, t.ports = a.z, t.id_cnt = a.w;
        t.misc = b.x, t.ts_lastack_sent = b.y, t.rsvd0 = b.z, t.rsvd1 = b.w;
        s0 = gload((uint64_t)state + 64ull * sid);                  // rcv_nxt, rcv_wnd, head_seq, merged_len
        s1 = gload((uint64_t)state + 64ull * sid + 16);             // size, ts_recent, ts_lastack_rcvd, tcp_state | ...
        snd_nxt = gload32((uint64_t)snd + 128ull * sid);
        bad = ackgen_bad(t, P.n_links);
        const uint32_t ss = seg_stop[j];
        deferred = ss < end || (ack_stop && ack_stop[j] < end) || (s1.w & 0xFFu) != MTCP_GPU_RCV_ST_ESTABLISHED;
        if (!bad) stopc = min(max(ss, start), end);
    }
    uint32_t f = (t.id_cnt >> 16) & 63u;
    const bool lng = stopc - start > LANE_MAX;
    if (!lng) {
        for (uint32_t p = start; p < stopc; ++p) {
            const uint32_t q = idx[p];
            if (q >= n) continue;
            f = ackgen_fold(f, gload32((uint64_t)place + 16ull * q + 12));
        }
    }
    // the long lists of these 64 segments, one after the other, as a whole wave
    uint64_t todo = __ballot(lng);
    while (todo) {
        const int l = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1;
        const uint32_t lstart = rcv_bcast(start, l), lend = rcv_bcast(stopc, l);
        uint32_t lf = rcv_bcast(f, l);
        for (uint32_t base = lstart; base < lend; base += kWave) {
            uint32_t w = 0;
            if (lane < lend - base) {
                const uint32_t q = idx[base + lane];
                if (q < n) w = gload32((uint64_t)place + 16ull * q + 12);
            }
            const uint32_t fl = w >> 24;
            lf = ackgen_fold_masks(lf, __ballot(fl & MTCP_GPU_RCV_ACK_NOW), __ballot(fl & MTCP_GPU_RCV_ACK_AGGREGATE),
                                   __ballot(ackgen_is_put(w)));
        }
        if ((int)lane == l) f = lf;
    }
    AckGenPlan pl;
    if (is_stream && !bad) pl = ackgen_plan(t, f, deferred, s0.x, s0.y, s0.z, s0.w, s1.y, snd_nxt);
    else pl = ackgen_plan_none(is_stream ? MTCP_GPU_ACKGEN_BAD : MTCP_GPU_ACKGEN_NONE);
    uint32_t c = 0;
    if (valid) {
        c = ackgen_planned(pl);
        const v4u a = {pl.saddr, pl.daddr, pl.ports, pl.snd_nxt}, b = {pl.rcv_nxt, pl.ts_recent, pl.win_id, pl.meta};
        *reinterpret_cast<gsv4u *>((uint64_t)plan + 32ull * j) = a;
        *reinterpret_cast<gsv4u *>((uint64_t)plan + 32ull * j + 16) = b;
    }
    uint32_t ec, tc;
    uint64_t eb, tb;
    txseg_block_scan<kWavesPerBlock>(c < P.seg_cap ? c : P.seg_cap, 0ull, P.seg_cap, ec, eb, tc, tb);
    if (valid) local[j] = ec;
    if (threadIdx.x == 0) part_c[blockIdx.x] = tc, part_b[blockIdx.x] = 0ull;
}

// ---- emit and commit ------------------------------------------------------------
// grid: one lane per record of seg_cap and per segment of n, whichever is
// more.  part_c: the scanned sums of nwg workgroups; tot_c: their total.
// With n == 0 nothing but seg, desc and d_total is touched.
__global__ __launch_bounds__(kBlock) void ackgen_emit_kernel(
    const v4u *__restrict__ plan, const uint32_t *__restrict__ local, const uint32_t *__restrict__ part_c,
    const uint32_t *__restrict__ tot_c, const uint32_t *__restrict__ nseg, uint32_t nwg, const AckGenParams P,
    const uint32_t *__restrict__ seg_sid, uint8_t *__restrict__ tx, mtcp_gpu_tx_seg *__restrict__ seg,
    mtcp_gpu_desc *__restrict__ desc, mtcp_gpu_ackgen_res *__restrict__ ares, uint64_t *__restrict__ d_total) {
    const uint32_t m = P.n ? min(nseg[0], P.n) : 0u;
    const uint32_t T = P.n ? min(*tot_c, P.room) : 0u;              // room <= seg_cap
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k == 0) d_total[0] = T, d_total[1] = (uint64_t)T * P.slot;
    if (k < P.seg_cap) {
        if (k < T) {
            const uint32_t b = txseg_search(part_c, 0u, nwg - 1, k);
            const uint32_t lo = b * kBlock, hi = min(m, lo + kBlock) - 1, r = k - part_c[b];
            const uint32_t j = txseg_search(local, lo, hi, r);
            const v4u pa = gload((uint64_t)plan + 32ull * j), pb = gload((uint64_t)plan + 32ull * j + 16);
            const AckGenPlan pl = {pa.x, pa.y, pa.z, pa.w, pb.x, pb.y, pb.z, pb.w};
            uint32_t w[12];
            ackgen_record(pl, r - local[j], P.cur_ts, w);
            const v4u a = {w[0], w[1], w[2], w[3]}, c = {w[4], w[5], w[6], w[7]}, e = {w[8], w[9], w[10], w[11]};
            const uint64_t at = (uint64_t)seg + 48ull * k;
            *reinterpret_cast<gsv4u *>(at) = a;
            *reinterpret_cast<gsv4u *>(at + 16) = c;
            *reinterpret_cast<gsv4u *>(at + 32) = e;
            const v2u d = {(uint32_t)((P.buf_off + (uint64_t)k * P.slot) >> P.off_shift), MTCP_GPU_ACKGEN_FRAME_LEN};
            *reinterpret_cast<gsv2u *>((uint64_t)desc + 8ull * k) = d;
        } else {
            txseg_store_void(seg, desc, k);
        }
    }
    if (k < m) {                                                    // the commit of segment k
        const v4u pa = gload((uint64_t)plan + 32ull * k), pb = gload((uint64_t)plan + 32ull * k + 16);
        const AckGenPlan pl = {pa.x, pa.y, pa.z, pa.w, pb.x, pb.y, pb.z, pb.w};
        const uint32_t S = txseg_add_c(part_c[k / kBlock], local[k], P.seg_cap);
        uint32_t t3[3], r[4];
        bool store_ts;
        ackgen_commit(pl, S, P.room, S < T ? S : T, P.cur_ts, t3, &store_ts, r);
        if (ackgen_status(pl) >= MTCP_GPU_ACKGEN_DEFERRED) {
            const uint32_t sid = seg_sid[k];
            if (sid <= P.max_id) {                                  // holds: the plan said so
                uint32_t *rec = reinterpret_cast<uint32_t *>(tx + 32ull * sid);
                rec[3] = t3[0], rec[4] = t3[1];
                if (store_ts) rec[5] = t3[2];
            }
        }
        const v4u rv = {r[0], r[1], r[2], r[3]};
        *reinterpret_cast<gsv4u *>((uint64_t)ares + 16ull * k) = rv;
    }
}

}  // namespace mg
