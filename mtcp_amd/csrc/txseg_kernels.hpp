// txseg_kernels.hpp — gfx950 kernels that cut send bursts into tx segment
// records: FlushTCPSendingBuffer's walk (mtcp/src/tcp_out.c:
// 357-449) over the streams of a send list as WriteTCPDataList runs it
// (tcp_out.c:587-674).  include/mtcp_gpu_txseg.h has the rule; the per-burst
// closed form below (txseg_plan, txseg_emitted) is the one the host entry
// point mtcp_gpu_tx_segment_plan runs as well.
//
// A burst's fan-out is anything from 0 to len / (mss - 12) records, so this is
// count, scan and emit:
//
//   plan   one lane per burst: validate, then in closed form the planned
//          segment count, the bytes of their slots and the stop bits; each
//          plan, parked in 16 B; each workgroup's sums of (count, slot bytes);
//   scan   ONE workgroup: the exclusive prefix of those sums over the
//          workgroups, and their totals;
//   place  one lane per burst again, from the 16 B of its plan that plan has
//          parked (not from the burst's 64 B a second time): the burst's first
//          record index and first slot byte from a workgroup scan on top of
//          the scanned sums; the room cut (seg_cap, buf_len, a 32-bit offset)
//          in closed form; the burst's result; the first burst that is cut
//          lowers the totals to where it stops (a fetch-and-min: every cut
//          burst behind it offers a larger value, so the outcome is a pure
//          function of the bursts);
//   emit   one lane per OUTPUT record, four records per lane, 1 024 per
//          workgroup: the tile's first and last record are searched in the
//          scanned first-record array (a wave each, 64 probes a step, log64
//          n_burst steps), the
//          bursts between them are staged in LDS, first record and first slot
//          byte (or searched in place where
//          more than kTxsegStage bursts, empty ones included, meet one tile)
//          and every lane finds its record's burst there; a 2 000-segment
//          burst among single-segment ones is spread over two tiles' lanes
//          like any other 2 000 records.  A record is three 16 B stores and
//          an 8 B descriptor store, consecutive lanes consecutive records.
//          Records at and past the total are void.  Also here: first_seg of
//          every result (it needs the total) and d_total.
//
// The counts saturate at seg_cap and the slot bytes at 2^62 (a burst may plan
// 2^32 segments, a batch 2^24 bursts): a saturated prefix is past every room
// test, so nothing that is emitted sees one.
//
// No workgroup waits on another (the order between the passes is the
// stream's), every loop's trip count is fixed by n_burst, seg_cap or the tile,
// and every store is bounded by n_burst or seg_cap whatever the bursts or the
// workspace hold.  A batch of at most one plan tile and kTxsegOneSegs records
// is one launch of one workgroup of 1 024 lanes (txseg_one_kernel) and uses no
// workspace.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mtcp_gpu_txseg.h"
#include "rx_kernels.hpp"
#include "txbuild_kernels.hpp"   // gsv4u, v2u

namespace mg {

constexpr uint32_t kTxsegTile = kBlock;                          // bursts per plan workgroup, one per lane
constexpr uint32_t kTxsegPerLane = 4;                            // records per lane of emit
constexpr uint32_t kTxsegEmitTile = kBlock * kTxsegPerLane;      // 1 024 records per emit workgroup
constexpr uint32_t kTxsegOneSegs = 4096;                         // seg_cap of the one-workgroup form
constexpr uint32_t kTxsegOneBlock = 1024;                        // its lanes
constexpr uint32_t kTxsegStage = 2048;                           // first-record entries a tile stages in LDS
constexpr uint64_t kTxsegByteSat = 1ull << 62;

typedef __attribute__((address_space(1))) v2u gsv2u;

struct TxSegParams {
    uint64_t payload_bytes;
    uint64_t buf_off;
    uint64_t room;        // bytes between buf_off and buf_len (0 where no offset from buf_off on fits 32 bits)
    uint64_t off_room;    // the largest byte distance from buf_off whose descriptor offset fits 32 bits
    uint32_t n_links, off_shift, slot_bytes, seg_cap, max_mss, align;
};

inline TxSegParams txseg_params(uint64_t payload_bytes, uint32_t n_links, uint64_t buf_off, uint64_t buf_len,
                                uint32_t off_shift, uint32_t slot_bytes, uint32_t seg_cap, uint32_t max_mss) {
    TxSegParams P{};
    const uint64_t lim = 0xFFFFFFFFull << off_shift;
    P.payload_bytes = payload_bytes;
    P.buf_off = buf_off;
    P.room = (buf_off <= lim && buf_len > buf_off) ? buf_len - buf_off : 0;
    P.off_room = buf_off <= lim ? lim - buf_off : 0;
    P.n_links = n_links;
    P.off_shift = off_shift;
    P.slot_bytes = slot_bytes;
    P.seg_cap = seg_cap;
    P.max_mss = max_mss ? max_mss : MTCP_GPU_TXB_DEFAULT_MSS;
    P.align = off_shift ? 1u << off_shift : 2u;
    return P;
}

// A burst record's sixteen dwords.
struct TxBurst {
    uint64_t payload_off;
    uint32_t saddr, daddr, ports, seq, ack, ts_val, ts_ecr, len, in_flight, window, peer_wnd;
    uint32_t win_id;      // tcp_window | ip_id << 16
    uint32_t mss_link;    // mss | link << 16 | rsvd0 << 24
    uint32_t rsvd1;
};

__host__ __device__ inline TxBurst txseg_unpack(const uint32_t w[16]) {
    TxBurst b;
    b.payload_off = ((uint64_t)w[1] << 32) | w[0];
    b.saddr = w[2], b.daddr = w[3], b.ports = w[4], b.seq = w[5], b.ack = w[6], b.ts_val = w[7], b.ts_ecr = w[8];
    b.len = w[9], b.in_flight = w[10], b.window = w[11], b.peer_wnd = w[12];
    b.win_id = w[13], b.mss_link = w[14], b.rsvd1 = w[15];
    return b;
}

// What the window lets through of one burst (tcp_out.c:357-449), before any
// room test.
struct TxPlan {
    uint32_t status, stop;    // stop: the window's bits
    uint32_t maxlen;          // mss - 12 (tcp_out.c:360)
    uint32_t k_full;          // planned segments of maxlen bytes
    uint32_t tail;            // bytes of the planned last, shorter segment (0: none)
    uint32_t count;           // k_full + (tail ? 1 : 0)
    uint32_t sf, st;          // slot stride of a full segment, of the tail segment
    uint64_t slot_sum;        // slot bytes of the planned segments
};

__host__ __device__ inline uint32_t txseg_align(uint32_t v, uint32_t a) { return (v + a - 1) & ~(a - 1); }

__host__ __device__ inline TxPlan txseg_plan(const TxBurst &b, const TxSegParams &P) {
    TxPlan r{};
    const uint32_t mss = b.mss_link & 0xFFFFu, link = (b.mss_link >> 16) & 0xFFu, rsvd0 = b.mss_link >> 24;
    const uint32_t maxlen = mss - 12u;                               // tcp_out.c:360
    const uint32_t Lf = 66u + maxlen;
    if (rsvd0 || b.rsvd1 || mss < 13u || maxlen > P.max_mss + 12u || Lf > 65535u ||
        (P.slot_bytes && Lf > P.slot_bytes) || link >= P.n_links ||
        (uint64_t)b.in_flight + b.len > 0xFFFFFFFFull) {
        r.status = MTCP_GPU_TXS_BAD_BURST;
        return r;
    }
    if (b.payload_off > P.payload_bytes || b.len > P.payload_bytes - b.payload_off) {
        r.status = MTCP_GPU_TXS_BAD_PAYLOAD;
        return r;
    }
    r.maxlen = maxlen;
    r.sf = P.slot_bytes ? P.slot_bytes : txseg_align(Lf, P.align);
    // segment j < nf is full and passes tcp_out.c:421 iff in_flight + (j + 1) maxlen <= window
    const uint32_t nf = b.len / maxlen, rest = b.len - nf * maxlen;
    const uint32_t avail = b.window >= b.in_flight ? b.window - b.in_flight : 0u;
    const uint32_t kw = avail / maxlen;
    r.k_full = nf < kw ? nf : kw;
    // the shorter last segment is reached iff every full one passed; with it the whole of len is in flight
    const bool tail_sent = r.k_full == nf && rest && (uint64_t)b.in_flight + b.len <= b.window;
    r.tail = tail_sent ? rest : 0u;
    r.count = r.k_full + (tail_sent ? 1u : 0u);
    const uint64_t sent = (uint64_t)r.k_full * maxlen + r.tail;
    if (sent < b.len) {                                              // tcp_out.c:421 failed for the next one
        const uint64_t left = b.len - sent;
        const uint64_t p = left < maxlen ? left : maxlen;
        r.stop = MTCP_GPU_TXS_STOP_WINDOW |
                 ((uint64_t)b.in_flight + sent + p > b.peer_wnd ? MTCP_GPU_TXS_STOP_PEER_WINDOW : 0u);
    }
    r.st = P.slot_bytes ? P.slot_bytes : txseg_align(66u + r.tail, P.align);
    r.slot_sum = (uint64_t)r.k_full * r.sf + (tail_sent ? r.st : 0u);
    return r;
}

// A plan as plan parks it for place, 16 B: k_full, maxlen | tail << 16,
// status | stop << 8, 0 (maxlen and tail are below 2^16 for every burst that
// is not refused); the rest follows from these and the call's parameters.
__host__ __device__ inline void txseg_park(const TxPlan &pl, uint32_t out[4]) {
    out[0] = pl.k_full;
    out[1] = pl.maxlen | (pl.tail << 16);
    out[2] = pl.status | (pl.stop << 8);
    out[3] = 0;
}
__host__ __device__ inline TxPlan txseg_unpark(const uint32_t in[4], const TxSegParams &P) {
    TxPlan r{};
    r.k_full = in[0];
    r.maxlen = in[1] & 0xFFFFu;
    r.tail = in[1] >> 16;
    r.status = in[2] & 0xFFu;
    r.stop = (in[2] >> 8) & 0xFFu;
    if (r.status) return r;
    r.count = r.k_full + (r.tail ? 1u : 0u);
    r.sf = P.slot_bytes ? P.slot_bytes : txseg_align(66u + r.maxlen, P.align);
    r.st = P.slot_bytes ? P.slot_bytes : txseg_align(66u + r.tail, P.align);
    r.slot_sum = (uint64_t)r.k_full * r.sf + (r.tail ? r.st : 0u);
    return r;
}

// What of a planned burst has room, its first record being S and its first
// slot B bytes past buf_off (both possibly saturated).
struct TxEmit {
    uint32_t n, bytes;
    uint64_t slot_sum;
};

__host__ __device__ inline TxEmit txseg_emitted(const TxPlan &pl, uint32_t S, uint64_t B, const TxSegParams &P) {
    uint32_t e = 0;
    if (pl.count && S < P.seg_cap) {
        const uint32_t left = P.seg_cap - S;
        const uint32_t want = pl.count < left ? pl.count : left;
        const uint32_t wf = want < pl.k_full ? want : pl.k_full;
        const uint32_t Lf = 66u + pl.maxlen;
        uint32_t ef = 0;
        if (wf && Lf <= P.room) {
            // full segment j fits iff B + j sf <= lim
            const uint64_t lim = P.off_room < P.room - Lf ? P.off_room : P.room - Lf;
            if (B + (uint64_t)(wf - 1) * pl.sf <= lim) {
                ef = wf;                                             // all of them: every burst but the one cut
            } else if (B <= lim) {
                const uint64_t m = (lim - B) / pl.sf + 1;
                ef = m < wf ? (uint32_t)m : wf;
            }
        }
        e = ef;
        if (ef == wf && want > pl.k_full) {                          // every full one fits and the tail is wanted
            const uint32_t Lt = 66u + pl.tail;
            const uint64_t rel = B + (uint64_t)pl.k_full * pl.sf;
            if (Lt <= P.room && rel <= P.off_room && rel <= P.room - Lt) e = pl.k_full + 1;
        }
    }
    TxEmit r;
    const uint32_t ef = e < pl.k_full ? e : pl.k_full;
    r.n = e;
    r.bytes = (uint32_t)((uint64_t)ef * pl.maxlen) + (e > pl.k_full ? pl.tail : 0u);
    r.slot_sum = (uint64_t)ef * pl.sf + (e > pl.k_full ? pl.st : 0u);
    return r;
}

// The prefix sums' saturating adds.
__host__ __device__ inline uint32_t txseg_add_c(uint32_t a, uint32_t b, uint32_t cap) {
    const uint64_t s = (uint64_t)a + b;
    return s < cap ? (uint32_t)s : cap;
}
__host__ __device__ inline uint64_t txseg_add_b(uint64_t a, uint64_t b) {
    const uint64_t s = a + b;                                        // both at most 2^62
    return s < kTxsegByteSat ? s : kTxsegByteSat;
}

// The result record as one 16 B value.
__host__ __device__ inline void txseg_result(const TxPlan &pl, const TxEmit &em, uint32_t first, uint32_t out[4]) {
    const uint32_t stop = em.n < pl.count ? MTCP_GPU_TXS_STOP_NO_ROOM : pl.stop;
    out[0] = first;
    out[1] = em.n;
    out[2] = em.bytes;
    out[3] = pl.status | (stop << 8);
}

#ifdef __HIPCC__

__device__ __forceinline__ TxBurst txseg_load(const mtcp_gpu_tx_burst *burst, uint32_t i) {
    const uint64_t a = (uint64_t)burst + 64ull * i;
    const v4u q0 = gload(a), q1 = gload(a + 16), q2 = gload(a + 32), q3 = gload(a + 48);
    const uint32_t w[16] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w,
                            q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w};
    return txseg_unpack(w);
}

// Exclusive saturating prefix of (c, b) over the workgroup's lanes (WAVES
// waves of them), and the workgroup's sums.  Every lane calls it.
template <int WAVES>
__device__ __forceinline__ void txseg_block_scan(uint32_t c, uint64_t b, uint32_t cap, uint32_t &ec, uint64_t &eb,
                                                 uint32_t &tc, uint64_t &tb) {
    __shared__ uint32_t wc[WAVES];
    __shared__ uint64_t wb[WAVES];
    const uint32_t lane = threadIdx.x & (kWave - 1), wib = threadIdx.x / kWave;
    uint32_t ic = c;
    uint64_t ib = b;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const uint32_t oc = __shfl_up(ic, d, kWave);
        const uint64_t ob = __shfl_up(ib, d, kWave);
        if (lane >= (uint32_t)d) {
            ic = txseg_add_c(oc, ic, cap);
            ib = txseg_add_b(ob, ib);
        }
    }
    if (lane == kWave - 1) wc[wib] = ic, wb[wib] = ib;
    const uint32_t pc = __shfl_up(ic, 1, kWave);                     // the lanes below this one
    const uint64_t pb = __shfl_up(ib, 1, kWave);
    __syncthreads();
    uint32_t before_c = 0;
    uint64_t before_b = 0;
    tc = 0, tb = 0;
    for (int w = 0; w < WAVES; ++w) {
        if (w < (int)wib) before_c = txseg_add_c(before_c, wc[w], cap), before_b = txseg_add_b(before_b, wb[w]);
        tc = txseg_add_c(tc, wc[w], cap), tb = txseg_add_b(tb, wb[w]);
    }
    ec = lane ? txseg_add_c(before_c, pc, cap) : before_c;
    eb = lane ? txseg_add_b(before_b, pb) : before_b;
    __syncthreads();
}

// The largest i in [lo, hi] with first[i] <= k; first[lo] <= k.
template <typename P>
__device__ __forceinline__ uint32_t txseg_search(P first, uint32_t lo, uint32_t hi, uint32_t k) {
    while (lo < hi) {
        const uint32_t m = lo + ((hi - lo + 1) >> 1);
        if (first[m] <= k) lo = m;
        else hi = m - 1;
    }
    return lo;
}

// The same over [0, n) by a whole wave, 64 probes a step: log64 n dependent
// loads where the binary search has log2 n.  Every lane of the wave calls it
// with the same arguments; first[0] <= k.
__device__ __forceinline__ uint32_t txseg_wave_search(const uint32_t *__restrict__ first, uint32_t n, uint32_t k) {
    const uint32_t lane = threadIdx.x & (kWave - 1);
    uint32_t lo = 0, len = n;                                        // the answer is in [lo, lo + len)
    while (len > 1) {
        const uint32_t step = (len + kWave - 1) / kWave;
        const bool ok = lane * step < len && first[lo + lane * step] <= k;       // lane 0's holds
        const uint64_t m = __ballot(ok) | 1ull;                      // first[] ascends: a run of lanes from 0
        const uint32_t j = 63u - (uint32_t)__clzll((long long)m);
        lo += j * step;
        len = len - j * step < step ? len - j * step : step;
    }
    return lo;
}

// Record k: segment j of burst u, whose first slot is B bytes past buf_off
// (tcp_out.c:404-411, :437; :284, :332; ip_out.c:139).
__device__ __forceinline__ void txseg_store(const TxBurst &u, uint32_t j, uint64_t B, const TxSegParams &P,
                                            mtcp_gpu_tx_seg *seg, mtcp_gpu_desc *desc, uint32_t k) {
    const uint32_t mss = u.mss_link & 0xFFFFu, link = (u.mss_link >> 16) & 0xFFu;
    const uint32_t maxlen = mss - 12u;
    const uint32_t sf = P.slot_bytes ? P.slot_bytes : txseg_align(66u + maxlen, P.align);
    const uint64_t sent = (uint64_t)j * maxlen;                      // every segment before j is full
    const uint64_t left = u.len - sent;
    const uint32_t p = left < maxlen ? (uint32_t)left : maxlen;      // tcp_out.c:407-411
    const uint64_t po = u.payload_off + sent;
    const uint32_t ip_id = ((u.win_id >> 16) + j) & 0xFFFFu;
    const v4u a = {(uint32_t)po, (uint32_t)(po >> 32), u.saddr, u.daddr};
    const v4u b = {u.ports, u.seq + (uint32_t)sent, u.ack, u.ts_val};
    const v4u c = {u.ts_ecr, (u.win_id & 0xFFFFu) | (ip_id << 16), p | (mss << 16),
                   MTCP_GPU_TXB_FLAG_ACK | (1u << 8) | (link << 24)};
    const uint64_t at = (uint64_t)seg + 48ull * k;
    *reinterpret_cast<gsv4u *>(at) = a;
    *reinterpret_cast<gsv4u *>(at + 16) = b;
    *reinterpret_cast<gsv4u *>(at + 32) = c;
    const v2u d = {(uint32_t)((P.buf_off + B + (uint64_t)j * sf) >> P.off_shift), 66u + p};
    *reinterpret_cast<gsv2u *>((uint64_t)desc + 8ull * k) = d;
}

__device__ __forceinline__ void txseg_store_void(mtcp_gpu_tx_seg *seg, mtcp_gpu_desc *desc, uint32_t k) {
    const v4u z = {0, 0, 0, 0};
    const v4u c = {0, 0, 0, MTCP_GPU_TXSEG_VOID_FORM << 8};
    const uint64_t at = (uint64_t)seg + 48ull * k;
    *reinterpret_cast<gsv4u *>(at) = z;
    *reinterpret_cast<gsv4u *>(at + 16) = z;
    *reinterpret_cast<gsv4u *>(at + 32) = c;
    const v2u d = {0, 0};
    *reinterpret_cast<gsv2u *>((uint64_t)desc + 8ull * k) = d;
}

// ---- plan -------------------------------------------------------------------
// grid: one workgroup per kTxsegTile bursts.  park[i]: burst i's plan (16 B);
// part_c / part_b[workgroup]: its sums.
__global__ __launch_bounds__(kBlock) void txseg_plan_kernel(const mtcp_gpu_tx_burst *__restrict__ burst, uint32_t n,
                                                            const TxSegParams P, v4u *__restrict__ park,
                                                            uint32_t *__restrict__ part_c,
                                                            uint64_t *__restrict__ part_b) {
    const uint32_t i = blockIdx.x * kTxsegTile + threadIdx.x;
    uint32_t c = 0;
    uint64_t b = 0;
    if (i < n) {
        const TxPlan pl = txseg_plan(txseg_load(burst, i), P);
        c = pl.count < P.seg_cap ? pl.count : P.seg_cap;
        b = pl.slot_sum;
        uint32_t w[4];
        txseg_park(pl, w);
        const v4u v = {w[0], w[1], w[2], w[3]};
        *reinterpret_cast<gsv4u *>((uint64_t)park + 16ull * i) = v;
    }
    uint32_t ec, tc;
    uint64_t eb, tb;
    txseg_block_scan<kWavesPerBlock>(c, b, P.seg_cap, ec, eb, tc, tb);
    if (threadIdx.x == 0) part_c[blockIdx.x] = tc, part_b[blockIdx.x] = tb;
}

// ---- scan -------------------------------------------------------------------
// grid: ONE workgroup.  The nwg sums in, their exclusive prefix out, in place;
// tot_c / tot_b: the totals (what place lowers where a burst is cut).
__global__ __launch_bounds__(kBlock) void txseg_scan_kernel(uint32_t *__restrict__ part_c,
                                                            uint64_t *__restrict__ part_b, uint32_t nwg,
                                                            uint32_t cap, uint32_t *__restrict__ tot_c,
                                                            unsigned long long *__restrict__ tot_b) {
    uint32_t carry_c = 0;
    uint64_t carry_b = 0;
    for (uint32_t base = 0; base < nwg; base += kBlock) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t c = i < nwg ? part_c[i] : 0u;
        const uint64_t b = i < nwg ? part_b[i] : 0ull;
        uint32_t ec, tc;
        uint64_t eb, tb;
        txseg_block_scan<kWavesPerBlock>(c < cap ? c : cap, b < kTxsegByteSat ? b : kTxsegByteSat, cap, ec, eb, tc,
                                         tb);
        if (i < nwg) part_c[i] = txseg_add_c(carry_c, ec, cap), part_b[i] = txseg_add_b(carry_b, eb);
        carry_c = txseg_add_c(carry_c, tc, cap);
        carry_b = txseg_add_b(carry_b, tb);
    }
    if (threadIdx.x == 0) *tot_c = carry_c, *tot_b = carry_b;
}

// ---- place ------------------------------------------------------------------
// grid: as plan.  first[i], boff[i]: burst i's first record and first slot
// byte; res[i] but for first_seg's cap at the total, which emit applies.
__global__ __launch_bounds__(kBlock) void txseg_place_kernel(const v4u *__restrict__ park, uint32_t n,
                                                             const TxSegParams P,
                                                             const uint32_t *__restrict__ part_c,
                                                             const uint64_t *__restrict__ part_b,
                                                             uint32_t *__restrict__ first,
                                                             uint64_t *__restrict__ boff,
                                                             mtcp_gpu_tx_burst_result *__restrict__ res,
                                                             uint32_t *__restrict__ tot_c,
                                                             unsigned long long *__restrict__ tot_b) {
    const uint32_t i = blockIdx.x * kTxsegTile + threadIdx.x;
    TxPlan pl{};
    if (i < n) {
        const v4u v = gload((uint64_t)park + 16ull * i);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        pl = txseg_unpark(w, P);
    }
    uint32_t ec, tc;
    uint64_t eb, tb;
    txseg_block_scan<kWavesPerBlock>(pl.count < P.seg_cap ? pl.count : P.seg_cap, pl.slot_sum, P.seg_cap, ec, eb,
                                     tc, tb);
    if (i >= n) return;
    const uint32_t S = txseg_add_c(part_c[blockIdx.x], ec, P.seg_cap);
    const uint64_t B = txseg_add_b(part_b[blockIdx.x], eb);
    const TxEmit em = txseg_emitted(pl, S, B, P);
    first[i] = S;
    boff[i] = B;
    uint32_t r[4];
    txseg_result(pl, em, S, r);
    const v4u rv = {r[0], r[1], r[2], r[3]};
    *reinterpret_cast<gsv4u *>((uint64_t)res + 16ull * i) = rv;
    if (em.n < pl.count) {                                           // cut: the totals end where this one stops
        atomicMin(tot_c, S + em.n);
        atomicMin(tot_b, (unsigned long long)(B + em.slot_sum));
    }
}

// ---- emit -------------------------------------------------------------------
// grid: one workgroup per kTxsegEmitTile records of seg_cap.
__global__ __launch_bounds__(kBlock) void txseg_emit_kernel(const mtcp_gpu_tx_burst *__restrict__ burst, uint32_t n,
                                                            const TxSegParams P,
                                                            const uint32_t *__restrict__ first,
                                                            const uint64_t *__restrict__ boff,
                                                            const uint32_t *__restrict__ tot_c,
                                                            const unsigned long long *__restrict__ tot_b,
                                                            mtcp_gpu_tx_seg *__restrict__ seg,
                                                            mtcp_gpu_desc *__restrict__ desc,
                                                            mtcp_gpu_tx_burst_result *__restrict__ res,
                                                            uint64_t *__restrict__ d_total) {
    __shared__ uint32_t sfirst[kTxsegStage];
    __shared__ uint64_t sboff[kTxsegStage];
    __shared__ uint32_t range[2];
    const uint32_t tid = threadIdx.x;
    const uint32_t T = n ? (*tot_c < P.seg_cap ? *tot_c : P.seg_cap) : 0u;
    for (uint32_t i = blockIdx.x * kBlock + tid; i < n; i += gridDim.x * kBlock) {
        const uint32_t f = first[i];
        *reinterpret_cast<__attribute__((address_space(1))) uint32_t *>((uint64_t)res + 16ull * i) = f < T ? f : T;
    }
    if (blockIdx.x == 0 && tid == 0) d_total[0] = T, d_total[1] = n ? *tot_b : 0ull;

    const uint32_t base = blockIdx.x * kTxsegEmitTile;
    uint32_t lo = 0, hi = 0;
    bool staged = false;
    if (base < T) {                                                  // the same in every lane
        const uint32_t last = (T - base < kTxsegEmitTile ? T : base + kTxsegEmitTile) - 1;
        if (tid < 2 * kWave) {                                       // wave 0: the first record's burst, wave 1: the last's
            const uint32_t at = txseg_wave_search(first, n, tid < kWave ? base : last);
            if ((tid & (kWave - 1)) == 0) range[tid / kWave] = at;
        }
        __syncthreads();
        lo = range[0], hi = range[1];
        staged = hi - lo < kTxsegStage;
        if (staged) {
            for (uint32_t i = tid; i <= hi - lo; i += kBlock) sfirst[i] = first[lo + i], sboff[i] = boff[lo + i];
            __syncthreads();
        }
    }
    // three sweeps over the lane's four records, so that their searches, then
    // their burst loads, are in flight together
    uint32_t src[kTxsegPerLane], seg_j[kTxsegPerLane];
    uint64_t slot0[kTxsegPerLane];
#pragma unroll
    for (uint32_t r = 0; r < kTxsegPerLane; ++r) {
        const uint32_t k = base + r * kBlock + tid;
        src[r] = seg_j[r] = 0, slot0[r] = 0;
        if (k >= T) continue;
        if (staged) {
            const uint32_t i = txseg_search(sfirst, 0u, hi - lo, k);
            src[r] = lo + i, seg_j[r] = k - sfirst[i], slot0[r] = sboff[i];
        } else {
            const uint32_t i = txseg_search(first, lo, hi, k);
            src[r] = i, seg_j[r] = k - first[i], slot0[r] = boff[i];
        }
    }
    TxBurst u[kTxsegPerLane];
#pragma unroll
    for (uint32_t r = 0; r < kTxsegPerLane; ++r) {
        u[r] = TxBurst{};
        if (base + r * kBlock + tid < T) u[r] = txseg_load(burst, src[r]);
    }
#pragma unroll
    for (uint32_t r = 0; r < kTxsegPerLane; ++r) {
        const uint32_t k = base + r * kBlock + tid;
        if (k >= P.seg_cap) continue;
        if (k < T) txseg_store(u[r], seg_j[r], slot0[r], P, seg, desc, k);
        else txseg_store_void(seg, desc, k);
    }
}

// ---- n_burst <= kTxsegTile and seg_cap <= kTxsegOneSegs: one workgroup ------
// of kTxsegOneBlock lanes: the first kTxsegTile plan a burst each, all of them
// emit, four records each at the most.
__global__ __launch_bounds__(kTxsegOneBlock) void txseg_one_kernel(const mtcp_gpu_tx_burst *__restrict__ burst,
                                                                   uint32_t n, const TxSegParams P,
                                                                   mtcp_gpu_tx_seg *__restrict__ seg,
                                                                   mtcp_gpu_desc *__restrict__ desc,
                                                                   mtcp_gpu_tx_burst_result *__restrict__ res,
                                                                   uint64_t *__restrict__ d_total) {
    __shared__ uint32_t sfirst[kTxsegTile];
    __shared__ uint64_t sboff[kTxsegTile];
    __shared__ uint32_t s_tot_c;
    __shared__ unsigned long long s_tot_b;
    const uint32_t tid = threadIdx.x;
    TxPlan pl{};
    if (tid < n) pl = txseg_plan(txseg_load(burst, tid), P);         // n <= kTxsegTile
    uint32_t S, tc;
    uint64_t B, tb;
    txseg_block_scan<kTxsegOneBlock / kWave>(pl.count < P.seg_cap ? pl.count : P.seg_cap, pl.slot_sum, P.seg_cap, S,
                                             B, tc, tb);
    if (tid == 0) s_tot_c = tc, s_tot_b = tb;
    if (tid < kTxsegTile) {
        sfirst[tid] = tid < n ? S : P.seg_cap;                       // past n: past every record
        sboff[tid] = B;
    }
    __syncthreads();
    const TxEmit em = txseg_emitted(pl, S, B, P);
    if (tid < n && em.n < pl.count) {
        atomicMin(&s_tot_c, S + em.n);
        atomicMin(&s_tot_b, (unsigned long long)(B + em.slot_sum));
    }
    __syncthreads();
    const uint32_t T = s_tot_c;
    if (tid < n) {
        uint32_t r[4];
        txseg_result(pl, em, S < T ? S : T, r);
        const v4u rv = {r[0], r[1], r[2], r[3]};
        *reinterpret_cast<gsv4u *>((uint64_t)res + 16ull * tid) = rv;
    }
    if (tid == 0) d_total[0] = T, d_total[1] = s_tot_b;
    static_assert(kTxsegOneSegs == kTxsegPerLane * kTxsegOneBlock, "four records per lane cover the form's seg_cap");
    uint32_t src[kTxsegPerLane];
#pragma unroll
    for (uint32_t r = 0; r < kTxsegPerLane; ++r) {
        const uint32_t k = r * kTxsegOneBlock + tid;
        src[r] = k < T ? txseg_search(sfirst, 0u, kTxsegTile - 1, k) : 0u;
    }
    TxBurst u[kTxsegPerLane];
#pragma unroll
    for (uint32_t r = 0; r < kTxsegPerLane; ++r) {
        u[r] = TxBurst{};
        if (r * kTxsegOneBlock + tid < T) u[r] = txseg_load(burst, src[r]);
    }
#pragma unroll
    for (uint32_t r = 0; r < kTxsegPerLane; ++r) {
        const uint32_t k = r * kTxsegOneBlock + tid;
        if (k >= P.seg_cap) continue;
        if (k < T) txseg_store(u[r], k - sfirst[src[r]], sboff[src[r]], P, seg, desc, k);
        else txseg_store_void(seg, desc, k);
    }
}

#endif  // __HIPCC__

}  // namespace mg
