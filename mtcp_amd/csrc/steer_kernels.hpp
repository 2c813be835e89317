// steer_kernels.hpp — gfx950 kernels of the steer step:
// a stable partition of an rx batch by destination queue, the device-side
// counterpart of what the NIC's RSS redirection table does in the reference
// (mtcp/src/dpdk_module.c:101-121: each frame into the receive ring of one
// core; dpdk_module.c:401-402: each mTCP thread reads only its own ring), over
// the queue byte GetRSSCPUCore (mtcp/src/rss.c:90-103) gave every frame.
//
// There are L = Q + 1 lists: the Q queues and the rest list (include/
// mtcp_gpu_steer.h has the rule).  A tile is kSteerTile consecutive packets,
// one workgroup; inside it wave w owns the kSteerWaveChunk consecutive packets
// [w * 1024, (w + 1) * 1024) and walks them in 16 rounds of 64, a lane one
// packet per round.  So packet order is (tile, wave, round, lane), and
// everything below ranks in that order:
//
//   count  every tile: the destination byte of each record (one dword load per
//          record), parked in the workspace (emit then reads 1 B per packet,
//          not the records again), and each WAVE's count per list;
//   scan   one workgroup per list: the exclusive prefix of that list's counts
//          over all waves of all tiles, in place, and the list's total;
//   emit   every tile: the lists' starts (an exclusive scan of the L totals,
//          redone by every workgroup: 129 values), then per wave and round
//          the rank of every packet, and the stores.
//
// The wave-level primitive (steer_group): one __ballot per bit of the
// destination (as many bits as tell 0 .. Q apart, eight at Q = 128) give every lane the 64-bit mask of its wave's lanes with the same
// destination; a lane's rank in the round is popc(mask & lanes_below), and the
// lowest lane of each group moves the wave's LDS counter of that list by the
// group's size.  No scan per list.
//
// That counter move is an LDS fetch-and-add, and it decides no order: a
// counter row belongs to one wave, within a round its writers hold distinct
// lists, and the rounds are one wave's instructions, which the LDS executes in
// the order they were issued.  It is that instruction rather than a load and
// a store because it needs no answer before the next round's is issued: the
// 16 rounds are in flight together instead of waiting on one another.  The
// result is a pure function of the records.
//
// No workgroup waits on another (the order between the passes is the
// stream's), every loop's trip count is fixed by n, the tile or L, and every
// store is bounded by n whatever the records or the workspace hold.
// A batch of at most one tile is one launch of one workgroup (steer_one_kernel)
// and uses no workspace.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mtcp_gpu.h"
#include "flow_kernels.hpp"      // block_exclusive_scan
#include "rx_kernels.hpp"

namespace mg {

constexpr int kSteerRounds = 16;                                  // packets per lane
constexpr uint32_t kSteerWaveChunk = kWave * kSteerRounds;        // 1024 consecutive packets per wave
constexpr uint32_t kSteerTile = kBlock * kSteerRounds;            // 4096 per workgroup
constexpr uint32_t kSteerMaxLists = 129;                          // MTCP_GPU_STEER_MAX_QUEUES + the rest list
constexpr uint32_t kSteerNone = 0xFFu;                            // a lane past n: in no list
static_assert(kSteerMaxLists <= kBlock, "one lane per list in the per-list steps");
static_assert(kSteerMaxLists <= kSteerNone, "kSteerNone must be no list");
static_assert(kWavesPerBlock == 4, "a tile's four wave counts of a list are one 16 B piece");

// The list of one record from its dword holding verdict and rss_queue (dword 9
// of a 40 B record: verdict byte 0, queue byte 1; dword 3 of a 16 B one:
// bytes 2 and 3).  drop: MTCP_GPU_STEER_DROP_BAD.
template <bool CMP>
__device__ __forceinline__ uint32_t steer_dest(uint32_t w, uint32_t Q, bool drop) {
    const uint32_t verdict = CMP ? (w >> 16) & 0xFFu : w & 0xFFu;
    const uint32_t queue = CMP ? w >> 24 : (w >> 8) & 0xFFu;
    const bool bad = verdict == MTCP_GPU_V_IP_CSUM_BAD || verdict == MTCP_GPU_V_TCP_CSUM_BAD ||
                     verdict >= MTCP_GPU_V_TRUNCATED;             // TRUNCATED, BAD_DESC and above
    return (queue >= Q || (drop && bad)) ? Q : queue;
}

template <bool CMP>
__device__ __forceinline__ uint32_t steer_load(const uint32_t *res, uint32_t i) {
    return res[CMP ? 4ull * i + 3 : 10ull * i + 9];
}

// Bits that tell the lists 0 .. Q apart: 1 for Q = 1, 5 for Q = 16, 8 for Q = 128.
__device__ __forceinline__ uint32_t steer_bits(uint32_t Q) { return 32u - (uint32_t)__clz((int)Q); }

// The lanes of this wave with lane's destination d (every lane calls it;
// d == kSteerNone joins no group and gets 0): one ballot per bit of the
// destination, kept where the lane's own bit is set and inverted where not.
__device__ __forceinline__ uint64_t steer_group(uint32_t d, uint32_t nbits) {
    uint64_t m = __ballot(d != kSteerNone);
    for (uint32_t b = 0; b < nbits; ++b) {
        const uint64_t v = __ballot((d >> b) & 1u);
        const uint32_t t = ((d >> b) & 1u) - 1u;                 // 0 where the bit is set, ~0 where not
        m &= v ^ (((uint64_t)t << 32) | t);
    }
    return d != kSteerNone ? m : 0ull;
}

// Lanes of m below this one.
__device__ __forceinline__ uint32_t steer_rank(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// One wave's fetch-and-add on its own counter row (see the head comment).
__device__ __forceinline__ uint32_t steer_bump(uint32_t *counter, uint32_t by) {
    return __hip_atomic_fetch_add(counter, by, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

// The 16 destinations of a lane, one byte each, round 0 first.
struct SteerDests {
    uint32_t w[kSteerRounds / 4];
    __device__ __forceinline__ uint32_t get(int r) const { return (w[r >> 2] >> (8 * (r & 3))) & 0xFFu; }
    __device__ __forceinline__ void set(int r, uint32_t d) { w[r >> 2] |= d << (8 * (r & 3)); }
};

// Packet of (tile, this lane's wave, round r).
__device__ __forceinline__ uint32_t steer_pkt(uint32_t tile, int r) {
    return tile * kSteerTile + (threadIdx.x / kWave) * kSteerWaveChunk + (uint32_t)r * kWave +
           (threadIdx.x & (kWave - 1));
}

// hist_w[l] += this wave's packets in list l (hist zeroed, a barrier since).
__device__ __forceinline__ void steer_wave_hist(const SteerDests &ds, uint32_t *hist_w, uint32_t nbits) {
#pragma unroll
    for (int r = 0; r < kSteerRounds; ++r) {
        const uint32_t d = ds.get(r);
        const uint64_t m = steer_group(d, nbits);
        if (m && steer_rank(m) == 0) (void)steer_bump(&hist_w[d], (uint32_t)__popcll(m));
    }
}

// cur_w[l]: where this wave's next packet of list l goes.  Stores idx of every
// packet of the wave's chunk; nothing at or past n.  With GATHER a lane loads
// its 16 descriptors first, all in flight at once: a load inside the ranking
// rounds would put its latency into every round.
template <bool GATHER>
__device__ __forceinline__ void steer_wave_emit(const SteerDests &ds, uint32_t *cur_w, uint32_t nbits,
                                                uint32_t tile, uint32_t n, uint32_t *__restrict__ idx,
                                                const uint2 *__restrict__ desc,
                                                uint2 *__restrict__ desc_out) {
    uint2 v[GATHER ? kSteerRounds : 1];
    if constexpr (GATHER) {
#pragma unroll
        for (int r = 0; r < kSteerRounds; ++r) {
            const uint32_t pkt = steer_pkt(tile, r);
            v[r] = pkt < n ? desc[pkt] : make_uint2(0u, 0u);
        }
    }
#pragma unroll
    for (int r = 0; r < kSteerRounds; ++r) {
        const uint32_t d = ds.get(r);
        const uint64_t m = steer_group(d, nbits);
        const uint32_t rank = steer_rank(m);
        uint32_t base = 0;
        if (m && rank == 0) base = steer_bump(&cur_w[d], (uint32_t)__popcll(m));
        base = __shfl(base, m ? __ffsll((unsigned long long)m) - 1 : 0, kWave);    // from the group's lowest lane
        const uint32_t p = base + rank;
        if (m && p < n) {
            idx[p] = steer_pkt(tile, r);
            if constexpr (GATHER) desc_out[p] = v[r];
        }
    }
}

// ---- count ------------------------------------------------------------------
// grid: one workgroup per tile.  dest[n]: the parked destination bytes;
// cnt[l * 4 * ntiles + 4 * tile + w]: wave w's packets in list l (list-major,
// so that scan reads one list contiguously).
template <bool CMP>
__global__ __launch_bounds__(kBlock) void steer_count_kernel(const uint32_t *__restrict__ res, uint32_t n,
                                                             uint32_t Q, uint32_t drop,
                                                             uint8_t *__restrict__ dest,
                                                             uint32_t *__restrict__ cnt, uint32_t ntiles) {
    __shared__ uint32_t hist[kWavesPerBlock][kSteerMaxLists];
    const uint32_t tid = threadIdx.x, L = Q + 1, tile = blockIdx.x;
    for (uint32_t i = tid; i < kWavesPerBlock * kSteerMaxLists; i += kBlock) (&hist[0][0])[i] = 0;
    SteerDests ds{};
#pragma unroll
    for (int r = 0; r < kSteerRounds; ++r) {
        const uint32_t pkt = steer_pkt(tile, r);
        uint32_t d = kSteerNone;
        if (pkt < n) {
            d = steer_dest<CMP>(steer_load<CMP>(res, pkt), Q, drop != 0);
            dest[pkt] = (uint8_t)d;
        }
        ds.set(r, d);
    }
    __syncthreads();
    steer_wave_hist(ds, hist[tid / kWave], steer_bits(Q));
    __syncthreads();
    if (tid < L)
        reinterpret_cast<uint4 *>(cnt)[(uint64_t)tid * ntiles + tile] =
            make_uint4(hist[0][tid], hist[1][tid], hist[2][tid], hist[3][tid]);
}

// ---- scan -------------------------------------------------------------------
// grid: one workgroup per list.  Its len = 4 * ntiles counts (every wave of
// every tile) in, their exclusive prefix out; totals[l]: the list's length.
__global__ __launch_bounds__(kBlock) void steer_scan_kernel(uint32_t *__restrict__ cnt, uint32_t len,
                                                            uint32_t *__restrict__ totals) {
    uint32_t *c = cnt + (uint64_t)blockIdx.x * len;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < len; base += kBlock) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < len ? c[i] : 0u;
        uint32_t excl;
        const uint32_t tot = block_exclusive_scan(v, excl);
        if (i < len) c[i] = carry + excl;
        carry += tot;
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

// ---- emit -------------------------------------------------------------------
// grid: one workgroup per tile.  Workgroup 0 also writes start[0 .. L].
template <bool GATHER>
__global__ __launch_bounds__(kBlock) void steer_emit_kernel(const uint8_t *__restrict__ dest, uint32_t n,
                                                            uint32_t Q, const uint32_t *__restrict__ cnt,
                                                            const uint32_t *__restrict__ totals,
                                                            uint32_t ntiles, uint32_t *__restrict__ idx,
                                                            uint32_t *__restrict__ start,
                                                            const uint2 *__restrict__ desc,
                                                            uint2 *__restrict__ desc_out) {
    __shared__ uint32_t cur[kWavesPerBlock][kSteerMaxLists];
    const uint32_t tid = threadIdx.x, L = Q + 1, tile = blockIdx.x;
    SteerDests ds{};
#pragma unroll
    for (int r = 0; r < kSteerRounds; ++r) {
        const uint32_t pkt = steer_pkt(tile, r);
        uint32_t d = kSteerNone;
        if (pkt < n) d = min((uint32_t)dest[pkt], Q);             // never a list past the rest list
        ds.set(r, d);
    }
    uint32_t first;                                               // list tid's start (exclusive scan of totals)
    (void)block_exclusive_scan(tid < L ? totals[tid] : 0u, first);
    if (tid < L) {
        if (tile == 0) start[tid] = first;
        const uint4 c = reinterpret_cast<const uint4 *>(cnt)[(uint64_t)tid * ntiles + tile];
        cur[0][tid] = first + c.x;
        cur[1][tid] = first + c.y;
        cur[2][tid] = first + c.z;
        cur[3][tid] = first + c.w;
    } else if (tid == L && tile == 0) {
        start[L] = n;
    }
    __syncthreads();
    steer_wave_emit<GATHER>(ds, cur[tid / kWave], steer_bits(Q), tile, n, idx, desc, desc_out);
}

// ---- n <= kSteerTile: everything in one workgroup -----------------------------
template <bool CMP, bool GATHER>
__global__ __launch_bounds__(kBlock) void steer_one_kernel(const uint32_t *__restrict__ res, uint32_t n,
                                                           uint32_t Q, uint32_t drop,
                                                           uint32_t *__restrict__ idx,
                                                           uint32_t *__restrict__ start,
                                                           const uint2 *__restrict__ desc,
                                                           uint2 *__restrict__ desc_out) {
    __shared__ uint32_t cur[kWavesPerBlock][kSteerMaxLists];
    const uint32_t tid = threadIdx.x, L = Q + 1;
    for (uint32_t i = tid; i < kWavesPerBlock * kSteerMaxLists; i += kBlock) (&cur[0][0])[i] = 0;
    SteerDests ds{};
#pragma unroll
    for (int r = 0; r < kSteerRounds; ++r) {
        const uint32_t pkt = steer_pkt(0, r);
        uint32_t d = kSteerNone;
        if (pkt < n) d = steer_dest<CMP>(steer_load<CMP>(res, pkt), Q, drop != 0);
        ds.set(r, d);
    }
    __syncthreads();
    steer_wave_hist(ds, cur[tid / kWave], steer_bits(Q));
    __syncthreads();
    uint32_t total = 0;
    if (tid < L) {
#pragma unroll
        for (int w = 0; w < kWavesPerBlock; ++w) total += cur[w][tid];
    }
    uint32_t first;
    (void)block_exclusive_scan(total, first);
    if (tid < L) {
        start[tid] = first;
        uint32_t run = first;
#pragma unroll
        for (int w = 0; w < kWavesPerBlock; ++w) {
            const uint32_t c = cur[w][tid];
            cur[w][tid] = run;
            run += c;
        }
    } else if (tid == L) {
        start[L] = n;
    }
    __syncthreads();
    // the second walk recomputes its groups: kept from the first walk, the 16
    // masks of both walks' unrolled rounds cost more registers than a wave has
#pragma unroll
    for (int i = 0; i < kSteerRounds / 4; ++i) asm volatile("" : "+v"(ds.w[i]));
    steer_wave_emit<GATHER>(ds, cur[tid / kWave], steer_bits(Q), 0, n, idx, desc, desc_out);
}

}  // namespace mg
