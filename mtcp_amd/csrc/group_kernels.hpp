// group_kernels.hpp — gfx950 kernels of the group step: a
// stable partition of an rx batch by stream id, the device-side counterpart of
// what RunMainLoop's burst walk (mtcp/src/core.c:768-777) gives the stateful
// tail behind StreamHTSearch (mtcp/src/tcp_in.c:1181-1186) for free: every
// stream's segments together, in arrival order.  include/mtcp_gpu_group.h has
// the contract.
//
// The key of a record is its stream id, max_id + 1 for MISS and max_id + 2 for
// NONE and for everything else (group_key), so the keys have as many bits as
// max_id + 2 and sort into the contract's class order.  The (key, index) pairs
// go through a least-significant-digit radix sort: `passes` stable partitions
// by one digit of at most kGroupDigitBits bits, the key bits spread evenly over
// the passes (group_digit).  The pairs ping-pong through the workspace; the
// first pass reads d_sid and the index is the position, the last writes its
// indices to d_idx.
//
// A pass is the three launches of steer_kernels.hpp, with its packet order
// (tile, wave, round, lane) and its wave-level ranking (a ballot per digit bit,
// mbcnt rank, per-wave LDS counters whose fetch-and-add decides no order):
//
//   count  every tile: each WAVE's count per digit value;
//   scan   one workgroup per digit value: the exclusive prefix of its counts
//          over all waves of all tiles;
//   emit   every tile: the values' starts (an exclusive scan of the totals,
//          redone by every workgroup), the rank of every pair, and the stores.
//
// A tile of these passes is kGroupSubTile = 1024 records, four rounds a lane:
// a wave's rounds are a serial walk, and at 16 rounds a batch of 1 M records is
// 256 workgroups that spend their time in that walk on an idle GPU.
//
// Behind the last pass the sorted keys are in the workspace; a record heads a
// segment when its key differs from its predecessor's.  seg_count counts the
// heads per wave, the scan kernel scans those counts, seg_emit ranks the heads
// and writes the table.
//
// As in the steer step: no workgroup waits on another (the order between the
// launches is the stream's), every loop's trip count is fixed by n, the tile or
// max_id, no global atomic decides a position, and every store is bounded by n
// whatever d_sid or the workspace hold.  A batch of at most kGroupTile = 4096
// records is one launch of one workgroup (group_one_kernel, 16 rounds a lane):
// the pairs ping-pong through LDS and no workspace is used.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mtcp_gpu.h"
#include "../../include/mtcp_gpu_flowtab.h"
#include "steer_kernels.hpp"     // steer_rank, steer_bump, block_exclusive_scan

namespace mg {

constexpr int kGroupOneRounds = kSteerRounds;                     // records per lane of group_one_kernel
constexpr uint32_t kGroupTile = kBlock * kGroupOneRounds;         // 4096: the largest batch of one workgroup
constexpr int kGroupRounds = 4;                                   // records per lane of the passes
constexpr uint32_t kGroupSubTile = kBlock * kGroupRounds;         // 1024 records per workgroup of the passes
constexpr uint32_t kGroupDigitBits = 8;                           // the widest digit of a pass
constexpr uint32_t kGroupBuckets = 1u << kGroupDigitBits;
static_assert(kGroupBuckets <= 2 * kBlock, "lane t owns the digit values 2 t and 2 t + 1 in the per-value steps");
static_assert(kGroupTile <= 65536, "group_one_kernel keeps its indices in 16 bits");
static_assert(kWavesPerBlock == 4, "a tile's four wave counts of a value are one 16 B piece");

// Bits of the largest key, max_id + 2 (max_id <= MTCP_GPU_FLOWTAB_MAX_ID): 2 .. 32.
__host__ __device__ inline uint32_t group_key_bits(uint32_t max_id) {
    return 32u - (uint32_t)__builtin_clz(max_id + 2u);
}
__host__ __device__ inline uint32_t group_passes(uint32_t key_bits) {
    return (key_bits + kGroupDigitBits - 1) / kGroupDigitBits;
}
// Digit p of `passes`: the key bits spread evenly, the wider digits first.
struct GroupDigit {
    uint32_t shift, bits;
};
__host__ __device__ inline GroupDigit group_digit(uint32_t key_bits, uint32_t passes, uint32_t p) {
    const uint32_t q = key_bits / passes, r = key_bits % passes;
    return GroupDigit{p * q + (p < r ? p : r), q + (p < r ? 1u : 0u)};
}

// The workspace of a batch above kGroupTile, every part 16 B aligned: the
// pairs' arrays (keys twice and indices twice with three passes or more; with
// two the second index array is d_idx; with one only the sorted keys are
// kept), the counts of every digit value for every wave of every tile
// (value-major), the values' totals, the head counts of every wave and their
// total.  ntiles: tiles of kGroupSubTile.
struct GroupWork {
    bool one;                                                     // group_one_kernel: no workspace
    uint32_t ntiles, key_bits, passes;
    uint64_t key_off[2], idx_off[2], cnt_off, tot_off, seg_off, segtot_off, bytes;
};
inline GroupWork group_work(uint32_t n, uint32_t max_id) {
    GroupWork w{};
    w.one = n <= kGroupTile;
    w.ntiles = (n + kGroupSubTile - 1) / kGroupSubTile;
    w.key_bits = group_key_bits(max_id);
    w.passes = group_passes(w.key_bits);
    if (w.one) {
        w.bytes = 16;
        return w;
    }
    const uint64_t arr = (4ull * n + 15) & ~15ull;
    uint64_t off = 0;
    w.key_off[0] = off, off += arr;
    if (w.passes >= 2) {
        w.key_off[1] = off, off += arr;
        w.idx_off[0] = off, off += arr;
    }
    if (w.passes >= 3) w.idx_off[1] = off, off += arr;
    w.cnt_off = off, off += 16ull * kGroupBuckets * w.ntiles;
    w.tot_off = off, off += 4ull * kGroupBuckets;
    w.seg_off = off, off += 16ull * w.ntiles;
    w.segtot_off = off, off += 16;
    w.bytes = off;
    return w;
}

__device__ __forceinline__ uint32_t group_key(uint32_t sid, uint32_t max_id) {
    return sid <= max_id ? sid : max_id + (sid == MTCP_GPU_FLOW_MISS ? 1u : 2u);
}
__device__ __forceinline__ uint32_t group_sid(uint32_t key, uint32_t max_id) {
    return key <= max_id ? key : key == max_id + 1u ? MTCP_GPU_FLOW_MISS : MTCP_GPU_FLOW_NONE;
}

// Record of (tile, this lane's wave, round r) in a tile of R rounds: steer_pkt's order.
template <int R>
__device__ __forceinline__ uint32_t group_pkt(uint32_t tile, int r) {
    return tile * (kBlock * R) + (threadIdx.x / kWave) * (kWave * R) + (uint32_t)r * kWave +
           (threadIdx.x & (kWave - 1));
}

// The lanes of this wave with lane's digit d (every lane calls it; a lane that
// is not valid joins no group and gets 0): steer_group with the validity apart
// from the digit, since every value of a full-width digit is a real one.
__device__ __forceinline__ uint64_t group_match(uint32_t d, bool valid, uint32_t nbits) {
    uint64_t m = __ballot(valid);
    for (uint32_t b = 0; b < nbits; ++b) {
        const uint64_t v = __ballot((d >> b) & 1u);
        const uint32_t t = ((d >> b) & 1u) - 1u;                 // 0 where the bit is set, ~0 where not
        m &= v ^ (((uint64_t)t << 32) | t);
    }
    return valid ? m : 0ull;
}

// The keys (or the indices) of a lane's R records, round 0 first.
template <int R>
struct GroupKeys {
    uint32_t k[R];
};

__device__ __forceinline__ uint32_t group_digit_of(uint32_t key, uint32_t shift, uint32_t nbits) {
    return (key >> shift) & ((1u << nbits) - 1u);
}

// hist_w[v] += this wave's records with digit value v (hist zeroed, a barrier since).
template <int R>
__device__ __forceinline__ void group_wave_hist(const GroupKeys<R> &ks, uint32_t tile, uint32_t n, uint32_t shift,
                                                uint32_t nbits, uint32_t *hist_w) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t d = group_digit_of(ks.k[r], shift, nbits);
        const uint64_t m = group_match(d, group_pkt<R>(tile, r) < n, nbits);
        if (m && steer_rank(m) == 0) (void)steer_bump(&hist_w[d], (uint32_t)__popcll(m));
    }
}

// cur_w[v]: where this wave's next pair of digit value v goes.  The position of
// the pair of one round, or `limit` for a lane without one.
__device__ __forceinline__ uint32_t group_wave_pos(uint32_t key, bool valid, uint32_t shift, uint32_t nbits,
                                                   uint32_t *cur_w, uint32_t limit) {
    const uint32_t d = group_digit_of(key, shift, nbits);
    const uint64_t m = group_match(d, valid, nbits);
    const uint32_t rank = steer_rank(m);
    uint32_t base = 0;
    if (m && rank == 0) base = steer_bump(&cur_w[d], (uint32_t)__popcll(m));
    base = __shfl(base, m ? __ffsll((unsigned long long)m) - 1 : 0, kWave);    // from the group's lowest lane
    return m ? base + rank : limit;
}

template <int R, bool FIRST>
__device__ __forceinline__ void group_load_keys(GroupKeys<R> &ks, const uint32_t *__restrict__ src, uint32_t tile,
                                                uint32_t n, uint32_t max_id) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t pkt = group_pkt<R>(tile, r);
        uint32_t k = 0;
        if (pkt < n) k = FIRST ? group_key(src[pkt], max_id) : src[pkt];
        ks.k[r] = k;
    }
}

// ---- count ------------------------------------------------------------------
// grid: one workgroup per tile.  src: d_sid (FIRST) or the keys the pass before
// wrote; cnt[v * 4 * ntiles + 4 * tile + w]: wave w's records with digit value v.
template <bool FIRST>
__global__ __launch_bounds__(kBlock) void group_count_kernel(const uint32_t *__restrict__ src, uint32_t n,
                                                             uint32_t max_id, uint32_t shift, uint32_t nbits,
                                                             uint32_t *__restrict__ cnt, uint32_t ntiles) {
    __shared__ uint32_t hist[kWavesPerBlock][kGroupBuckets];
    const uint32_t tid = threadIdx.x, tile = blockIdx.x, nb = 1u << nbits;
    for (uint32_t v = tid; v < nb; v += kBlock) hist[0][v] = hist[1][v] = hist[2][v] = hist[3][v] = 0;
    GroupKeys<kGroupRounds> ks;
    group_load_keys<kGroupRounds, FIRST>(ks, src, tile, n, max_id);
    __syncthreads();
    group_wave_hist<kGroupRounds>(ks, tile, n, shift, nbits, hist[tid / kWave]);
    __syncthreads();
    for (uint32_t v = tid; v < nb; v += kBlock)
        reinterpret_cast<uint4 *>(cnt)[(uint64_t)v * ntiles + tile] =
            make_uint4(hist[0][v], hist[1][v], hist[2][v], hist[3][v]);
}

// ---- scan -------------------------------------------------------------------
// grid: one workgroup per digit value (or one, for the head counts).  Its len4
// pieces of four counts (every wave of every tile) in, their exclusive prefix
// out; totals[v]: the value's total.  A lane takes four pieces a step.
__global__ __launch_bounds__(kBlock) void group_scan_kernel(uint4 *__restrict__ cnt4, uint32_t len4,
                                                            uint32_t *__restrict__ totals) {
    uint4 *c = cnt4 + (uint64_t)blockIdx.x * len4;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < len4; base += 4 * kBlock) {
        uint4 v[4];
        uint32_t s = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t i = base + 4 * threadIdx.x + j;
            v[j] = i < len4 ? c[i] : make_uint4(0u, 0u, 0u, 0u);
            s += v[j].x + v[j].y + v[j].z + v[j].w;
        }
        uint32_t excl;
        const uint32_t tot = block_exclusive_scan(s, excl);
        uint32_t run = carry + excl;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t i = base + 4 * threadIdx.x + j;
            uint4 o;
            o.x = run, run += v[j].x;
            o.y = run, run += v[j].y;
            o.z = run, run += v[j].z;
            o.w = run, run += v[j].w;
            if (i < len4) c[i] = o;
        }
        carry += tot;
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

// ---- emit -------------------------------------------------------------------
// grid: one workgroup per tile.  cnt: scanned per value by group_scan_kernel.
// The pairs go to dst_key / dst_idx (the last pass: dst_idx = d_idx).
template <bool FIRST>
__global__ __launch_bounds__(kBlock) void group_emit_kernel(const uint32_t *__restrict__ src_key,
                                                            const uint32_t *__restrict__ src_idx, uint32_t n,
                                                            uint32_t max_id, uint32_t shift, uint32_t nbits,
                                                            const uint32_t *__restrict__ cnt,
                                                            const uint32_t *__restrict__ totals, uint32_t ntiles,
                                                            uint32_t *__restrict__ dst_key,
                                                            uint32_t *__restrict__ dst_idx) {
    constexpr int R = kGroupRounds;
    __shared__ uint32_t cur[kWavesPerBlock][kGroupBuckets];
    const uint32_t tid = threadIdx.x, tile = blockIdx.x, nb = 1u << nbits;
    GroupKeys<R> ks, is;
    group_load_keys<R, FIRST>(ks, src_key, tile, n, max_id);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t pkt = group_pkt<R>(tile, r);
        is.k[r] = FIRST ? pkt : pkt < n ? src_idx[pkt] : 0u;
    }
    // the values' starts (an exclusive scan of the totals): a lane's two values
    const uint32_t v0 = 2 * tid;
    const uint32_t t0 = v0 < nb ? totals[v0] : 0u, t1 = v0 + 1 < nb ? totals[v0 + 1] : 0u;
    uint32_t first;
    (void)block_exclusive_scan(t0 + t1, first);
#pragma unroll
    for (uint32_t j = 0; j < 2; ++j) {
        const uint32_t v = v0 + j;
        if (v < nb) {
            const uint4 c = reinterpret_cast<const uint4 *>(cnt)[(uint64_t)v * ntiles + tile];
            cur[0][v] = first + c.x;
            cur[1][v] = first + c.y;
            cur[2][v] = first + c.z;
            cur[3][v] = first + c.w;
        }
        first += t0;
    }
    __syncthreads();
    uint32_t *cur_w = cur[tid / kWave];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t p = group_wave_pos(ks.k[r], group_pkt<R>(tile, r) < n, shift, nbits, cur_w, n);
        if (p < n) {
            dst_key[p] = ks.k[r];
            dst_idx[p] = is.k[r];
        }
    }
}

// ---- segment table ------------------------------------------------------------
// key[n]: the sorted keys.  Position pos heads a segment when its key differs
// from its predecessor's.
__device__ __forceinline__ bool group_head(const uint32_t *__restrict__ key, uint32_t pos, uint32_t n) {
    return pos < n && (pos == 0 || key[pos] != key[pos - 1]);
}

// grid: one workgroup per tile.  segcnt[4 * tile + w]: the heads in wave w's chunk.
__global__ __launch_bounds__(kBlock) void group_seg_count_kernel(const uint32_t *__restrict__ key, uint32_t n,
                                                                 uint32_t *__restrict__ segcnt) {
    uint32_t c = 0;
#pragma unroll
    for (int r = 0; r < kGroupRounds; ++r)
        c += (uint32_t)__popcll(__ballot(group_head(key, group_pkt<kGroupRounds>(blockIdx.x, r), n)));
    if ((threadIdx.x & (kWave - 1)) == 0) segcnt[4 * blockIdx.x + threadIdx.x / kWave] = c;
}

// grid: one workgroup per tile.  segcnt: scanned by group_scan_kernel (one
// workgroup), segtot[0]: the number of heads.  Workgroup 0 also writes nseg[0]
// and seg_start[m].
__global__ __launch_bounds__(kBlock) void group_seg_emit_kernel(const uint32_t *__restrict__ key, uint32_t n,
                                                                uint32_t max_id,
                                                                const uint32_t *__restrict__ segcnt,
                                                                const uint32_t *__restrict__ segtot,
                                                                uint32_t *__restrict__ seg_sid,
                                                                uint32_t *__restrict__ seg_start,
                                                                uint32_t *__restrict__ nseg) {
    uint32_t base = segcnt[4 * blockIdx.x + threadIdx.x / kWave];
#pragma unroll
    for (int r = 0; r < kGroupRounds; ++r) {
        const uint32_t pos = group_pkt<kGroupRounds>(blockIdx.x, r);
        const bool h = group_head(key, pos, n);
        const uint64_t m = __ballot(h);
        const uint32_t j = base + steer_rank(m);
        if (h && j < n) {
            seg_sid[j] = group_sid(key[pos], max_id);
            seg_start[j] = pos;
        }
        base += (uint32_t)__popcll(m);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const uint32_t m = min(segtot[0], n);
        nseg[0] = m;
        seg_start[m] = n;
    }
}

// ---- n <= kGroupTile: everything in one workgroup -----------------------------
__global__ __launch_bounds__(kBlock) void group_one_kernel(const uint32_t *__restrict__ sid, uint32_t n,
                                                           uint32_t max_id, uint32_t *__restrict__ idx,
                                                           uint32_t *__restrict__ seg_sid,
                                                           uint32_t *__restrict__ seg_start,
                                                           uint32_t *__restrict__ nseg) {
    constexpr int R = kGroupOneRounds;
    __shared__ uint32_t cur[kWavesPerBlock][kGroupBuckets];
    __shared__ uint32_t skey[kGroupTile];
    __shared__ uint16_t sidx[kGroupTile];
    __shared__ uint32_t wheads[kWavesPerBlock];
    const uint32_t tid = threadIdx.x, wave = tid / kWave;
    const uint32_t key_bits = group_key_bits(max_id), passes = group_passes(key_bits);
    GroupKeys<R> ks, is;
    group_load_keys<R, true>(ks, sid, 0, n, max_id);
#pragma unroll
    for (int r = 0; r < R; ++r) is.k[r] = group_pkt<R>(0, r);
    for (uint32_t p = 0; p < passes; ++p) {
        const GroupDigit dg = group_digit(key_bits, passes, p);
        const uint32_t nb = 1u << dg.bits;
        for (uint32_t i = tid; i < kWavesPerBlock * kGroupBuckets; i += kBlock) (&cur[0][0])[i] = 0;
        __syncthreads();
        group_wave_hist<R>(ks, 0, n, dg.shift, dg.bits, cur[wave]);
        __syncthreads();
        const uint32_t v0 = 2 * tid;                              // a lane's two values
        uint32_t t0 = 0, t1 = 0;
#pragma unroll
        for (int w = 0; w < kWavesPerBlock; ++w) {
            if (v0 < nb) t0 += cur[w][v0];
            if (v0 + 1 < nb) t1 += cur[w][v0 + 1];
        }
        uint32_t run;
        (void)block_exclusive_scan(t0 + t1, run);
#pragma unroll
        for (uint32_t j = 0; j < 2; ++j) {
            const uint32_t v = v0 + j;
            if (v < nb) {
#pragma unroll
                for (int w = 0; w < kWavesPerBlock; ++w) {
                    const uint32_t c = cur[w][v];
                    cur[w][v] = run;
                    run += c;
                }
            }
        }
        __syncthreads();
        // the second walk recomputes its groups (steer_one_kernel has the reason)
#pragma unroll
        for (int r = 0; r < R; ++r) asm volatile("" : "+v"(ks.k[r]));
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const uint32_t q = group_wave_pos(ks.k[r], group_pkt<R>(0, r) < n, dg.shift, dg.bits, cur[wave], kGroupTile);
            if (q < kGroupTile) {
                skey[q] = ks.k[r];
                sidx[q] = (uint16_t)is.k[r];
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const uint32_t pos = group_pkt<R>(0, r);
            ks.k[r] = pos < n ? skey[pos] : 0u;
            is.k[r] = pos < n ? sidx[pos] : 0u;
        }
    }
    // the sorted keys are in skey (nothing writes it any more), a lane's own in ks
    uint32_t heads = 0;                                           // bit r: the record of round r heads a segment
    uint32_t c = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t pos = group_pkt<R>(0, r);
        if (pos < n) idx[pos] = is.k[r];
        const bool h = pos < n && (pos == 0 || ks.k[r] != skey[pos - 1]);
        heads |= (uint32_t)h << r;
        c += (uint32_t)__popcll(__ballot(h));
    }
    if ((tid & (kWave - 1)) == 0) wheads[wave] = c;
    __syncthreads();
    uint32_t base = 0, m_all = 0;
#pragma unroll
    for (int w = 0; w < kWavesPerBlock; ++w) {
        if (w < (int)wave) base += wheads[w];
        m_all += wheads[w];
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const bool h = (heads >> r) & 1u;
        const uint64_t m = __ballot(h);
        const uint32_t j = base + steer_rank(m);
        if (h && j < n) {
            seg_sid[j] = group_sid(ks.k[r], max_id);
            seg_start[j] = group_pkt<R>(0, r);
        }
        base += (uint32_t)__popcll(m);
    }
    if (tid == 0) {
        nseg[0] = min(m_all, n);
        seg_start[min(m_all, n)] = n;
    }
}

}  // namespace mg
