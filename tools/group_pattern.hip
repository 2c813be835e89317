// group_pattern.hip — the memory pattern of the group passes
// (mtcp_amd/csrc/group_kernels.hpp) without any ranking: the yardstick of
// tools/group_bench.py.  Measurement infrastructure: nothing here is part of
// libmtcp_gpu.so.
//
// The same launches on the same grids with the same traffic as the passes (or
// the one workgroup of a batch of at most one tile).  Per radix pass: count
// loads one key per record and writes 4 counts per digit value and tile; scan
// reads and rewrites one value's counts per workgroup; emit loads the pair (the
// first pass: the id alone), the totals and its counts and stores the pair.
// Then the segment passes: two key loads per position and one count per wave,
// the scan, and two 4 B stores per segment head.  What differs: no ballot, no
// LDS counter, no rank: pair i goes to position i, so every store of a wave is
// one contiguous run, and a head's table entry goes to the head's own position.
// The segment passes read the SORTED keys a run of the library left in its
// workspace (group_pattern_sorted_off), so they see the same heads.  The
// one-workgroup form has no sorted keys to read: it takes the heads of the
// unsorted ids, which are more.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../mtcp_amd/csrc/group_kernels.hpp"

namespace {

using namespace mg;

template <bool FIRST>
__global__ __launch_bounds__(kBlock) void pattern_count(const uint32_t *__restrict__ src, uint32_t n, uint32_t nb,
                                                        uint32_t *__restrict__ cnt, uint32_t ntiles) {
    uint32_t acc = 0;
#pragma unroll
    for (int r = 0; r < kGroupRounds; ++r) {
        const uint32_t pkt = group_pkt<kGroupRounds>(blockIdx.x, r);
        if (pkt < n) acc += src[pkt];
    }
    for (uint32_t v = threadIdx.x; v < nb; v += kBlock)
        reinterpret_cast<uint4 *>(cnt)[(uint64_t)v * ntiles + blockIdx.x] = make_uint4(acc, acc, acc, acc);
}

__global__ __launch_bounds__(kBlock) void pattern_scan(uint4 *__restrict__ cnt4, uint32_t len4,
                                                       uint32_t *__restrict__ totals) {
    uint4 *c = cnt4 + (uint64_t)blockIdx.x * len4;
    uint32_t acc = 0;
    for (uint32_t base = 0; base < len4; base += 4 * kBlock) {
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t i = base + 4 * threadIdx.x + j;
            if (i < len4) {
                uint4 v = c[i];
                acc += v.x + v.y + v.z + v.w;
                v.x += 1;
                c[i] = v;
            }
        }
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = acc;
}

template <bool FIRST>
__global__ __launch_bounds__(kBlock) void pattern_emit(const uint32_t *__restrict__ src_key,
                                                       const uint32_t *__restrict__ src_idx, uint32_t n, uint32_t nb,
                                                       const uint32_t *__restrict__ cnt,
                                                       const uint32_t *__restrict__ totals, uint32_t ntiles,
                                                       uint32_t *__restrict__ dst_key,
                                                       uint32_t *__restrict__ dst_idx) {
    uint32_t extra = 0;
    for (uint32_t v = threadIdx.x; v < nb; v += kBlock) {
        const uint4 c = reinterpret_cast<const uint4 *>(cnt)[(uint64_t)v * ntiles + blockIdx.x];
        extra += totals[v] + c.x + c.y + c.z + c.w;
    }
    uint32_t k[kGroupRounds], x[kGroupRounds];
#pragma unroll
    for (int r = 0; r < kGroupRounds; ++r) {
        const uint32_t pkt = group_pkt<kGroupRounds>(blockIdx.x, r);
        k[r] = pkt < n ? src_key[pkt] : 0u;
        x[r] = FIRST ? pkt : pkt < n ? src_idx[pkt] : 0u;
    }
#pragma unroll
    for (int r = 0; r < kGroupRounds; ++r) {
        const uint32_t pkt = group_pkt<kGroupRounds>(blockIdx.x, r);
        if (pkt < n) {
            dst_key[pkt] = k[r] + (extra >> 31);             // extra < 2^31: keeps its loads live
            dst_idx[pkt] = x[r];
        }
    }
}

__global__ __launch_bounds__(kBlock) void pattern_seg_count(const uint32_t *__restrict__ key, uint32_t n,
                                                            uint32_t *__restrict__ segcnt) {
    uint32_t c = 0;
#pragma unroll
    for (int r = 0; r < kGroupRounds; ++r) c += group_head(key, group_pkt<kGroupRounds>(blockIdx.x, r), n);
    if ((threadIdx.x & (kWave - 1)) == 0) segcnt[4 * blockIdx.x + threadIdx.x / kWave] = c;
}

__global__ __launch_bounds__(kBlock) void pattern_seg_emit(const uint32_t *__restrict__ key, uint32_t n,
                                                           const uint32_t *__restrict__ segcnt,
                                                           const uint32_t *__restrict__ segtot,
                                                           uint32_t *__restrict__ seg_sid,
                                                           uint32_t *__restrict__ seg_start,
                                                           uint32_t *__restrict__ nseg) {
    const uint32_t base = segcnt[4 * blockIdx.x + threadIdx.x / kWave];
#pragma unroll
    for (int r = 0; r < kGroupRounds; ++r) {
        const uint32_t pos = group_pkt<kGroupRounds>(blockIdx.x, r);
        if (group_head(key, pos, n)) {
            seg_sid[pos] = key[pos] + (base >> 31);
            seg_start[pos] = pos;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        nseg[0] = segtot[0];
        seg_start[n] = n;
    }
}

__global__ __launch_bounds__(kBlock) void pattern_one(const uint32_t *__restrict__ sid, uint32_t n,
                                                      uint32_t *__restrict__ idx, uint32_t *__restrict__ seg_sid,
                                                      uint32_t *__restrict__ seg_start,
                                                      uint32_t *__restrict__ nseg) {
#pragma unroll
    for (int r = 0; r < kGroupOneRounds; ++r) {
        const uint32_t pos = group_pkt<kGroupOneRounds>(0, r);
        if (pos < n) idx[pos] = pos;
        if (group_head(sid, pos, n)) {
            seg_sid[pos] = sid[pos];
            seg_start[pos] = pos;
        }
    }
    if (threadIdx.x == 0) {
        nseg[0] = n;
        seg_start[n] = n;
    }
}

}  // namespace

// Where, in a workspace of mtcp_gpu_group_work_bytes(n, max_id) bytes, a run of
// mtcp_gpu_group_dev leaves its sorted keys (n above one tile).
extern "C" uint64_t group_pattern_sorted_off(uint32_t n, uint32_t max_id) {
    const mg::GroupWork w = mg::group_work(n, max_id);
    return w.key_off[(w.passes - 1) & 1];
}

// The group passes' pattern for n ids and stream numbers up to max_id, on
// `stream`; d_work as mtcp_gpu_group_work_bytes sizes it (same layout);
// d_sorted: the sorted keys of the same ids (NULL for n of at most one tile).
// 0, or -1 on a launch error.
extern "C" int group_pattern_launch(const void *d_sid, uint32_t n, uint32_t max_id, void *d_idx, void *d_seg_sid,
                                    void *d_seg_start, void *d_nseg, void *d_work, const void *d_sorted,
                                    void *stream) {
    if (!n) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const uint32_t *sid = static_cast<const uint32_t *>(d_sid), *sorted = static_cast<const uint32_t *>(d_sorted);
    uint32_t *idx = static_cast<uint32_t *>(d_idx), *seg_sid = static_cast<uint32_t *>(d_seg_sid);
    uint32_t *seg_start = static_cast<uint32_t *>(d_seg_start), *nseg = static_cast<uint32_t *>(d_nseg);
    const mg::GroupWork w = mg::group_work(n, max_id);
    const dim3 block(kBlock), tiles(w.ntiles);
    if (w.one) {
        hipLaunchKernelGGL(pattern_one, dim3(1), block, 0, st, sid, n, idx, seg_sid, seg_start, nseg);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    }
    uint8_t *work = static_cast<uint8_t *>(d_work);
    auto at = [&](uint64_t off) { return reinterpret_cast<uint32_t *>(work + off); };
    uint32_t *cnt = at(w.cnt_off), *totals = at(w.tot_off), *segcnt = at(w.seg_off), *segtot = at(w.segtot_off);
    const uint32_t *src_key = sid, *src_idx = nullptr;
    for (uint32_t p = 0; p < w.passes; ++p) {
        const uint32_t nb = 1u << mg::group_digit(w.key_bits, w.passes, p).bits;
        uint32_t *dst_key = at(w.key_off[p & 1]);
        uint32_t *dst_idx = p + 1 == w.passes ? idx : at(w.idx_off[p & 1]);
        if (p == 0) hipLaunchKernelGGL(pattern_count<true>, tiles, block, 0, st, src_key, n, nb, cnt, w.ntiles);
        else hipLaunchKernelGGL(pattern_count<false>, tiles, block, 0, st, src_key, n, nb, cnt, w.ntiles);
        hipLaunchKernelGGL(pattern_scan, dim3(nb), block, 0, st, reinterpret_cast<uint4 *>(cnt), w.ntiles, totals);
        if (p == 0)
            hipLaunchKernelGGL(pattern_emit<true>, tiles, block, 0, st, src_key, src_idx, n, nb, cnt, totals, w.ntiles,
                               dst_key, dst_idx);
        else
            hipLaunchKernelGGL(pattern_emit<false>, tiles, block, 0, st, src_key, src_idx, n, nb, cnt, totals,
                               w.ntiles, dst_key, dst_idx);
        src_key = dst_key;
        src_idx = dst_idx;
    }
    hipLaunchKernelGGL(pattern_seg_count, tiles, block, 0, st, sorted, n, segcnt);
    hipLaunchKernelGGL(pattern_scan, dim3(1), block, 0, st, reinterpret_cast<uint4 *>(segcnt), w.ntiles, segtot);
    hipLaunchKernelGGL(pattern_seg_emit, tiles, block, 0, st, sorted, n, segcnt, segtot, seg_sid, seg_start, nseg);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
