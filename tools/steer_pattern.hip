// steer_pattern.hip — the memory pattern of the steer passes
// (mtcp_amd/csrc/steer_kernels.hpp) without any ranking: the yardstick of
// tools/steer_bench.py.  Measurement infrastructure: nothing here is part of
// libmtcp_gpu.so.
//
// The same grids and the same traffic as the three passes (or the one
// workgroup of a batch of at most one tile): count loads one dword per record
// and parks one byte per packet, writes 4 L counts per tile; scan reads and
// rewrites one list's counts per workgroup; emit reads the parked bytes, the
// L totals and its 4 L counts and stores one 4 B index per packet, and, with
// descriptors, loads and stores 8 B per packet.  What differs: no ballot, no
// LDS counter, no rank: packet i's index goes to position i, so every store
// of a wave is one contiguous run.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr uint32_t kBlock = 256, kRounds = 16, kTile = kBlock * kRounds;

__device__ __forceinline__ uint32_t pkt_of(uint32_t tile, uint32_t r) {
    return tile * kTile + (threadIdx.x / 64) * (64 * kRounds) + r * 64 + (threadIdx.x & 63);
}

template <bool CMP>
__device__ __forceinline__ uint32_t rec_dword(const uint32_t *res, uint32_t i) {
    return res[CMP ? 4ull * i + 3 : 10ull * i + 9];
}

template <bool CMP>
__global__ __launch_bounds__(kBlock) void pattern_count(const uint32_t *__restrict__ res, uint32_t n, uint32_t L,
                                                        uint8_t *__restrict__ dest, uint32_t *__restrict__ cnt,
                                                        uint32_t ntiles) {
    uint32_t acc = 0;
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r) {
        const uint32_t pkt = pkt_of(blockIdx.x, r);
        if (pkt < n) {
            const uint32_t w = rec_dword<CMP>(res, pkt);
            dest[pkt] = (uint8_t)(w >> 8);
            acc += w;
        }
    }
    if (threadIdx.x < L)
        reinterpret_cast<uint4 *>(cnt)[(uint64_t)threadIdx.x * ntiles + blockIdx.x] = make_uint4(acc, acc, acc, acc);
}

__global__ __launch_bounds__(kBlock) void pattern_scan(uint32_t *__restrict__ cnt, uint32_t len,
                                                       uint32_t *__restrict__ totals) {
    uint32_t *c = cnt + (uint64_t)blockIdx.x * len;
    uint32_t acc = 0;
    for (uint32_t i = threadIdx.x; i < len; i += kBlock) {
        const uint32_t v = c[i];
        c[i] = v + 1;
        acc += v;
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = acc;
}

template <bool GATHER>
__global__ __launch_bounds__(kBlock) void pattern_emit(const uint8_t *__restrict__ dest, uint32_t n, uint32_t L,
                                                       const uint32_t *__restrict__ cnt,
                                                       const uint32_t *__restrict__ totals, uint32_t ntiles,
                                                       uint32_t *__restrict__ idx, uint32_t *__restrict__ start,
                                                       const uint2 *__restrict__ desc,
                                                       uint2 *__restrict__ desc_out) {
    uint32_t extra = 0;
    if (threadIdx.x < L) {
        const uint4 c = reinterpret_cast<const uint4 *>(cnt)[(uint64_t)threadIdx.x * ntiles + blockIdx.x];
        extra = totals[threadIdx.x] + c.x + c.y + c.z + c.w;
        if (blockIdx.x == 0) start[threadIdx.x] = extra;
    } else if (threadIdx.x == L && blockIdx.x == 0) {
        start[L] = n;
    }
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r) {
        const uint32_t pkt = pkt_of(blockIdx.x, r);
        if (pkt < n) {
            idx[pkt] = pkt + dest[pkt] + (extra >> 31);      // extra < 2^31: keeps its loads live
            if constexpr (GATHER) desc_out[pkt] = desc[pkt];
        }
    }
}

template <bool CMP, bool GATHER>
__global__ __launch_bounds__(kBlock) void pattern_one(const uint32_t *__restrict__ res, uint32_t n, uint32_t L,
                                                      uint32_t *__restrict__ idx, uint32_t *__restrict__ start,
                                                      const uint2 *__restrict__ desc,
                                                      uint2 *__restrict__ desc_out) {
    if (threadIdx.x <= L) start[threadIdx.x] = threadIdx.x == L ? n : 0u;
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r) {
        const uint32_t pkt = pkt_of(0, r);
        if (pkt < n) {
            idx[pkt] = pkt + (rec_dword<CMP>(res, pkt) >> 8);
            if constexpr (GATHER) desc_out[pkt] = desc[pkt];
        }
    }
}

}  // namespace

// The steer passes' pattern for n records of `compact` ? 16 : 40 bytes and
// L = Q + 1 lists, on `stream`; d_desc / d_desc_out both NULL or both given;
// d_work as mtcp_gpu_steer_work_bytes sizes it (same layout).  0, or -1 on a
// launch error.
extern "C" int steer_pattern_launch(const void *d_res, int compact, uint32_t n, uint32_t Q, void *d_idx,
                                    void *d_start, const void *d_desc, void *d_desc_out, void *d_work,
                                    void *stream) {
    if (!n) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const uint32_t *res = static_cast<const uint32_t *>(d_res);
    uint32_t *idx = static_cast<uint32_t *>(d_idx), *start = static_cast<uint32_t *>(d_start);
    const uint2 *desc = static_cast<const uint2 *>(d_desc);
    uint2 *dout = static_cast<uint2 *>(d_desc_out);
    const uint32_t L = Q + 1, ntiles = (n + kTile - 1) / kTile;
    const bool g = desc != nullptr;
    if (ntiles == 1) {
        if (compact) {
            if (g) hipLaunchKernelGGL((pattern_one<true, true>), dim3(1), dim3(kBlock), 0, st, res, n, L, idx, start, desc, dout);
            else hipLaunchKernelGGL((pattern_one<true, false>), dim3(1), dim3(kBlock), 0, st, res, n, L, idx, start, desc, dout);
        } else {
            if (g) hipLaunchKernelGGL((pattern_one<false, true>), dim3(1), dim3(kBlock), 0, st, res, n, L, idx, start, desc, dout);
            else hipLaunchKernelGGL((pattern_one<false, false>), dim3(1), dim3(kBlock), 0, st, res, n, L, idx, start, desc, dout);
        }
        return hipGetLastError() == hipSuccess ? 0 : -1;
    }
    uint8_t *work = static_cast<uint8_t *>(d_work);
    const uint64_t cnt_off = ((uint64_t)n + 15) & ~15ull;
    const uint64_t tot_off = cnt_off + 16ull * L * ntiles;
    uint32_t *cnt = reinterpret_cast<uint32_t *>(work + cnt_off);
    uint32_t *totals = reinterpret_cast<uint32_t *>(work + tot_off);
    if (compact)
        hipLaunchKernelGGL(pattern_count<true>, dim3(ntiles), dim3(kBlock), 0, st, res, n, L, work, cnt, ntiles);
    else
        hipLaunchKernelGGL(pattern_count<false>, dim3(ntiles), dim3(kBlock), 0, st, res, n, L, work, cnt, ntiles);
    hipLaunchKernelGGL(pattern_scan, dim3(L), dim3(kBlock), 0, st, cnt, 4 * ntiles, totals);
    if (g)
        hipLaunchKernelGGL(pattern_emit<true>, dim3(ntiles), dim3(kBlock), 0, st, work, n, L, cnt, totals, ntiles,
                           idx, start, desc, dout);
    else
        hipLaunchKernelGGL(pattern_emit<false>, dim3(ntiles), dim3(kBlock), 0, st, work, n, L, cnt, totals, ntiles,
                           idx, start, desc, dout);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
